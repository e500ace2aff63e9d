"""The workspace contract of include/dnmf.h (size, state, bounds, alignment) for the beta-divergence entry points, dnmf_beta_*: the
driver, the guard and the runs of tests/test_gpu_workspace.py (poisoned, zeroed, 0x7F-filled and leftover workspaces of exactly the
query, four times the query, a 16-byte base) over a case table of this family's own.  tests/test_beta_workspace_cpu.py holds the table
to pydnmfk_amd._lib.BETA_SIGNATURES: no launching entry point of the family is left out.

  beta-*     the pairs at beta = 2 on exact operands (P = exp2 of an exact zero = 1: tests/_beta.py::exact), the updates and the
             divergence at beta = 0.5 (gamma = 2 / 3) within 1e-5 of float64 (tests/test_gpu_beta.py)
  beta-fit   a 12-step whole fit at beta = 0.5 against the float64 statement"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _is as I  # noqa: E402
from tests import test_gpu_workspace as G  # noqa: E402
from tests.test_gpu_workspace import env  # noqa: E402,F401  (the module's fixture: engine and library on cuda:0)

EPS = G.EPS
BETA_NAMES = ("dnmf_beta_aht_pair", "dnmf_beta_wta_pair", "dnmf_beta_update_w", "dnmf_beta_update_h", "dnmf_beta_divergence")


def _beta_case(shape, k):
    m, n = shape

    def make(engine, lib):
        from tests import _beta as B
        from tests import test_gpu_beta as tb
        ops = engine.HIP_OPS
        A, W, H, ref = B.exact_problem(m, n, k, 2.0)
        exp = tb._expected(A, W, H, 0.5)
        Ap, Wp, Hp = G._P(A), G._P(W), G._P(H)

        @G._nout(8)
        def call():
            out = []
            for side, (r, c) in (("w", (m, k)), ("h", (k, n))):
                num, den = G._out(r, c), G._out(r, c)
                ops.beta_pair_into(side, Ap.view, Wp.view, Hp.view, EPS, 2.0, num.view, den.view)
                out += [num.check("beta %s num" % side), den.check("beta %s den" % side)]
            W1, H1, H2 = G._P(W), G._P(H), G._P(H)
            ops.beta_update_w(Ap.view, W1.view, Hp.view, EPS, 0.5)
            ops.beta_update_h(Ap.view, Wp.view, H1.view, EPS, 0.5)
            ops.beta_update_h(Ap.view, Wp.view, H2.view, EPS, 0.5, clamp=True)
            div = ops.beta_divergence(Ap.view, Wp.view, Hp.view, EPS, 0.5)
            return out + [W1.check("W1"), H1.check("H1"), H2.check("H2"), div.cpu().numpy()]

        def chk(nw, dw, nh, dh, w1, h1, h2, div, w):
            for g, r_, name in zip((nw, dw, nh, dh), ref["w"] + ref["h"], ("num_w", "den_w", "num_h", "den_h")):
                assert np.array_equal(g.astype(np.float64), r_), "%s %s: %d elements differ from the exact answer" % (w, name, int((g != r_).sum()))
            du = [tb._rel(w1, exp["W"]), tb._rel(h1, exp["H"]), tb._rel(h2, np.maximum(exp["H"], EPS))]
            dd = abs(float(div[0]) - exp["div"]) / exp["scale"]
            assert max(du) <= tb.BOUND and dd <= tb.BOUND, (w, du, dd)
        S = G.Steps()
        S.add("beta", call, chk)
        return S.prob()
    return G.Case("beta-%dx%d-k%d" % (m, n, k), BETA_NAMES, make, align16=True, query=lambda lib: {lib.dnmf_beta_ws_bytes(m, n, k)})


def _beta_fit_case():
    def make(engine, lib):
        from tests import _beta as B
        from tests import test_gpu_beta as tb
        from tests._golden import rel_fro
        A, W0, H0, k = tb._fit_problem()
        Wr, Hr, err_r = B.fit(A, W0, H0, 0.5, G.FIT_ITR)

        @G._nout(3)
        def fit():
            Ad, W, H = G._dev(A), G._dev(W0), G._dev(H0)
            sq = engine.HIP_OPS.beta_fit(Ad, W, H, EPS, 0.5, True, G.FIT_ITR)
            return W.cpu().numpy(), H.cpu().numpy(), sq.cpu().numpy()

        def chk(w_, h_, sq, w):
            err = float(np.sqrt(sq[0, 0] / sq[0, 1]))
            dw, dh, de = rel_fro(w_, Wr), rel_fro(h_, Hr), abs(err - err_r) / err_r
            assert dw <= tb.FIT_BOUND and dh <= tb.FIT_BOUND and de <= tb.ERR_BOUND, (w, dw, dh, de)
        fit.free = (2,)
        S = G.Steps()
        S.add("beta fit, %d steps" % G.FIT_ITR, fit, chk)
        return S.prob()
    return G.Case("beta-fit", ("dnmf_beta_mu_fit",), make, align16=True, query=lambda lib: {lib.dnmf_beta_ws_bytes_fit(200, 136, 5)})


CASES = [_beta_case(s, k) for s in (I.EXACT_SHAPES[0], I.EXACT_LOOP_CASES[0]["shape"]) for k in (3, 128)] + [_beta_fit_case()]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_beta_workspace_contract(env, case):  # noqa: F811
    G.test_workspace_contract(env, case)
