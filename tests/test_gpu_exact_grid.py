"""The grid steps on exact operands, element by element: one update() of nmf_algorithms_1D / _2D per kind of tests/_exact.py GRID_KINDS on
every grid and shape of GRID_EXACT, through the Python choreography and through the library-sequenced step (dnmf_*_step_{1d,2d},
csrc/dnmf_grid.hip; on 1D grids also with the direct allreduce over the peer regions, on row grids also with the H phase cut into
chunks).  Every sum that crosses ranks is exact in any order, so a ragged 2 x 3 grid must give the bits of one rank: each rank's slice
is held to the whole-matrix answer (tests/_mp.py `_exact_check`):
  fro, fro_bf16   new W equal; new H within 3 ulps of the float64 quotient (mu_quot, then the factor); also with the clamp
  kl_wfixed       W unchanged; H within 2 ulps (kl_update_h: one IEEE division, one product -- the choreography and dnmf_mu_kl_step_{1d,2d} alike)
  kl_w            W within 2 ulps (kl_update_w); H within 1e-5 of each element of the float64 step from the gathered new W
  kl_fixed        W and H come back bit for bit
  hals, hals_bf16 new W equal; H finite, >= eps and within the generator's derived bound H_err (loose from k of about 16 on)
  hals_wfixed     W unchanged; new H equal
One test per grid: all its cases share ONE set of rank processes (a GPU process takes seconds to start, a step milliseconds).
tests/test_exact_grid_cpu.py runs the same cases through the checker back end without a GPU."""
import pytest

from tests import _exact as ex
from tests.conftest import long_param

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry", [long_param(e, id=e[0]) if e[4] else pytest.param(e, id=e[0]) for e in ex.GRID_EXACT])
def test_grid_steps_on_exact_operands(entry):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tests._mp import run_exact_cases
    done = run_exact_cases(entry[1], ex.grid_exact_cases(entry), use_hip=True, timeout=150)
    print("%s: per rank %s" % (entry[0], done[0]))
