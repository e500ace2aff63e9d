"""The grid exact tier without a GPU: every grid, shape and kind of tests/_exact.py GRID_EXACT through the Python choreography of
pydnmfk_amd/dist_nmf.py with the checker back end (tests/_ops_double.py) under gloo -- the same harness and the same assertions as
tests/test_gpu_exact_grid.py (tests/_mp.py run_exact_cases, use_hip=False).  It proves the expected values, the slicing and the
harness before a GPU sees them, and holds the choreography itself -- packed offsets, chunk spans, re-blocking copies, gathers -- to
exact operands: every sum that crosses ranks is exact in any order, so each rank's slice must equal the whole-matrix answer."""
import pytest

from tests import _exact as ex
from tests.conftest import long_param


@pytest.mark.parametrize("entry", [long_param(e, id=e[0]) if e[4] else pytest.param(e, id=e[0]) for e in ex.GRID_EXACT])
def test_grid_choreography_on_exact_operands(entry):
    from tests._mp import run_exact_cases
    done = run_exact_cases(entry[1], ex.grid_exact_cases(entry, cpu=True), use_hip=False, timeout=300)
    print("%s: per rank %s" % (entry[0], done[0]))
