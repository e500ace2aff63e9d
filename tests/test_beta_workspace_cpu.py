"""The workspace contract of include/dnmf.h for the beta-divergence entry points, what can be held without a GPU (the checks of
tests/test_workspace_cpu.py and tests/test_capi.py for the core table, over this family's table pydnmfk_amd._lib.BETA_SIGNATURES):

  * the family's ABI: every dnmf_beta_* function that include/dnmf_beta_api.h declares is exported and bound, and nothing else is in the
    table; include/dnmf.h includes that header;
  * completeness: every entry point of the table that takes `(ws, ws_bytes)` is reached by a case of tests/test_gpu_beta_workspace.py;
  * a misaligned workspace is refused with DNMF_EWS as the FIRST check (every other argument is made up);
  * the queries of the case table answer."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")

from pydnmfk_amd import _lib  # noqa: E402
from tests import test_gpu_beta_workspace as GB  # noqa: E402
from tests.test_capi import EWS, ODD, P16  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = _lib.lib


def ws_taking():
    """the names of BETA_SIGNATURES whose argument list holds c_void_p followed by c_size_t"""
    return [name for name, args in _lib.BETA_SIGNATURES.items()
            if any(args[i] is ctypes.c_void_p and args[i + 1] is ctypes.c_size_t for i in range(len(args) - 1))]


def test_the_family_header_is_part_of_the_abi_and_bound():
    txt = open(os.path.join(ROOT, "include", "dnmf_beta_api.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(dnmf_[a-z0-9_]+)\s*\(", txt)))
    assert len(names) == 10 and all(n.startswith("dnmf_beta_") for n in names), names
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), "symbol %s declared in include/dnmf_beta_api.h but not exported" % n
        assert callable(getattr(lib, n))
    assert sorted(_lib.BETA_SIGNATURES) == names and not set(_lib.BETA_SIGNATURES) & set(_lib.SIGNATURES)
    core = open(os.path.join(ROOT, "include", "dnmf.h")).read()
    assert '#include "dnmf_beta_api.h"' in re.sub(r"/\*.*?\*/", "", core, flags=re.S)


def test_every_ws_taking_entry_point_is_in_the_case_table():
    names = ws_taking()
    assert len(names) == 6, names                              # the two pairs, the two updates, the divergence, the whole fit
    covered = {n for c in GB.CASES for n in c.names}
    assert covered == set(names), (sorted(covered), sorted(names))
    ids = [c.id for c in GB.CASES]
    assert len(ids) == len(set(ids)) and all(c.query is not None and c.align16 for c in GB.CASES)


def test_a_misaligned_workspace_is_refused_before_anything_else():
    """the loop of tests/test_capi.py over this family: a pointer nothing may dereference and 8 for every integer, so a refusal that came
    later would be another one, or a fault"""
    for name in ws_taking():
        args = _lib.BETA_SIGNATURES[name]
        at = next(i for i in range(len(args) - 1) if args[i] is ctypes.c_void_p and args[i + 1] is ctypes.c_size_t)
        call = [P16 if a is ctypes.c_void_p else 1 << 20 if a is ctypes.c_size_t else 1e-7 if a in (ctypes.c_float, ctypes.c_double) else 8
                for a in args]
        for odd in (ODD, P16 + 8, P16 + 1):
            call[at] = odd
            rc = getattr(lib, name)(*call)
            err = lib.dnmf_last_error()
            assert rc == EWS and b"16-byte boundary" in err, "%s with ws at %#x returned %d (%r)" % (name, odd, rc, err)


@pytest.mark.parametrize("case", GB.CASES, ids=lambda c: c.id)
def test_the_queries_of_the_case_table_answer(case):
    sizes = {int(q) for q in case.query(lib)}
    assert sizes and all(q > 0 for q in sizes), (case.id, sizes)
