"""The argument-check layer of every AOT entry point, without a GPU (include/minddet_hip.h "Conventions": the checks complete before
any device or runtime call).  From each valid row of tests/abi_cases.py this derives calls with ONE defect, makes them in-process with
dummy host pointers (a refused call never dereferences a tensor pointer) and expects rc 1 for a wrong parameter count and rc 2 for
everything else.  tests/test_abi_accept_gpu.py shows on the GPU that the unmutated rows are accepted."""
import ctypes as C
import re

import pytest

from minddet_amd import _lib
from tests.abi_cases import CASES
from tests.abi_derive import ITEM, WRONG_DTYPE, Call, _numel, mutations, rank_defects  # noqa: F401 (other tests import them from here)


def aot_symbols():
    hdr = open(_lib.LIB_PATH.replace("minddet_amd/" + _lib.LIB_PATH.split("/")[-1], "include/minddet_hip.h")).read()
    aot = set(re.findall(r"^\s*int\s+(\w+)\s*\(MD_AOT_ARGS\)\s*;", hdr, flags=re.M))
    return [n for n in _lib.exported_symbols() if n in aot]


def test_table_has_a_row_for_every_declared_symbol():
    declared = aot_symbols()
    assert len(declared) == 53, len(declared)
    rows = {c.sym for c in CASES}
    assert not set(declared) - rows, f"no abi_cases row for {sorted(set(declared) - rows)}"
    assert not rows - set(declared), f"rows for undeclared symbols {sorted(rows - set(declared))}"
    assert len({c.id for c in CASES}) == len(CASES)


def test_every_required_operand_contributes_every_applicable_defect():
    """nothing can be left out silently: per op and operand, count the derived calls of each kind against what the row's flags make applicable"""
    for case in CASES:
        got = {}
        for kind, i, _, _ in mutations(case):
            got.setdefault(i, set()).add(kind)
        assert {"nparam", "params_null", "ndims_null", "shapes_null"} <= got[None], case.id
        assert ("extra_null" in got[None]) == case.extra_required, case.id
        for i, t in enumerate(case.operands):
            if t.null:
                continue
            want = {"dtype"}
            if t.kind == "req":
                want |= {"shape_null", "ptr_null"}
                if t.rank == "exact":
                    want |= {"rank-1", "rank+1"}
                elif t.rank == "min":
                    want |= {"rank-1"}
                else:
                    assert t.why, (case.id, i)
            elif t.kind == "loose":
                want |= {"ptr_null"}
                assert t.why, (case.id, i)
            else:
                want |= {k for k, _ in rank_defects(t)}
            assert want <= got.get(i, set()), (case.id, i, sorted(want - got.get(i, set())))
        assert any("rank_without_dtypes" in k for k in got.values()), case.id


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_single_defect_calls_are_refused_with_the_documented_code(case):
    if not __import__("os").path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = C.CDLL(_lib.LIB_PATH)
    bad = []
    for kind, i, call, want in mutations(case):
        rc = call.run(lib)          # the process surviving every one of these is part of the assertion
        if rc != want:
            bad.append((kind, i, rc, want))
    assert not bad, f"{case.id}: (defect, operand, rc, expected) {bad}"
