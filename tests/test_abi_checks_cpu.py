"""The argument-check layer of every AOT entry point, without a GPU (include/minddet_hip.h "Conventions": the checks complete before
any device or runtime call).  From each valid row of tests/abi_cases.py this derives calls with ONE defect (tests/abi_derive.py:
mutations), makes them in-process with dummy host pointers (a refused call never dereferences a tensor pointer) and expects rc 1 for a
wrong parameter count and rc 2 for everything else (refuse_single_defects; each feature's test file does the same with its own table).
The rule that no operand silently contributes no defect is held over the rows of every table (all_rows).
tests/test_abi_accept_gpu.py shows on the GPU that the unmutated rows are accepted."""
import glob
import importlib
import os
import re

import pytest

from minddet_amd import _lib
from tests.abi_cases import CASES
from tests.abi_derive import KINDS, all_rows, mutations, rank_defects, refuse_single_defects
from tests.abi_header import aot_symbols, header

ROWS = all_rows()


def test_table_has_a_row_for_every_declared_symbol():
    main = set(aot_symbols(header("minddet_hip.h")))
    declared = [n for n in _lib.exported_symbols() if n in main]
    assert len(declared) == 53, len(declared)
    rows = {c.sym for c in CASES}
    assert not set(declared) - rows, f"no abi_cases row for {sorted(set(declared) - rows)}"
    assert not rows - set(declared), f"rows for undeclared symbols {sorted(rows - set(declared))}"
    assert len({c.id for c in CASES}) == len(CASES)


def test_every_table_is_collected():
    """a table that stops being collected fails here instead of vanishing, and so does a row that no single-defect test is made from:
    every row of every table is handed to refuse_single_defects by a parametrised test of some tests/test_*_cpu.py (the main table's
    by this file, a feature's by its own file, where the ids have always been)"""
    assert len(ROWS) == 163 and len({(table, case.id) for table, case in ROWS}) == 163 and len({case.sym for _, case in ROWS}) == 103
    assert {table for table, _ in ROWS} == set(KINDS) and len(KINDS) == 21
    wrapper = re.compile(r'''@pytest\.mark\.parametrize\("case", (\w+), ids=\[c\.id for c in \1\]\)
def test_single_defect_calls_are_refused_\w+\(case\):
    refuse_single_defects\("(\w+)", case\)
''')
    handed = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_*_cpu.py"))):
        for rows, table in wrapper.findall(open(path).read()):
            handed.setdefault(table, []).extend(c.id for c in getattr(importlib.import_module("tests." + table), rows))
    for table in KINDS:
        assert sorted(handed.get(table, [])) == sorted(case.id for t, case in ROWS if t == table), table


def test_every_required_operand_contributes_every_applicable_defect():
    """nothing can be left out silently: per op and operand, count the derived calls of each kind against what the row's flags make applicable"""
    for _, case in ROWS:
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
    refuse_single_defects("abi_cases", case)
