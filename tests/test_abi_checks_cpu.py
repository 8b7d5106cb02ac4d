"""The argument-check layer of every AOT entry point, without a GPU (include/minddet_hip.h "Conventions": the checks complete before
any device or runtime call).  From each valid row of tests/abi_cases.py this derives calls with ONE defect, makes them in-process with
dummy host pointers (a refused call never dereferences a tensor pointer) and expects rc 1 for a wrong parameter count and rc 2 for
everything else.  tests/test_abi_accept_gpu.py shows on the GPU that the unmutated rows are accepted."""
import ctypes as C
import re

import pytest

from minddet_amd import _lib
from tests.abi_cases import CASES

ITEM = {"float32": 4, "bfloat16": 2, "int32": 4, "int64": 8, "uint8": 1}
WRONG_DTYPE = b"float64"    # no operand of any op is float64


def aot_symbols():
    hdr = open(_lib.LIB_PATH.replace("minddet_amd/" + _lib.LIB_PATH.split("/")[-1], "include/minddet_hip.h")).read()
    aot = set(re.findall(r"^\s*int\s+(\w+)\s*\(MD_AOT_ARGS\)\s*;", hdr, flags=re.M))
    return [n for n in _lib.exported_symbols() if n in aot]


class Call:
    """the C arrays of one call; every field can be replaced before `run`"""

    def __init__(self, case):
        self.case = case
        ops = case.operands
        self.n = len(ops)
        self.shapes = [list(t.shape) for t in ops]
        self.dtypes = [None if t.null else t.dtype.encode() for t in ops]
        self.null_ptr = [t.null for t in ops]
        self.null_shape = [False] * self.n
        self.params_null = self.ndims_null = self.shapes_null = self.dtypes_null = self.extra_null = False

    def run(self, lib):
        n = self.n
        # one host block per operand, disjoint and as large as the tensor (md_c3_pair / md_conv2d_grouped compare address ranges)
        sizes = [max(64, ITEM[t.dtype] * max(1, _numel(t.shape)) + 64) for t in self.case.operands] + [64] * (n - len(self.case.operands))
        arena = (C.c_char * sum(sizes))()
        base, off = C.addressof(arena), 0
        params = (C.c_void_p * n)()
        ndims = (C.c_int * n)()
        shapes = (C.POINTER(C.c_int64) * n)()
        dtypes = (C.c_char_p * n)()
        keep = []
        for i in range(n):
            described = i < len(self.shapes)
            null = described and self.null_ptr[i]
            params[i] = None if null else base + off
            off += sizes[i]
            shp = ([] if self.case.operands[i].null else self.shapes[i]) if described else [64]
            ndims[i] = len(shp)
            buf = (C.c_int64 * max(len(shp), 1))(*shp)
            keep.append(buf)
            shapes[i] = None if (described and self.null_shape[i]) else C.cast(buf, C.POINTER(C.c_int64))
            dtypes[i] = self.dtypes[i] if described else b"uint8"
        extra = None if (self.case.extra is None or self.extra_null) else C.byref(self.case.extra)
        return getattr(lib, self.case.sym)(n, None if self.params_null else params, None if self.ndims_null else ndims,
                                           None if self.shapes_null else shapes, None if self.dtypes_null else dtypes, None, extra)


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def rank_defects(t):
    """the shapes a rank +- 1 defect of operand t gives, per abi_cases' `rank` kinds"""
    if t.kind == "loose" or t.rank == "free":
        return []
    out = [("rank-1", list(t.shape[:-1]))]
    if t.rank == "exact":
        out.append(("rank+1", list(t.shape) + [2]))
    return out


def mutations(case):
    """-> [(kind, operand index or None, Call, expected rc)]"""
    out = []
    lo, hi = min(case.nparam), max(case.nparam)
    for n in sorted({lo - 1, hi + 1} | {k for k in range(lo, hi) if k not in case.nparam}):
        c = Call(case)
        c.n = n
        if n < len(case.operands):
            c.shapes, c.dtypes, c.null_ptr, c.null_shape = c.shapes[:n], c.dtypes[:n], c.null_ptr[:n], c.null_shape[:n]
        out.append(("nparam", None, c, 1))
    for field in ("params_null", "ndims_null", "shapes_null"):
        c = Call(case)
        setattr(c, field, True)
        out.append((field, None, c, 2))
    if case.extra_required:
        c = Call(case)
        c.extra_null = True
        out.append(("extra_null", None, c, 2))
    first_rank = True
    for i, t in enumerate(case.operands):
        if t.null:
            continue            # an optional operand the valid row leaves out: nothing about it is looked at
        if t.kind == "req":
            c = Call(case)
            c.null_shape[i] = True
            out.append(("shape_null", i, c, 2))
        if t.kind != "opt":
            c = Call(case)
            c.null_ptr[i] = True
            out.append(("ptr_null", i, c, 2))
        c = Call(case)
        c.dtypes[i] = WRONG_DTYPE
        out.append(("dtype", i, c, 2))
        for kind, shp in rank_defects(t):
            c = Call(case)
            c.shapes[i] = shp
            out.append((kind, i, c, 2))
            if first_rank:      # an undescribed dtype passes: the same rank defect with dtypes == NULL is still refused by the rank
                first_rank = False
                c = Call(case)
                c.shapes[i] = shp
                c.dtypes_null = True
                out.append(("rank_without_dtypes", i, c, 2))
    return out


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
