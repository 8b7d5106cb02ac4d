"""The call side of the ABI tests, stated once.  From the rows of the tests/abi_cases*.py tables: the single-defect calls (Call,
mutations) and the test that makes them in-process (refuse_single_defects, with the kinds each table's rows must give rise to);
the edit kit with which a feature's own test states its semantic
refusals (lib_handle, edited, rc, raw and the edit constructors attr, item, shape, both); and the same calls written as lines of a
case file for the host replay program of tests/host/ (tests/test_host_replay_cpu.py), together with that test's hostile extents.
tests/abi_header.py is the header side."""
import copy
import ctypes as C
import functools
import os

ITEM = {"float32": 4, "float64": 8, "bfloat16": 2, "int32": 4, "int64": 8, "uint8": 1}


def wrong_dtype(t):
    """a dtype operand t does not have: float64, and float32 for a float64 operand"""
    return b"float32" if t.dtype == "float64" else b"float64"


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
        c.dtypes[i] = wrong_dtype(t)
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


# table -> the defects every one of its rows must give rise to, whatever its operands are (the main table has rows without a rank defect).
# A new table gets its line here and a parametrised test over its rows that calls refuse_single_defects; tests/test_abi_checks_cpu.py
# fails for a table that lacks either
_EVERY = frozenset({"nparam", "params_null", "ndims_null", "shapes_null", "shape_null", "ptr_null", "dtype", "rank-1", "rank+1"})
KINDS = {"abi_cases": frozenset()}
KINDS.update({"abi_cases_" + t: _EVERY for t in ("chain", "cocoeval", "cpaug", "kitti", "kittieval", "pcaug")})
KINDS.update({"abi_cases_" + t: _EVERY | {"extra_null"}
              for t in ("cn", "cnaug", "cp", "cploss", "cpsweeps", "cptargets", "nusceval", "points", "pp", "pploss", "ppreader")})
KINDS.update({"abi_cases_" + t: _EVERY | {"rank_without_dtypes", "extra_null"} for t in ("convbwd", "groupedbwd")})
KINDS["abi_cases_train"] = _EVERY | {"rank_without_dtypes"}      # (its rows without an attribute struct have no extra_null)


def refuse_single_defects(table, case):
    """the single-defect test of one row of `table`: every derived call, made in-process with dummy host pointers (a refused call never
    dereferences a tensor pointer), returns its documented code, and the kinds of KINDS[table] are all among them.  (This module is
    not assertion-rewritten by pytest: every assert carries its own message.)"""
    lib = lib_handle()
    muts = mutations(case)
    kinds = {k for k, _, _, _ in muts}
    assert KINDS[table] <= kinds, (case.id, sorted(KINDS[table] - kinds))
    assert ("extra_null" in kinds) == case.extra_required, case.id
    if table == "abi_cases_train":
        assert case.extra_required == (case.extra is not None), case.id
    bad = []
    for kind, i, call, expected in muts:
        got = call.run(lib)          # the process surviving every one of these is part of the assertion
        if got != expected:
            bad.append((kind, i, got, expected))
    assert not bad, f"{case.id}: (defect, operand, rc, expected) {bad}"


# ----- the edit kit: a feature's semantic refusals are edits of a valid row, made in-process
@functools.lru_cache(maxsize=None)
def lib_handle():
    """the library as a plain ctypes handle, built first if it is missing"""
    from minddet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return C.CDLL(_lib.LIB_PATH)


def edited(case, edit):
    """a Call of `case` after edit(copy of the case): the copy has its own attribute struct and operand list"""
    c = copy.copy(case)
    if case.extra is not None:
        c.extra = type(case.extra).from_buffer_copy(case.extra)
    c.operands = list(case.operands)
    edit(c)
    return Call(c)


def rc(case, edit):
    return edited(case, edit).run(lib_handle())


def raw(case, edit=None, same=(), shift=None):
    """the case's call after edit(copy) on dummy addresses 4 KiB apart and 4 KiB aligned (a refused call never dereferences a tensor
    pointer, so the extents may describe more memory than exists); same = [(o, k)]: operand o gets the address of operand k;
    shift = (o, bytes): operand o's address is moved by so many bytes -> rc"""
    call = edited(case, edit or (lambda c: None))
    ops, n = call.case.operands, call.n
    arena = (C.c_char * (4096 * (n + 2)))()
    base = (C.addressof(arena) + 4095) // 4096 * 4096
    addr = {i: base + 4096 * i for i in range(n)}
    for o, k in same:
        addr[o] = addr[k]
    if shift:
        addr[shift[0]] += shift[1]
    params, ndims = (C.c_void_p * n)(), (C.c_int * n)()
    shapes, dtypes = (C.POINTER(C.c_int64) * n)(), (C.c_char_p * n)()
    keep = []
    for i in range(n):
        params[i] = None if ops[i].null else addr[i]
        shp = [] if ops[i].null else list(ops[i].shape)
        ndims[i] = len(shp)
        keep.append((C.c_int64 * max(len(shp), 1))(*shp))
        shapes[i] = C.cast(keep[-1], C.POINTER(C.c_int64))
        dtypes[i] = None if ops[i].null else ops[i].dtype.encode()
    extra = None if call.case.extra is None else C.byref(call.case.extra)
    return getattr(lib_handle(), call.case.sym)(n, params, ndims, shapes, dtypes, None, extra)


def attr(name, v):
    return lambda c: setattr(c.extra, name, v)


def item(name, index, v):
    """element `index` of the array attribute `name`"""
    def edit(c):
        getattr(c.extra, name)[index] = v
    return edit


def shape(i, shp, dtype=None):
    """operand i with another shape (and dtype, where one is given); its kind, rank and why stay"""
    def edit(c):
        t = copy.copy(c.operands[i])
        t.shape, t.dtype = tuple(shp), dtype or t.dtype
        c.operands[i] = t
    return edit


def both(*edits):
    def edit(c):
        for e in edits:
            e(c)
    return edit


# ----- the same calls as lines of a case file for tests/host/replay (the format is described at the top of tests/host/replay.cpp)
# the hostile substitutions: a call that carries one is refused (1, 2 or 4, never 0)
HOSTILE = (-1, -2 ** 63, 2 ** 31, 2 ** 32, 2 ** 62, 2 ** 63 - 1)
WRAP_PAIRS = ((2 ** 32, 2 ** 32), (2 ** 31, 2 ** 33), (2 ** 33, 2 ** 31))      # products that wrap int64 to 0
WRAP_TRIPLE = (2 ** 21 + 1, 2 ** 21, 2 ** 22)     # wraps to 2^43, small and positive; each extent is below the cap of Args::tensor
# the probes: every extent below the cap of Args::tensor, so the op's own products are reached.  They wrap `int` to 0 / to 65536, or
# fit int64 only until the op multiplies by an element width.  An op without a size limit may take such a call (a probe is decided
# by membership in these sets, never by the range of a value: the triple above is hostile)
PROBE = (2 ** 31 - 1,)
PROBE_PAIRS = ((65536, 65536), (65537, 65536), (65536, 65537), (2 ** 31 - 1, 2 ** 31 - 1))
PROBE_TRIPLE = (2 ** 20, 2 ** 20, 2 ** 21)        # 2^61: fits int64, times 4 does not


def all_rows():
    """[(table, Case)] of every tests/abi_cases*.py table, in file order"""
    import glob
    import importlib
    here = os.path.dirname(os.path.abspath(__file__))
    rows = []
    for path in sorted(glob.glob(os.path.join(here, "abi_cases*.py"))):
        name = os.path.basename(path)[:-3]
        rows += [(name, c) for c in importlib.import_module("tests." + name).CASES]
    return rows


def workspace_index(case):
    """the index of the row's workspace operand (an optional trailing byte buffer), or None"""
    i = max(case.nparam) - 1
    if len(case.nparam) > 1 and len(case.operands) == i + 1:
        t = case.operands[i]
        if t.dtype == "uint8" and t.kind == "opt" and t.rank == "free" and len(t.shape) == 1:
            return i
    return None


def call_line(ident, call, stream=0):
    """one CALL line: what Call.run hands the entry point, with the data pointers as offsets into the replay's arena (one block per
    operand, disjoint, as large as the VALID row's tensor: md_c3_pair / md_conv2d_grouped compare address ranges)"""
    ops, n = call.case.operands, call.n
    sizes = [max(64, ITEM[t.dtype] * max(1, _numel(t.shape)) + 64) for t in ops] + [64] * (n - len(ops))
    sizes = [(s + 255) // 256 * 256 for s in sizes]
    words = ["CALL", ident.replace(" ", "_"), call.case.sym, str(stream), str(n),
             str(call.params_null * 1 + call.ndims_null * 2 + call.shapes_null * 4 + call.dtypes_null * 8),
             "-" if (call.case.extra is None or call.extra_null) else bytes(call.case.extra).hex()]
    off = 256
    for i in range(max(n, 0)):
        described = i < len(call.shapes)
        null = described and call.null_ptr[i]
        shp = ([] if ops[i].null else call.shapes[i]) if described else [64]
        dt = (call.dtypes[i] if described else b"uint8")
        words += ["N" if null else str(off), str(int(described and call.null_shape[i])), str(len(shp)), dt.decode() if dt else "-"]
        words += [str(int(v)) for v in shp]
        off += sizes[i]
    assert off < 1 << 30, ident
    return " ".join(words)


def substituted(case, table):
    """a Call of the row with every extent v of table replaced by table[v], in every operand but the workspace"""
    c = Call(case)
    ws = workspace_index(case)
    for i, t in enumerate(case.operands):
        if i != ws and not t.null:
            c.shapes[i] = [table.get(v, v) for v in t.shape]
    return c


def hostile_tables(case):
    """[(label, {extent: replacement}, probe)]: each distinct extent of the row by each hostile / probe value; each pair of distinct
    extents of one operand by the wrapping / probe pairs; each triple of distinct extents of one operand of rank >= 3 by the
    wrapping / probe triple.  probe: the substitution comes from the PROBE sets"""
    import itertools
    ws = workspace_index(case)
    shapes = [t.shape for i, t in enumerate(case.operands) if i != ws and not t.null]
    values = sorted({v for s in shapes for v in s})
    out = [(f"{v}->{h}", {v: h}, h in PROBE) for v in values for h in HOSTILE + PROBE]
    pairs, triples = set(), set()
    for s in shapes:
        distinct = sorted(set(s))
        pairs |= set(itertools.combinations(distinct, 2))
        if len(s) >= 3:
            triples |= set(itertools.combinations(distinct, 3))
    for a, b in sorted(pairs):
        out += [(f"{a},{b}->{x},{y}", {a: x, b: y}, (x, y) in PROBE_PAIRS) for x, y in WRAP_PAIRS + PROBE_PAIRS]
    for tr in sorted(triples):
        out += [(f"{tr}->{w}".replace(" ", ""), dict(zip(tr, w)), w is PROBE_TRIPLE) for w in (WRAP_TRIPLE, PROBE_TRIPLE)]
    return out
