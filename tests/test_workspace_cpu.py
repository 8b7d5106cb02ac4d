"""Scratch sizes have one owner (include/minddet_hip.h "Conventions"): every op that takes a workspace exports a host function
md_<op>_workspace_bytes, holds a caller's workspace to exactly that number, and Python asks it instead of mirroring a formula.  Without
a GPU: the functions are pure host code, and a call refused for its workspace never touches a tensor pointer (the dummy-pointer calls of
tests/abi_derive.py)."""
import copy
import ctypes as C
import glob
import itertools
import os
import re

import pytest

from minddet_amd import _lib, det_ops
from tests import (abi_cases, abi_cases_cn, abi_cases_cnaug, abi_cases_cp, abi_cases_cpaug, abi_cases_cploss, abi_cases_cpsweeps,
                   abi_cases_cptargets, abi_cases_kitti, abi_cases_pcaug, abi_cases_points, abi_cases_pploss, abi_cases_ppreader)
from tests.abi_cases import F, U8, T
from tests.abi_derive import Call
from tests.abi_header import defines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))}
DEFINES = defines(*HEADERS.values())
DECLARED = {name: args.count("int64_t") for txt in HEADERS.values()
            for name, args in re.findall(r"^int64_t (md_\w+)_workspace_bytes\(([^)]*)\);", txt, flags=re.M)}

# every entry point whose Python wrapper hands it a workspace -> the op whose function it uses (a _grad twin shares its forward's)
COVERED = {s: s for s in ("md_nms_aligned", "md_nms_rotated", "md_topk_segmented", "md_voxelize", "md_pp_anchor_mask", "md_pc_augment_points",
                          "md_cp_aug_count_points", "md_cp_aug_select", "md_cp_aug_points", "md_cp_sweeps_merge", "md_cp_assign_targets",
                          "md_cp_loss", "md_pp_loss", "md_cn_assign_targets", "md_cn_loss", "md_cn_aug_image", "md_pc_crop_hulls")}
COVERED.update(md_cp_loss_grad="md_cp_loss", md_pp_loss_grad="md_pp_loss", md_cn_loss_grad="md_cn_loss")


def ask(op, *dims):
    return _lib.workspace_bytes(op, *dims)


def cdiv(a, b):
    return (a + b - 1) // b


def test_every_declared_function_is_exported_and_every_covered_op_has_one():
    assert set(DECLARED) == set(COVERED.values())
    lib = _lib.lib()
    for name in DECLARED:
        assert hasattr(lib, name + "_workspace_bytes"), name
    for name, txt in HEADERS.items():     # each is declared in the header of its op, directly under it (under the _grad twin for the losses)
        for op in re.findall(r"^int64_t (md_\w+)_workspace_bytes\(", txt, flags=re.M):
            last = op + "_grad" if op + "_grad" in COVERED else op
            assert re.search(rf"^int {last}\(MD_AOT_ARGS\);[^\n]*\nint64_t {op}_workspace_bytes\(", txt, flags=re.M), (name, op)
    hip = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(ROOT, "minddet_amd", "csrc", "*.hip"))}
    for op in DECLARED:                   # defined once, in the file of the op
        assert [f'extern "C" int {op}(MD_AOT_ARGS)' in t or f"int {op[3:]}_entry(MD_AOT_ARGS" in t
                for t in hip.values() if f'extern "C" int64_t {op}_workspace_bytes(' in t] == [True], op
    # no entry point hands acquire arithmetic of its own, but the seven that no Python wrapper sizes a workspace for: the five
    # reference-ABI ops (three sites), md_circle_nms, md_assign_targets, md_anchor_mask and md_conv2d_head
    sized = re.compile(r"\.acquire\(\(size_t\)(w\.total|w\.flags|need|md_\w+_workspace_bytes\([\w, ]+\)), ")
    sites = [ln.strip() for t in hip.values() for ln in t.splitlines() if re.search(r"\b\w+\.acquire\(", ln)]
    assert len(sites) == 25 and sum(not sized.search(ln) for ln in sites) == 7, [ln for ln in sites if not sized.search(ln)]
    new = set(_lib.exported_symbols()) & {n + "_workspace_bytes" for n in DECLARED}
    assert new == {"md_nms_aligned_workspace_bytes", "md_topk_segmented_workspace_bytes"}      # those of minddet_hip.h


def test_a_negative_extent_answers_minus_one():
    lib = _lib.lib()
    for op, n in DECLARED.items():
        fn = getattr(lib, op + "_workspace_bytes")
        fn.restype, fn.argtypes = C.c_int64, [C.c_int64] * n
        assert fn(*[1] * n) >= 0, op
        for k in range(n):
            assert fn(*[-1 if j == k else 1 for j in range(n)]) == -1, (op, k)
        with pytest.raises(_lib.MindDetHipError):
            ask(op, *[-1] * n)


ROWS, BATCH, BOXES = (0, 1, 255, 256, 257, 300), (1, 2), (0, 3)
STRIP_CP, STRIP_PP, CHUNK_PP = DEFINES["MD_CP_LOSS_STRIP"], DEFINES["MD_PP_LOSS_STRIP"], DEFINES["MD_PP_LOSS_COUNT_CHUNK"]
STRIP_CN, CHUNK_CN, CHUNK_GREY = DEFINES["MD_CN_LOSS_STRIP"], DEFINES["MD_CN_LOSS_COUNT_CHUNK"], DEFINES["MD_CNAUG_GREY_CHUNK"]

# op -> (the sweep of its extents, the bound its header documents, True where the header says "at least": the formula is exact)
BOUNDS = {
    "md_nms_aligned": (itertools.product(BATCH, ROWS + (1023, 1024, 2048), (0, 100)),
                       lambda B, n, q: 8 * B * n * cdiv(n, 64) + 4 * B + 252, False),
    "md_nms_rotated": (itertools.product(BATCH, ROWS), lambda L, n: L * n * (20 * 4 + cdiv(n, 64) * 8), True),
    "md_voxelize": (itertools.product(ROWS, BATCH, (1, 100), (0, 3, 400)),
                    lambda N, B, cells, mv: 4 * (2 * B * cells + 3 * N + 2 * B * mv + (N + B * mv) // 1024) + 4096, False),
    "md_pp_anchor_mask": (itertools.product(BATCH, (1, 8, 300), (1, 7)), lambda B, gx, gy: B * gy * gx * 4, True),
    "md_pc_augment_points": (itertools.product(ROWS, BATCH, BOXES, BOXES),
                             lambda N, B, G, R: 128 * B * (G + R) + 64 * B + 4 * (N // 256 + 3), False),
    "md_cp_aug_count_points": (itertools.product(BATCH, BOXES), lambda B, G: 96 * B * G, False),
    "md_cp_aug_select": (itertools.product(BATCH, BOXES, (0, 4, 62)), lambda B, G, S: 8 * B * S * ((G + S + 63) // 64), False),
    "md_cp_aug_points": (itertools.product(ROWS, (0, 40), BATCH), lambda N, Ns, B: 64 * B + (N + Ns) + 4 * ((N + Ns) // 256 + 3), False),
    "md_cp_sweeps_merge": (itertools.product(ROWS, BATCH, BOXES), lambda N, B, S: 4 * (N // 256 + B * S + 3), False),
    "md_cp_assign_targets": (itertools.product(BATCH, (1, 6), BOXES), lambda B, T_, G: B * T_ * (G + 1) * 16, True),
    "md_cp_loss": (itertools.product(BATCH, (1, 6), (1, 8, 300), (1, 12)), lambda B, T_, H, W: 8 * B * T_ * (12 + cdiv(H * W, STRIP_CP)), True),
    "md_pp_loss": (itertools.product(BATCH, (1, 8, 300), (1, 12), (1, 2)),
                   lambda B, H, W, A: 40 * B * cdiv(H * W, STRIP_PP) + 4 * B * cdiv(H * W * A, CHUNK_PP), True),
    "md_cn_assign_targets": (itertools.product(BATCH, (0, 4, 128)), lambda B, M: 16 * B * M, True),
    "md_cn_loss": (itertools.product(BATCH, (1, 80), (1, 8, 300), (1, 12)),
                   lambda B, Cn, H, W: 8 * B * (4 + 2 * cdiv(H * W, STRIP_CN)) + 4 * cdiv(B * Cn * H * W, CHUNK_CN), True),
    "md_cn_aug_image": (itertools.product(BATCH, (1, 6, 300), (1, 10, 257)),
                        lambda B, h, w: 8 * B * ((h * w + CHUNK_GREY - 1) // CHUNK_GREY + 1), False),
    "md_pc_crop_hulls": (itertools.product(ROWS, BATCH, BOXES), lambda N, B, K: 192 * B * K + 4 * (N // 256 + 3), False),
}


def test_the_answer_never_exceeds_the_bound_the_header_documents():
    assert set(BOUNDS) | {"md_topk_segmented"} == set(DECLARED)
    for op, (sweep, bound, exact) in BOUNDS.items():
        n = 0
        for dims in sweep:
            got, cap = ask(op, *dims), bound(*dims)
            assert (got == cap) if exact else (0 <= got <= cap), (op, dims, got, cap)
            n += 1
        assert n >= 4, op
    # the formulas the test evaluates are the headers' own text
    for hdr, text in (("minddet_hip_pcaug.h", "128 B (G + R) + 64 B + 4 (N / 256 + 3)"), ("minddet_hip_cpaug.h", "96 B G"),
                      ("minddet_hip_cpaug.h", "8 B S ((G + S + 63) / 64)"), ("minddet_hip_cpaug.h", "64 B + (N + Ns) + 4 ((N + Ns) / 256 + 3)"),
                      ("minddet_hip_cpsweeps.h", "4 (N / 256 + B S + 3)"), ("minddet_hip_kitti.h", "192 B K + 4 (N / 256 + 3)"),
                      ("minddet_hip_cnaug.h", "8 B ((out_h out_w + 2047) / 2048 + 1)"), ("minddet_hip_cptargets.h", "B T (G + 1) x 16"),
                      ("minddet_hip_cn.h", "16 B M"), ("minddet_hip_cp.h", "L N (20 x 4 + ceil(N / 64) x 8)"),
                      ("minddet_hip_cn.h", "8 B (4 + 2 ceil(H W / MD_CN_LOSS_STRIP)) + 4 ceil(B C H W / MD_CN_LOSS_COUNT_CHUNK)"),
                      ("minddet_hip_cploss.h", "8 B T (12 + ceil(H W / MD_CP_LOSS_STRIP))"),
                      ("minddet_hip_pploss.h", "40 B ceil(H W / MD_PP_LOSS_STRIP) + 4 B ceil(N / MD_PP_LOSS_COUNT_CHUNK)"),
                      ("minddet_hip_points.h", "4 * (2 B gx gy gz + 3 N + 2 B max_voxels + (N + B max_voxels) / 1024) + 4096"),
                      ("minddet_hip_ppreader.h", "B * grid_y * grid_x * 4"), ("minddet_hip.h", "8 B N ceil(N / 64) + 4 B + 252")):
        assert text in " ".join(HEADERS[hdr].replace("*      ", "").replace(" * ", " ").split()) or text in HEADERS[hdr], (hdr, text)


def test_the_exact_values_follow_from_the_layouts():
    """by hand from the layout comments over each function in csrc/*.hip"""
    assert ask("md_pc_augment_points", 300, 2, 3, 2) == 2 * 5 * 16 * 8 + 2 * 8 * 8 + (2 + 1) * 4 == 1420
    assert ask("md_cp_aug_points", 300, 40, 2) == 2 * 8 * 8 + (2 + 1) * 4 + 340 == 480
    assert ask("md_cp_sweeps_merge", 300, 2, 3) == (2 + 6 + 1) * 4 == 36
    assert ask("md_cp_sweeps_merge", 1040000, 4, 10) == (4063 + 40 + 1) * 4 == 16416
    assert ask("md_cp_sweeps_merge", 0, 0, 0) == 8                                   # one workgroup at the least
    assert ask("md_pc_crop_hulls", 300, 2, 3) == 6 * 24 * 8 + (2 + 1) * 4 == 1164
    assert ask("md_pc_crop_hulls", 480000, 4, 1) == 4 * 24 * 8 + (1875 + 1) * 4 == 8272
    assert ask("md_cn_aug_image", 2, 6, 10) == 2 * (1 + 1) * 8 == 32
    assert ask("md_cp_aug_count_points", 2, 3) == 6 * 12 * 8 == 576
    assert ask("md_cp_aug_select", 2, 3, 4) == 2 * 4 * 1 * 8 == 64
    assert ask("md_cp_loss", 4, 6, 128, 128) == 8 * 4 * 6 * (12 + 256)
    assert ask("md_voxelize", 300, 2, 100, 10) == 4 * (2 * 256 + 2 * 320 + 320 + 64 + 64 + 64) == 6656


def _constant(name):
    txt = open(os.path.join(ROOT, "minddet_amd", "csrc", "detops.hip")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", txt).group(1))


def test_topk_takes_scratch_on_the_multi_workgroup_path_alone():
    chunk, cap, bins = _constant("TK_CHUNK"), _constant("TK_CAP"), _constant("TK_BINS")
    src = open(os.path.join(ROOT, "minddet_amd", "csrc", "detops.hip")).read()
    assert "if (max_segment > 4 * TK_CHUNK && k <= TK_CAP / 2 && L <= 65535) {" in src
    seg, kmax, lmax = 4 * chunk, cap // 2, 65535
    assert (seg, kmax) == (32768, 4096)                                              # the figures of include/minddet_hip.h
    for L, k in itertools.product((1, 2, lmax), (1, 2, kmax)):
        want = (L * (bins * 4 + 4) + 255) // 256 * 256 + L * cap * 8                 # the header's formula
        assert ask("md_topk_segmented", L, k, seg + 1) == ask("md_topk_segmented", L, k, 1 << 30) == want > 0
        for m in (0, 1, 30000, seg):
            assert ask("md_topk_segmented", L, k, m) == 0
    for m in (seg + 1, 1 << 30):
        assert ask("md_topk_segmented", 2, kmax + 1, m) == 0 and ask("md_topk_segmented", lmax + 1, 2, m) == 0


def test_nms_aligned_adds_the_flag_block_from_two_prefixes_on():
    mask = lambda B, n: 8 * B * n * cdiv(n, 64)
    for B in BATCH:
        for n in ROWS + (1023, 1024, 2048, 65536):
            assert ask("md_nms_aligned", B, n, 0) == mask(B, n)
        # quota 100: the prefix is P = max(4 x 100, 512) rounded up to the tile = 512 boxes (csrc/nms.hip)
        assert ask("md_nms_aligned", B, 1023, 100) == mask(B, 1023)
        assert ask("md_nms_aligned", B, 1024, 100) == mask(B, 1024) + 256
        # quota 300: P = 1216 (YOLO's 4 096 candidates run the two-level form)
        assert ask("md_nms_aligned", B, 2431, 300) == mask(B, 2431) and ask("md_nms_aligned", B, 2432, 300) == mask(B, 2432) + 256
    assert ask("md_nms_aligned", 65, 4096, 300) == mask(65, 4096) + 512


def test_the_python_functions_are_the_librarys_answers():
    for name, op, dims in (("voxelize", "md_voxelize", (300, 2, 100, 10)), ("pc_augment_points", "md_pc_augment_points", (300, 2, 3, 2)),
                           ("cp_aug_count_points", "md_cp_aug_count_points", (2, 3)), ("cp_aug_select", "md_cp_aug_select", (2, 3, 4)),
                           ("cp_aug_points", "md_cp_aug_points", (300, 40, 2)), ("cp_sweeps_merge", "md_cp_sweeps_merge", (300, 2, 3)),
                           ("cp_loss", "md_cp_loss", (4, 6, 128, 128)), ("pp_loss", "md_pp_loss", (2, 8, 12, 2)),
                           ("cn_loss", "md_cn_loss", (2, 3, 8, 12)), ("cn_aug_image", "md_cn_aug_image", (2, 6, 10)),
                           ("crop_hulls", "md_pc_crop_hulls", (300, 2, 3))):
        assert getattr(det_ops, name + "_workspace_bytes")(*dims) == ask(op, *dims) > 0, name
    src = open(os.path.join(ROOT, "minddet_amd", "det_ops.py")).read()
    for body in re.findall(r"^def \w+_workspace_bytes\(.*?\):\n((?:    .*\n)+)", src, flags=re.M):
        code = [ln for ln in body.splitlines() if not ln.strip().startswith('"""')]
        assert len(code) == 1 and code[0].startswith("    return _lib.workspace_bytes("), body
    assert "dtype=torch.uint8" not in "".join(ln for ln in src.splitlines(True) if "// 256" in ln or "// 64" in ln or "8192" in ln or "* 16,)" in ln)


# ----- a workspace one byte short is refused with MD_ERR_SIZE, before anything touches the device
def _grid_cells(at):
    return int(__import__("numpy").prod(det_ops.voxel_grid(list(at.voxel_size), list(at.range))))


def _lead(ops):
    return 1 if len(ops[0].shape) == 2 else ops[0].shape[0]


DIMS = {
    "md_nms_aligned": lambda o, at: (_lead(o), o[0].shape[-2], at.max_output),
    "md_nms_rotated": lambda o, at: (_lead(o), o[0].shape[-2]),
    "md_topk_segmented": lambda o, at: (o[1].shape[0] - 1, at.k, at.max_segment),
    "md_voxelize": lambda o, at: (o[0].shape[0], o[1].shape[0] - 1, _grid_cells(at), o[2].shape[1]),
    "md_pp_anchor_mask": lambda o, at: (o[0].shape[0], at.grid_x, at.grid_y),
    "md_pc_augment_points": lambda o, at: (o[0].shape[0], o[1].shape[0] - 1, o[2].shape[1], 0 if o[6].null else o[6].shape[1]),
    "md_cp_aug_count_points": lambda o, at: o[2].shape[:2],
    "md_cp_aug_select": lambda o, at: (*o[0].shape[:2], o[3].shape[1]),
    "md_cp_aug_points": lambda o, at: (o[0].shape[0], 0 if o[2].null else o[2].shape[0], o[1].shape[0] - 1),
    "md_cp_sweeps_merge": lambda o, at: (o[0].shape[0], *o[1].shape[:2]),
    "md_cp_assign_targets": lambda o, at: (o[0].shape[0], o[2].shape[1], o[0].shape[1]),
    "md_cp_loss": lambda o, at: (o[0].shape[0], o[1].shape[1], *o[0].shape[1:3]),
    "md_pp_loss": lambda o, at: (*o[0].shape[:3], at.head.num_anchors),
    "md_cn_assign_targets": lambda o, at: (o[0].shape[0], o[3].shape[1]),
    "md_cn_loss": lambda o, at: (o[0].shape[0], o[1].shape[1], *o[0].shape[1:3]),
    "md_cn_aug_image": lambda o, at: (o[0].shape[0], at.out_h, at.out_w),
    "md_pc_crop_hulls": lambda o, at: (o[0].shape[0], o[1].shape[0] - 1, o[2].shape[1]),
}
TABLES = (abi_cases, abi_cases_cn, abi_cases_cnaug, abi_cases_cp, abi_cases_cpaug, abi_cases_cploss, abi_cases_cpsweeps, abi_cases_cptargets,
          abi_cases_kitti, abi_cases_pcaug, abi_cases_points, abi_cases_pploss, abi_cases_ppreader)
COVERED_ROWS = [c for t in TABLES for c in t.CASES if c.sym in COVERED]


def test_every_covered_entry_point_has_a_row():
    assert {c.sym for c in COVERED_ROWS} == set(COVERED) and set(DIMS) == set(COVERED.values())


def _with_workspace(case, nbytes):
    """the row with its workspace operand described as nbytes (absent optional operands in front of it stay NULL)"""
    c = copy.copy(case)
    at = max(case.nparam) - 1
    ops = list(case.operands[:at])
    ops += [T((1,), F, "opt", null=True) for _ in range(at - len(ops))]
    c.operands, c.nparam = ops + [T((nbytes,), U8, "opt", "free")], case.nparam
    return Call(c)


def _need(case):
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ask(COVERED[case.sym], *DIMS[COVERED[case.sym]](case.operands, case.extra))


def test_the_tables_own_workspaces_hold_the_answers():
    for case in COVERED_ROWS:
        given = case.operands[max(case.nparam) - 1:]
        assert not given or given[0].shape[0] >= _need(case), case.id


# (rows whose answer is 16 bytes or less are left out: Scratch::acquire holds an answer of 0 to 16 bytes, so "one byte short" of a tiny
# answer is not one rule)
SHORT_ROWS = [c for c in COVERED_ROWS if _need(c) > 16]


@pytest.mark.parametrize("case", SHORT_ROWS, ids=[c.id for c in SHORT_ROWS])
def test_a_workspace_one_byte_short_is_refused_with_size(case):
    assert _with_workspace(case, _need(case) - 1).run(C.CDLL(_lib.LIB_PATH)) == 4


def test_the_short_rows_reach_every_covered_op_but_the_scratch_free_topk_row():
    assert {c.sym for c in SHORT_ROWS} == set(COVERED) - {"md_topk_segmented"}
