"""-m gpu: the CenterPoint post-processing chain (include/minddet_hip_cp.h, det_ops.CenterHeadPostBatched) against what it replaces.
(1) md_nms_rotated on six clustered lists of different counts == the single-list operators on each list's valid rows, bit for bit;
(2) md_nms_rotated on three permutations of the SURVEY 8(d) rotated boxes == oracle.nms_rot_aot / oracle.nms_rot_mask;
(3) md_cp_scores / md_cp_decode_selected == md_centerpoint_decode per task (bit for bit) and np_ops.centerpoint_decode (tolerances of
    tests/test_centerpoint_gpu.py::test_detector_end_to_end);
(4) md_cp_pack == graphs.merge_center_tasks on crafted counts;
(5) the detector: forward(x) through the chain (cp_post=True) == forward(x, return_aux=True) (the per-task path), one and two streams,
    and with MD_CP_POST=1 / MD_CP_POST=0 in a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import np_ops
from tests import nms_contract as nc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {n: os.path.join(ROOT, "configs", "centerpoint", f"centerpoint_pp_{n}.py") for n in ("nusc", "tiny")}
_cache = {}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------- (1) batched NMS
COUNTS = (0, 1, 64, 65, 130, 200)
N1 = 200
FILL = np.array([0.0, 0.0, 0.0, 500.0, 500.0, 1.0, 0.0], np.float32)     # overlaps every box of every list: must never be read
DEAD_ROWS = (3, 40, 66, 129)                                             # zero-area boxes (mode 1), inside the counts that reach them


def nms_lists(mode):
    key = ("lists", mode)
    if key not in _cache:
        b = np.stack([nc.rot_clustered(N1, 9, 40 + l, span=12.0) for l in range(len(COUNTS))])
        if mode == 1:
            b[:, DEAD_ROWS, 3] = 0.0
        valid = b.copy()
        for l, c in enumerate(COUNTS):
            b[l, c:] = FILL
        _cache[key] = (b, valid)
    return _cache[key]


def single_list(boxes, thr, mode):
    """the existing operator of the mode on one list -> (keep, num)"""
    from minddet_amd import det_ops

    if boxes.shape[0] == 0:
        return np.zeros((0,), np.int64), 0
    if mode == 1:
        keep, num = det_ops.NMS()(T(boxes), thr)
        return keep.cpu().numpy().astype(np.int64), int(num)
    keep, num = det_ops.NumGpu()(T(boxes), thr)
    return keep.cpu().numpy(), int(num[0])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("max_output", [0, 7])
def test_batched_rotated_nms_equals_the_single_list_operators(mode, max_output):
    from minddet_amd import det_ops

    thr = 0.2
    boxes, _ = nms_lists(mode)
    count = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    keep, num = det_ops.nms_rotated(T(boxes), thr, mode, count=count, max_output=max_output)
    torch.cuda.synchronize()
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    assert keep.shape == (len(COUNTS), N1) and keep.dtype == np.int32 and num.shape == (len(COUNTS),)
    suppressed = 0
    for l, c in enumerate(COUNTS):
        k_s, n_s = single_list(boxes[l, :c], thr, mode)
        suppressed += int(n_s < c)
        want = min(n_s, max_output) if max_output else n_s
        assert int(num[l]) == want, (l, int(num[l]), want)
        np.testing.assert_array_equal(keep[l, :want], k_s[:want])
        assert (keep[l, want:] == 0).all()
    assert suppressed >= 1                       # a chain that never suppresses cannot pass
    if mode == 1:                                # the zero-area rows are dropped, and a list whose only row is alive keeps it
        assert not np.isin(keep[5, :num[5]], DEAD_ROWS).any() and int(num[1]) == 1


@pytest.mark.parametrize("mode", [0, 1])
def test_batched_rotated_nms_null_count_and_one_list_forms(mode):
    from minddet_amd import det_ops

    thr = 0.2
    _, valid = nms_lists(mode)
    keep, num = det_ops.nms_rotated(T(valid), thr, mode)                   # count NULL: all N rows of every list
    k1, n1 = det_ops.nms_rotated(T(valid[2]), thr, mode, max_output=5)     # [N,7]
    torch.cuda.synchronize()
    for l in range(valid.shape[0]):
        k_s, n_s = single_list(valid[l], thr, mode)
        assert int(num[l]) == n_s and n_s < N1
        np.testing.assert_array_equal(keep[l].cpu().numpy(), k_s)
    k_s, n_s = single_list(valid[2], thr, mode)
    assert tuple(k1.shape) == (N1,) and tuple(n1.shape) == (1,) and int(n1[0]) == 5 and n_s > 5
    np.testing.assert_array_equal(k1.cpu().numpy()[:5], k_s[:5])
    assert (k1.cpu().numpy()[5:] == 0).all()
    # no workspace operand: the library's own scratch pool serves
    from minddet_amd import _lib
    k2 = torch.empty((valid.shape[0], N1), dtype=torch.int32, device=DEV)
    n2 = torch.empty((valid.shape[0],), dtype=torch.int32, device=DEV)
    _lib.call("md_nms_rotated", [T(valid), None, k2, n2], extra=det_ops._NmsRotatedAttrs(thr, mode, 0))
    torch.cuda.synchronize()
    assert torch.equal(k2, keep) and torch.equal(n2, num)


# ------------------------------------------------------------------------------------------------------------------- (2) the oracle
def survey_boxes(n=1000, seed=0, span=50.0):
    """centres U(-span, span)^2, dims U(1, 5), heading U(-pi, pi)"""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-span, span, (n, 2))
    b[:, 2] = rng.uniform(-2, 2, n)
    b[:, 3:6] = rng.uniform(1, 5, (n, 3))
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def test_batched_rotated_nms_against_the_oracle():
    from minddet_amd import det_ops

    thr = 0.2
    base = survey_boxes()
    rng = np.random.default_rng(1)
    lists = np.stack([base, base[rng.permutation(len(base))], base[rng.permutation(len(base))]])
    for mode, ref in ((1, oracle.nms_rot_aot), (0, oracle.nms_rot_mask)):
        keep, num = det_ops.nms_rotated(T(lists), thr, mode)
        torch.cuda.synchronize()
        for l in range(3):
            k_o, n_o = ref(lists[l], thr)
            assert int(num[l]) == n_o and 0 < n_o < len(base)
            np.testing.assert_array_equal(keep[l].cpu().numpy(), k_o)


# ------------------------------------------------------------------------------------------------------------- (3) scores and decode
NUSC_NC = (1, 2, 2, 1, 2, 2)
K3 = 100


def nusc_offsets():
    out, base = [], 0
    for ncls in NUSC_NC:
        out.append(dict(reg=base, height=base + 2, dim=base + 3, rot=base + 6, vel=base + 8, hm=base + 10))
        base += 10 + ncls
    assert base == 70
    return out


def cp_layout(name):
    """-> (head [2,16,24,C] bf16 on the device, per task offsets, per task num_class, test config, planted cells)"""
    if name in _cache:
        return _cache[name]
    from minddet_amd import det_ops

    g = torch.Generator().manual_seed(5 if name == "nusc" else 6)
    B, H, W = 2, 16, 24
    if name == "nusc":
        offs, ncs, C = nusc_offsets(), list(NUSC_NC), 72
    else:       # two tasks without a vel head in 16 channels (the second task's heads share channels with the first's: any layout is legal)
        offs, ncs, C = [dict(reg=0, height=2, dim=3, rot=6, hm=8), dict(reg=10, height=12, dim=13, rot=4, hm=6)], [2, 2], 16
    head = torch.randn((B, H, W, C), generator=g)
    for off in offs:
        head[..., off["reg"]:off["reg"] + 2] = torch.rand((B, H, W, 2), generator=g)
        head[..., off["dim"]:off["dim"] + 3] *= 0.3
    plants = {}
    if name == "nusc":
        # exact class ties in task 1 (cells 5 .. 24 of sample 0): the first class wins
        o = offs[1]["hm"]
        head[0, 0, 5:24, o + 1] = head[0, 0, 5:24, o]
        plants["ties"] = (0, 1, list(range(5, 24)))
        # task 3 of sample 1: nearly every cell below the score threshold -> cnt < k
        o = offs[3]["hm"]
        head[1, :, :, o] = -6.0
        head[1, 2, 1:9, o] = torch.linspace(0.5, 2.0, 8)
        # the score threshold is the score of cell (0, 3, 2) of task 0: `best > thr` fails there by equality
        head[0, 3, 2, offs[0]["hm"]] = -1.5
        head[0, 3, 3, offs[0]["hm"]] = -1.4921875          # the next bf16 above: passes
        head[0, 3, 2:4, offs[0]["reg"]:offs[0]["reg"] + 2] = 0.5
        head[0, 3, 2:4, offs[0]["height"]] = 0.0
        plants["at_thr"] = (0, 0, 3 * W + 2)
    head = head.to(torch.bfloat16)
    # 0.8 m cells from (-9.6, -6.4): the x range ends in the middle of the map -> about half of the cells are outside
    cfg = dict(post_center_limit_range=[-20.0, -20.0, -2.5, 0.0, 20.0, 2.5], score_threshold=0.1, pc_range=[-9.6, -6.4], out_size_factor=4,
               voxel_size=[0.2, 0.2], nms=dict(nms_pre_max_size=K3, nms_post_max_size=10, nms_iou_threshold=0.2))
    if name == "nusc":
        # the threshold = the fp32 sigmoid of the planted logit as the device computes it (read from the existing kernel with threshold 0)
        probe = det_ops.CenterHeadPost(offs[0], 1, dict(cfg, score_threshold=0.0))(head.to(DEV), return_aux=True)[1]["scores"]
        cfg["score_threshold"] = float(probe[0, 3 * W + 2])
        assert 0.18 < cfg["score_threshold"] < 0.19
    _cache[name] = (head.to(DEV), offs, ncs, cfg, plants)
    return _cache[name]


def per_task_reference(name):
    """md_centerpoint_decode per task: the kernel the per-task path runs"""
    key = ("ref", name)
    if key not in _cache:
        from minddet_amd import det_ops

        head, offs, ncs, cfg, _ = cp_layout(name)
        refs = []
        for off, ncls in zip(offs, ncs):
            aux = det_ops.CenterHeadPost(off, ncls, cfg)(head, return_aux=True)[1]
            refs.append({k: aux[k] for k in ("scores", "labels", "boxes", "nms_boxes")})
        torch.cuda.synchronize()
        _cache[key] = refs
    return _cache[key]


def chain_tensors(name):
    key = ("chain", name)
    if key not in _cache:
        from minddet_amd import det_ops

        head, offs, ncs, cfg, _ = cp_layout(name)
        post = det_ops.CenterHeadPostBatched(offs, ncs, cfg)
        out, aux = post(head, return_aux=True)
        torch.cuda.synchronize()
        _cache[key] = (post, out, aux)
    return _cache[key]


@pytest.mark.parametrize("name", ["nusc", "two"])
def test_scores_and_selected_decode_equal_the_per_task_kernel(name):
    head, offs, ncs, cfg, plants = cp_layout(name)
    refs = per_task_reference(name)
    _, _, aux = chain_tensors(name)
    B, n, Tn = head.shape[0], head.shape[1] * head.shape[2], len(offs)
    assert tuple(aux["scores"].shape) == (B, Tn, n) and tuple(aux["boxes"].shape) == (B, Tn, K3, 9)
    short = full = 0
    for t in range(Tn):
        r = refs[t]
        assert torch.equal(aux["scores"][:, t], r["scores"]), t
        frac = float((r["scores"] > -1).float().mean())
        if not (name == "nusc" and t == 3):
            assert 0.2 < frac < 0.6, (t, frac)                  # the range cut takes about half of the cells, the threshold some more
        for b in range(B):
            c = int(aux["topk_cnt"][b, t])
            assert c == min(int((r["scores"][b] > -1).sum()), K3)
            short += int(c < K3)
            full += int(c == K3)
            idx = aux["topk_idx"][b, t, :c].long()
            assert bool((r["scores"][b][idx] > -1).all())
            assert torch.equal(aux["boxes"][b, t, :c], r["boxes"][b][idx])
            assert torch.equal(aux["nms_boxes"][b, t, :c], r["nms_boxes"][b][idx])
            assert torch.equal(aux["labels"][b, t, :c], r["labels"][b][idx])
            assert not bool(aux["boxes"][b, t, c:].any()) and not bool(aux["nms_boxes"][b, t, c:].any()) and not bool(aux["labels"][b, t, c:].any())
    assert full >= 1
    if name == "nusc":
        assert short >= 1                        # a chain that never pads cannot pass
        b, t, cells = plants["ties"]
        passed = [c for c in cells if float(refs[t]["scores"][b, c]) > -1]
        assert len(passed) >= 3 and all(int(refs[t]["labels"][b, c]) == 0 for c in passed)
        sel = aux["topk_idx"][b, t, :int(aux["topk_cnt"][b, t])].cpu().tolist()
        tied = [j for j, c in enumerate(sel) if c in cells]
        assert tied and all(int(aux["labels"][b, t, j]) == 0 for j in tied)
        b, t, cell = plants["at_thr"]
        assert float(aux["scores"][b, t, cell]) == -1.0 and float(aux["scores"][b, t, cell + 1]) > cfg["score_threshold"]


def test_chain_tensors_against_the_numpy_decode():
    head, offs, ncs, cfg, _ = cp_layout("nusc")
    _, _, aux = chain_tensors("nusc")
    hf = head.float().cpu().numpy()
    checked = same = 0
    for t, (off, ncls) in enumerate(zip(offs, ncs)):
        s_o, l_o, b_o, nb_o, mask_o = np_ops.centerpoint_decode(hf, off, ncls, cfg)
        s_d = aux["scores"][:, t].cpu().numpy()
        near = np.abs(np.where(mask_o, s_o, 1.0) - cfg["score_threshold"]) < 1e-5
        assert ((s_d > -1) == mask_o)[~near].all()
        both = (s_d > -1) & mask_o
        np.testing.assert_allclose(s_d[both], s_o[both], rtol=2e-6, atol=1e-7)
        for b in range(hf.shape[0]):
            c = int(aux["topk_cnt"][b, t])
            idx = aux["topk_idx"][b, t, :c].cpu().numpy()
            ok = both[b][idx]
            np.testing.assert_allclose(aux["boxes"][b, t, :c].cpu().numpy()[ok], b_o[b][idx][ok], rtol=3e-6, atol=2e-5)
            np.testing.assert_allclose(aux["nms_boxes"][b, t, :c].cpu().numpy()[ok], nb_o[b][idx][ok], rtol=3e-6, atol=2e-5)
            same += int((aux["labels"][b, t, :c].cpu().numpy()[ok] == l_o[b][idx][ok]).sum())
            checked += int(ok.sum())
    assert checked > 500 and same / checked > 0.9999


def test_chain_on_the_planted_heads_equals_the_per_task_path():
    from minddet_amd import det_ops, graphs

    for name in ("nusc", "two"):
        head, offs, ncs, cfg, _ = cp_layout(name)
        _, (dets, count), aux = chain_tensors(name)
        outs = [det_ops.CenterHeadPost(off, ncls, cfg)(head) for off, ncls in zip(offs, ncs)]
        want, want_count = graphs.merge_center_tasks(outs, ncs, cfg["nms"]["nms_post_max_size"])
        assert torch.equal(dets, want) and torch.equal(count, want_count) and int(count.sum()) > 0
        assert bool((aux["num"] < aux["topk_cnt"]).any())       # the NMS suppressed something


# --------------------------------------------------------------------------------------------------------------------------- (4) pack
def test_pack_equals_merge_center_tasks():
    from minddet_amd import det_ops, graphs

    B, Tn, k, m = 3, 3, 12, 4
    g = torch.Generator().manual_seed(8)
    boxes = torch.randn((B, Tn, k, 9), generator=g)
    labels = torch.randint(0, 2, (B, Tn, k), generator=g, dtype=torch.int32)
    scores = torch.sort(torch.rand((B, Tn, k), generator=g) * 0.8 + 0.1, dim=2, descending=True)[0]
    keep = torch.zeros((B, Tn, k), dtype=torch.int32)
    #            sample 0: cnt = 0 | num > m | num < cnt          sample 1: a zero score inside the count | .. | ..      sample 2: all full
    num = torch.tensor([[0, 7, 2], [3, 4, 1], [4, 6, 5]], dtype=torch.int32)
    cnt = torch.tensor([[0, 9, 12], [5, 12, 3], [12, 12, 12]], dtype=torch.int32)
    for b in range(B):
        for t in range(Tn):
            nk = int(num[b, t])
            keep[b, t, :nk] = torch.sort(torch.randperm(max(int(cnt[b, t]), 1), generator=g)[:nk])[0].to(torch.int32)
    scores[1, 0, int(keep[1, 0, 1])] = 0.0           # kept row 1 of (1, 0) has score exactly 0: size = 2 of 3, the FIRST two rows go out
    scores[1, 1, int(keep[1, 1, 3])] = -0.0
    ncs = [1, 2, 2]
    at = det_ops.cp_head_attrs([dict(reg=0, height=2, dim=3, rot=6, hm=8)] * Tn, ncs,
                               dict(score_threshold=0.1, out_size_factor=4, voxel_size=[0.2, 0.2], pc_range=[0, 0],
                                    post_center_limit_range=[0] * 6, nms=dict(nms_post_max_size=m)))
    dv = [x.to(DEV) for x in (boxes, scores, labels, keep, num, cnt)]
    dets, count = det_ops.cp_pack(*dv, at)
    outs = []
    for t in range(Tn):
        bx, sc, lb, kp = dv[0][:, t], dv[1][:, t], dv[2][:, t], dv[3][:, t]
        c = torch.minimum(torch.minimum(dv[4][:, t], dv[5][:, t]), torch.full_like(dv[4][:, t], m))
        outs.append([det_ops.gather_rows(bx.contiguous(), kp.contiguous()), torch.gather(sc, 1, kp.long()), torch.gather(lb, 1, kp.long()), c])
    want, want_count = graphs.merge_center_tasks(outs, ncs, m)
    torch.cuda.synchronize()
    assert tuple(dets.shape) == (B, Tn * m, 11) and torch.equal(count, want_count) and torch.equal(dets, want)
    assert count.cpu().tolist() == [4 + 2, 2 + 3 + 1, 12]
    assert not bool(dets[0, 6:].any()) and float(dets[2, -1, 10]) in (3.0, 4.0)


# ------------------------------------------------------------------------------------------------------------------- (5) the detector
def _detector(name, seed, cp_post=True, **test_over):
    from minddet.models import Config, build_detector

    cfg = Config.fromfile(CFG[name])
    return build_detector(dict(cfg.model, seed=seed, cp_post=cp_post), cfg.train_cfg, dict(cfg.test_cfg, **test_over)).to(DEV), cfg


def _library_calls(fn):
    """the entry points fn() calls, in order"""
    from minddet_amd import _lib

    names, real = [], _lib.call

    def spy(name, tensors, extra=None, stream=None):
        names.append(name)
        return real(name, tensors, extra=extra, stream=stream)

    _lib.call = spy
    try:
        out = fn()
    finally:
        _lib.call = real
    return out, names


CHAIN_CALLS = ["md_cp_scores", "md_topk_segmented", "md_cp_decode_selected", "md_nms_rotated", "md_cp_pack"]


def _pseudo_image(B, hw, frac, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn((B, hw, hw, 64), generator=g))
    mask = torch.rand((B, hw, hw, 1), generator=g) < frac
    return (x * mask).to(torch.bfloat16)


@pytest.mark.parametrize("name,B,hw", [("tiny", 3, 128), ("nusc", 2, 512)])
def test_detector_chain_equals_the_per_task_path(name, B, hw):
    m, cfg = _detector(name, 9)
    assert m.cp_post is True
    x = _pseudo_image(B, hw, 0.1, 11).to(DEV)
    (want, want_count), aux = m.forward(x, return_aux=True)
    (dets, count), names = _library_calls(lambda: m.forward(x))
    torch.cuda.synchronize()
    assert names[-5:] == CHAIN_CALLS and "md_centerpoint_decode" not in names        # five calls, seven launches, for all tasks and samples
    mt = 6 * cfg.test_cfg["nms"]["nms_post_max_size"]
    assert tuple(dets.shape) == (B, mt, 11) and "tasks" in aux
    assert torch.equal(dets, want) and torch.equal(count, want_count) and int(count.sum()) > 0
    # two streams: the parts of the batch through the chain on their own streams
    m2, _ = _detector(name, 9, streams=2)
    assert m2.streams == 2
    xb = x if B % 2 == 0 else torch.cat([x, x[:1]])
    d2, c2 = m2.forward_split(xb)
    torch.cuda.synchronize()
    assert torch.equal(d2[:B], want) and torch.equal(c2[:B], want_count)
    # the constructor argument selects the per-task path in-process
    m3, _ = _detector(name, 9, cp_post=False)
    (d3, c3), names = _library_calls(lambda: m3.forward(x))
    assert torch.equal(d3, want) and torch.equal(c3, want_count) and names.count("md_centerpoint_decode") == 6 and "md_cp_scores" not in names


CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from minddet.models import Config, build_detector
from minddet_amd import _lib, graphs
assert graphs.CP_POST is {on}
cfg = Config.fromfile({cfg!r})
m = build_detector(dict(cfg.model, seed=9), cfg.train_cfg, cfg.test_cfg).to("cuda:0")
assert m.cp_post is {on}
x = torch.load({inp!r}).to("cuda:0")
names, real = [], _lib.call
def spy(name, tensors, extra=None, stream=None):
    names.append(name)
    return real(name, tensors, extra=extra, stream=stream)
_lib.call = spy
dets, count = m.forward(x)
torch.cuda.synchronize()
assert ("md_cp_scores" in names) is {on} and ("md_centerpoint_decode" in names) is not {on}
torch.save((dets.cpu(), count.cpu()), {out!r})
"""


@pytest.mark.parametrize("value", ["1", "0"])
def test_env_switch_selects_the_path_in_a_fresh_process(tmp_path, value):
    m, _ = _detector("tiny", 9)
    x = _pseudo_image(3, 128, 0.1, 11)
    dets, count = m.forward(x.to(DEV))
    torch.cuda.synchronize()
    inp, out = str(tmp_path / "x.pt"), str(tmp_path / "out.pt")
    torch.save(x, inp)
    env = dict(os.environ, MD_CP_POST=value)
    subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, cfg=CFG["tiny"], inp=inp, out=out, on=value == "1")], check=True, env=env,
                   timeout=300)
    d0, c0 = torch.load(out)
    assert torch.equal(d0, dets.cpu()) and torch.equal(c0, count.cpu()) and int(c0.sum()) > 0
