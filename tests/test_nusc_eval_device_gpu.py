"""-m gpu: the nuScenes detection evaluation on the device (include/minddet_hip_nusceval.h) judged by the host evaluator it replaces
(minddet_amd/nusc_eval.py: dets_to_nusc, NuscDetectionEval.evaluate, summarize) -- never by itself.  Every comparison is exact
(np.array_equal on the values, the float tables on their bits) except dt_quat and dt_yaw, which go through the device's sin, cos and
atan2 and are held to the interval of tests/nusc_eval_contract.py (each within 4 ulp of the float64 value, propagated through the two
Hamilton products and the matrix entries; measured on the MI355X: worst 0.081 of the bound for dt_quat, 0.097 for dt_yaw).  The set is
tests/nusc_eval_contract.py's: 12 samples x 10 classes, 500 rows per sample."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import nusc_eval_contract as nc
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs MI355X")]

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.linspace(0, 1, 101)
EXACT = ("dtm", "err", "cell_ngt", "tp_scan", "m_conf", "m_cum", "precision", "confidence", "tp_err", "n_gt", "n_match")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _host():
    """the host evaluator on the test set's records, evaluated once and left unchanged"""
    from minddet_amd import nusc_eval as ne
    s = nc.test_set()
    return ne.NuscDetectionEval(s["gt_records"], s["dt_records"], s["ego"], nc.CLASSES).evaluate()


def _device_rows(batches=((0, 5), (7, 5), (5, 2))):
    """pack_nusc of the ground truth on the device and md_nusc_rows on the test set's (dets, count), B = 5 with first_sample 0 and 7"""
    from minddet_amd import nusc_eval as ne
    s = nc.test_set()
    p = ne.pack_nusc(s["gt_records"], s["ego"], nc.CLASSES, device=DEV)
    td, tc, tp = torch.from_numpy(s["dets"]).to(DEV), torch.from_numpy(s["count"]).to(DEV), torch.from_numpy(s["poses"]).to(DEV)
    for first, B in batches:
        p.add_dets(td[first:first + B], tc[first:first + B], tp[first:first + B], first)
    return p


@functools.lru_cache(maxsize=None)
def _rows():
    p = _device_rows()
    return p, p.numpy()


def _tables(p):
    """md_nusc_eval_match and md_nusc_eval_accumulate on a pack -> the dict of NuscDetectionEval.tables"""
    from minddet_amd import nusc_eval as ne
    ev = ne.NuscDetectionEval.from_packed(p).evaluate(backend="device")
    assert set(ev.tables) == {"precision", "confidence", "tp_err", "n_gt", "n_match"}      # what is read back; the rest stays on the device
    return {n: t.cpu().numpy() for n, t in ev.device_tables.items()}


def test_rows_equal_the_host_and_quat_and_yaw_lie_in_the_interval():
    from minddet_amd import nusc_eval as ne
    ev, s = _host(), nc.test_set()
    z, (p, got) = ev.z, _rows()
    M, Kc = nc.MAX_DET, nc.KC
    assert _same(got["dt_cnt"], z["dt_cnt"]) and got["dt_cnt"].max() == 300 and len(got["dt_cat"]) == nc.I * M
    mv, st = ne.attr_tables(nc.CLASSES)
    rng_ = [ne.DETECTION_CVPR_2019["class_range"][n] for n in nc.CLASSES]
    used = np.zeros(len(got["dt_cat"]), bool)
    before = np.concatenate([[0], np.cumsum(s["count"])])
    worst_q = worst_y = 0.0
    for i in range(nc.I):
        con = nc.rows_sample(s["dets"][i], s["count"][i], s["poses"][i], list(range(Kc)), rng_, mv, st, Kc)
        n = int(z["dt_cnt"][i * Kc:(i + 1) * Kc].sum())
        a, b = i * M, int(z["dt_beg"][i * Kc])
        assert (got["dt_beg"][i * Kc:(i + 1) * Kc] - a == z["dt_beg"][i * Kc:(i + 1) * Kc] - b).all() and int(con["cnt"].sum()) == n
        for name in ("dt_xyz", "dt_size", "dt_vel", "dt_score", "dt_cat", "dt_attr", "dt_rank"):
            assert _same(got[name][a:a + n], z[name][b:b + n]), (i, name)
        assert (got["dt_src"][a:a + n] + before[i] == z["dt_gidx"][b:b + n]).all() and (got["dt_sample"][a:a + M] == i).all()
        # no row left out: every kept row's quaternion and yaw against the host's, inside the contract's interval
        dq = np.abs(got["dt_quat"][a:a + n] - z["dt_quat"][b:b + n])
        dy = np.abs(got["dt_yaw"][a:a + n] - z["dt_yaw"][b:b + n])
        assert (dq <= con["quat_bound"][:n]).all() and (dy <= con["yaw_bound"][:n]).all(), i
        with np.errstate(invalid="ignore", divide="ignore"):
            worst_q = max(worst_q, float(np.nanmax(np.where(con["quat_bound"][:n] > 0, dq / con["quat_bound"][:n], 0.0), initial=0.0)))
        worst_y = max(worst_y, float((dy / con["yaw_bound"][:n]).max(initial=0.0)))
        used[a:a + n] = True
    print(f"nusc_rows: worst fraction of the bound: dt_quat {worst_q:.3f}, dt_yaw {worst_y:.3f}")
    for name in ("dt_xyz", "dt_size", "dt_quat", "dt_vel", "dt_yaw", "dt_score", "dt_attr", "dt_rank"):
        assert (got[name][~used] == 0).all(), name
    assert (got["dt_cat"][~used] == Kc).all() and (got["dt_src"][~used] == -1).all() and used.sum() == len(z["dt_score"]) < int(s["count"].sum())


def test_match_and_accumulate_equal_the_host_on_host_records():
    from minddet_amd import nusc_eval as ne
    ev, s = _host(), nc.test_set()
    p = ne.pack_nusc(s["gt_records"], s["ego"], nc.CLASSES, device=DEV, dt_records=s["dt_records"])
    got = _tables(p)
    for name in EXACT + ("cat_off",):
        assert _same(got[name], ev.tables[name]), name
    n = int(ev.tables["cat_off"][-1])
    assert _same(got["order"][:n], ev.tables["order"][:n]) and n == len(ev.z["dt_score"])
    t = ev.tables
    assert (t["n_match"] > 0).any() and ((t["precision"] > 0) & (t["precision"] < 1)).any() and np.isnan(t["err"]).any() and (t["tp_err"] != 1).any()
    car = ev.z["gt_cnt"][0::nc.KC]
    for i in np.nonzero(car >= 63)[0]:                       # a match in every chunk of 64 ground truths
        g0 = ev.z["gt_beg"][i * nc.KC]
        hit = t["dtm"][3][(ev.z["dt_sample"] == i) & (ev.z["dt_cat"] == 0)]
        assert len({(g - g0) // 64 for g in hit[hit >= 0].tolist()}) == (car[i] + 63) // 64, i


def test_match_and_accumulate_equal_the_host_on_the_device_rows_read_back():
    from minddet_amd import nusc_eval as ne
    p, z = _rows()
    host = ne.NuscDetectionEval.from_arrays(z, nc.CLASSES).evaluate()
    got = _tables(p)
    for name in EXACT + ("cat_off",):
        assert _same(got[name], host.tables[name]), name
    n = int(host.tables["cat_off"][-1])
    assert _same(got["order"][:n], host.tables["order"][:n])
    # and the numpy statement of the operators on the same rows
    con = nc.tables(z, nc.KC, host.cfg["dist_ths"], host.periods(), REC, host.tp_index())
    for name in EXACT:
        assert _same(got[name], con[name]), name


def test_two_calls_give_the_same_bits_and_two_streams_agree():
    from minddet_amd import det_ops
    p, z = _rows()
    first = _tables(p)
    again = _tables(p)
    for name in EXACT:
        assert first[name].tobytes() == again[name].tobytes(), name
    # the rows from operands that start from other bytes: every element of the batch's samples is written
    s = nc.test_set()
    td, tc, tp = torch.from_numpy(s["dets"]).to(DEV), torch.from_numpy(s["count"]).to(DEV), torch.from_numpy(s["poses"]).to(DEV)
    consts = p.constants(nc.CLASSES)
    M, Kc, outs = nc.MAX_DET, nc.KC, []
    f64, i32 = torch.float64, torch.int32
    for fill in (0, 0x5a):
        Dt, C = nc.I * M, nc.I * Kc
        ops = [torch.empty(sh, dtype=dt, device=DEV) for sh, dt in (((Dt, 3), f64), ((Dt, 3), f64), ((Dt, 4), f64), ((Dt, 2), f64), ((Dt,), f64), ((Dt,), f64),
                                                                    ((Dt,), i32), ((Dt,), i32), ((Dt,), i32), ((Dt,), i32), ((C,), i32), ((C,), i32))]
        for t in ops:
            t.view(torch.uint8).fill_(fill)
        det_ops.nusc_rows(td, tc, tp, *consts, 0, *ops)
        outs.append([t.cpu().numpy().tobytes() for t in ops])
    assert outs[0] == outs[1]
    from minddet_amd import nusc_eval as ne
    assert outs[0] == [z[n].tobytes() for n in ne.DT_NAMES]
    # two streams: each runs rows, match and accumulate on its own pack
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    res = []
    for st in streams:
        with torch.cuda.stream(st):
            res.append(_tables(_device_rows()))
    torch.cuda.synchronize()
    for t in res:
        for name in EXACT:
            assert t[name].tobytes() == first[name].tobytes(), name


def test_evaluate_device_and_evaluate_nusc_return_what_the_host_judge_returns():
    from minddet.models import Config, build_detector
    from minddet_amd import nusc_eval as ne
    ev, s = _host(), nc.test_set()
    same = lambda a, b: repr(a) == repr(b)                   # dicts with NaN entries
    got = ne.NuscDetectionEval(s["gt_records"], s["dt_records"], s["ego"], nc.CLASSES).evaluate(backend="device", device=DEV).summarize()
    assert same(got, ev.summarize()) and got["mean_ap"] > 0.05
    # the detector's own output: the tiny CenterPoint config, ground truth made around its boxes
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "centerpoint", "centerpoint_pp_tiny.py"))
    m = build_detector(dict(cfg.model, seed=9, cp_post=True), cfg.train_cfg, cfg.test_cfg).to(DEV)
    g = torch.Generator().manual_seed(11)
    x = torch.relu(torch.randn((3, 128, 128, 64), generator=g)) * (torch.rand((3, 128, 128, 1), generator=g) < 0.1)
    dets, count = m.forward(x.to(torch.bfloat16).to(DEV))
    torch.cuda.synchronize()
    assert tuple(dets.shape) == (3, 120, 11) and int(count.sum()) > 0
    names = [n for task in cfg.tasks for n in task["class_names"]]
    poses = s["poses"][[0, 9, 10]]
    ego = poses[:, 11:14]
    recs = ne.dets_to_nusc(dets.cpu().numpy(), count.cpu().numpy(), poses, names)
    gts = [dict(r, translation=[r["translation"][0] + 0.25 * (j % 7), r["translation"][1], r["translation"][2]], num_pts=4,
                attribute_name="" if j % 4 == 0 else r["attribute_name"]) for j, r in enumerate(recs) if j % 3]
    got = m.evaluate_nusc(dets, count, poses, gts, ego)
    packed = ne.pack_nusc(gts, ego, names, device=DEV).add_dets(dets, count, poses, 0)
    results = ne.rows_to_results(packed)
    assert set(results) == {"results", "meta"} and list(results["results"]) == [0, 1, 2]
    flat = [r for tok in results["results"] for r in results["results"][tok]]
    host = ne.NuscDetectionEval(gts, flat, ego, names).evaluate()
    assert same(got, host.summarize()) and got["mean_ap"] > 0 and len(flat) > 0
    assert {"sample_token", "translation", "size", "rotation", "velocity", "detection_name", "detection_score", "attribute_name"} <= set(flat[0])
