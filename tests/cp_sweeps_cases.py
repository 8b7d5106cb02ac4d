"""What tests/test_cp_sweeps_cpu.py, tests/test_cp_sweeps_gpu.py and tools/centerpoint_sweeps_step.py share about the multi-sweep
input: the fixture (tests/golden/cp_sweeps_vectors.npz, written by tests/golden/gen_cp_sweeps.py from the reference's loader) by
case, the operator's tables for a case (the samples' pools back to back), the contract (tests/cp_sweeps_contract.py) evaluated on
them, and a seeded scene for the shapes the fixture does not hold."""
import functools
import os

import numpy as np

from tests import cp_sweeps_contract as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cp_sweeps_vectors.npz")
NAMES = ("small", "pad", "batch", "plants")


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """-> the case's samples, a tuple of dicts"""
    z = np.load(GOLD)
    out = []
    for i in range(int(z[f"{name}_n"])):
        pre = f"{name}_{i}_"
        out.append({k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})
    return tuple(out)


def radius():
    return float(np.load(GOLD)["radius"])


@functools.lru_cache(maxsize=None)
def case_tables(name):
    """the operator's operands for the case, from the fixture's own tables: dict(points [N,5], seg_range [B,S,2], transforms
    [B,S,12], time_lag [B,S], seg_flags [B,S])"""
    ss = fixture_case(name)
    B, S = len(ss), len(ss[0]["lengths"])
    seg, tf = np.zeros((B, S, 2), np.int32), np.zeros((B, S, 12))
    lag, flags = np.zeros((B, S)), np.zeros((B, S), np.int32)
    base = 0
    for b, s in enumerate(ss):
        frames = [0] + [1 + int(k) for k in s["order"]]
        seg[b] = s["seg_range"] + base
        flags[b] = s["seg_flags"]
        tf[b] = s["matrices"][frames][:, :3].reshape(S, 12)
        lag[b] = s["time_lags"][frames]
        base += len(s["points"])
    return dict(points=np.concatenate([s["points"] for s in ss]), seg_range=seg, transforms=tf, time_lag=lag, seg_flags=flags)


@functools.lru_cache(maxsize=None)
def contract_case(name):
    t = case_tables(name)
    return sc.merge(t["points"], t["seg_range"], t["transforms"], t["time_lag"], t["seg_flags"], radius())


def reference_cloud(name):
    """what the reference returned for the case's samples, back to back -> (points [n,5] fp32, offsets [B+1])"""
    ss = fixture_case(name)
    return np.concatenate([s["combined"] for s in ss]), np.concatenate([[0], np.cumsum([len(s["combined"]) for s in ss])]).astype(np.int32)


def pose(rng, scale=8.0):
    """a 4x4 float64: yaw within 0.3 rad, a small tilt, a translation within `scale` metres"""
    yaw, pitch = rng.uniform(-0.3, 0.3), rng.uniform(-0.02, 0.02)
    cz, sz, cy, sy = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    m = np.eye(4)
    m[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    m[:3, 3] = rng.uniform(-scale, scale, 3) * (1, 1, 0.05)
    return m


def scene(seed, lengths, fin=5, spread=2.5, flags=None, scale=8.0):
    """a seeded pool for segment lengths [B][S] laid back to back: dict of the operator's operands; flags [B][S] (None: segment 0 of a
    sample plain, the others filtered and transformed)"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    B, S = lengths.shape
    n = int(lengths.sum())
    pts = np.stack([rng.normal(0, spread, n), rng.normal(0, spread, n), rng.uniform(-3, 1, n), rng.uniform(0, 255, n), rng.integers(0, 32, n)], 1)
    end = np.cumsum(lengths.reshape(-1)).reshape(B, S)
    seg = np.stack([end - lengths, end], 2).astype(np.int32)
    tf = np.stack([pose(rng, scale)[:3].reshape(12) for _ in range(B * S)]).reshape(B, S, 12)
    lag = rng.uniform(0, 0.5, (B, S))
    if flags is None:
        flags = np.full((B, S), 3, np.int32)
        flags[:, 0] = 0
    return dict(points=pts.astype(np.float32)[:, :fin].copy(), seg_range=seg, transforms=tf, time_lag=lag, seg_flags=np.asarray(flags, np.int32))
