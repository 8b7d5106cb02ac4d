"""Golden vectors for the CenterPoint multi-sweep input, produced BY THE REFERENCE: the nuScenes branch of
LoadPointCloudFromFile.__call__ with its own read_file, remove_close and read_sweep
(minddet/models/centerpoint/det3d_ms/datasets/pipelines/loading.py:18-80, 123-159).  loading.py is loaded as a file under stub
packages (its `..registry.PIPELINES` is an identity register_module, as in gen_cp_targets.py); the clouds are written as 5-wide .bin
files in a temporary directory, as nuScenes stores them; numpy's generator is seeded and np.random.choice is wrapped during the call
(Capture of gen_pc_augment.py), so the sweep order the loader drew is recorded and becomes the operator's table.  Run here only:

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_cp_sweeps.py <path of the reference checkout>

Nothing of the reference is copied: the file holds seeded inputs, the recorded order and what the routines returned.

Cases: `small` (B = 1, the key frame and two sweeps), `pad` (a padding sweep: transform_matrix None, time lag 0, still filtered),
`batch` (B = 2 with different orders), `plants` (rows planted at remove_close's boundaries: |x| or |y| exactly the radius, nextafter
on either side, one coordinate inside and one outside, negative signs, -0.0, a NaN coordinate; and one row whose transformed x cancels
to below 1e-6 of its terms).

Asserted while generating (tests/cp_sweeps_contract.py): the contract keeps, orders and stamps exactly as the reference did; the
reference's xyz meets the contract's condition and its cap; in `plants` the planted rows are decided as listed and the interval of the
cancelling coordinate is not a single fp32 value.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from gen_cp_targets import PKG, _load  # noqa: E402
from gen_pc_augment import Capture  # noqa: E402

RADIUS = 1.0          # read_sweep's min_distance
f = np.float32


def reference_loading(ref_root):
    for pkg in ("det3d_ms", "det3d_ms.datasets", "det3d_ms.datasets.pipelines"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    registry = types.ModuleType("det3d_ms.datasets.registry")
    registry.PIPELINES = types.SimpleNamespace(register_module=lambda cls: cls)
    sys.modules["det3d_ms.datasets.registry"] = registry
    return _load("det3d_ms.datasets.pipelines.loading", os.path.join(ref_root, PKG, "datasets/pipelines/loading.py"))


def cloud(rng, n):
    """[n,5] fp32 as a nuScenes .bin holds it: x, y, z, intensity, ring index; about one row in nine is within the radius"""
    return np.stack([rng.normal(0, 2.5, n), rng.normal(0, 2.5, n), rng.uniform(-3, 1, n), rng.uniform(0, 255, n), rng.integers(0, 32, n)], 1).astype(f)


def pose(rng):
    """a sweep's 4x4 into the key frame, float64: yaw within 0.3 rad, a small tilt, a translation within 8 m"""
    yaw, pitch, roll = rng.uniform(-0.3, 0.3), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    m = np.eye(4)
    m[:3, :3] = rz @ ry @ rx
    m[:3, 3] = rng.uniform(-8, 8, 3) * (1, 1, 0.05)
    return m


def tables(lengths, has_matrix, matrices, lags, order):
    """the operator's tables for one sample whose frames lie back to back from row 0: the key frame, then the sweeps in `order`"""
    start = np.concatenate([[0], np.cumsum(lengths)])
    S = len(lengths)
    seg, tf = np.zeros((1, S, 2), np.int32), np.tile(np.eye(4)[:3].reshape(12), (1, S, 1))
    lag, flags = np.zeros((1, S)), np.zeros((1, S), np.int32)
    for s, i in enumerate([0] + [1 + int(k) for k in order]):
        seg[0, s] = (start[i], start[i + 1])
        if i:
            lag[0, s], flags[0, s] = lags[i], 1 | (2 if has_matrix[i] else 0)
            if has_matrix[i]:
                tf[0, s] = matrices[i][:3].reshape(12)
    return seg, tf, lag, flags


def drive(loading, tmp, tag, seed, frames, matrices, lags):
    """one sample through LoadPointCloudFromFile.__call__; frames[0] the key frame; matrices[i] None = transform_matrix None"""
    from tests import cp_sweeps_contract as sc

    paths = []
    for i, fr in enumerate(frames):
        paths.append(os.path.join(tmp, f"{tag}_{i}.bin"))
        fr.tofile(paths[-1])
    info = dict(lidar_path=paths[0], sweeps=[dict(lidar_path=paths[i], transform_matrix=matrices[i], time_lag=lags[i]) for i in range(1, len(frames))])
    res = dict(lidar=dict(nsweeps=len(frames)), virtual=False)
    np.random.seed(seed)
    with Capture() as cap:
        res, _ = loading.LoadPointCloudFromFile(dataset="NuScenesDataset")(res, info)
    assert [k for k, _, _ in cap.draws] == ["choice"]
    order = np.asarray(cap.draws[0][2], np.int64)
    combined = res["lidar"]["combined"]
    assert combined.dtype == np.float32 and combined.shape[1] == 5
    pool = np.concatenate(frames)
    lengths = np.array([len(fr) for fr in frames], np.int32)
    has = np.array([m is not None for m in matrices])
    mats = np.stack([np.eye(4) if m is None else m for m in matrices])
    seg, tf, lag, flags = tables(lengths, has, mats, lags, order)
    c = sc.merge(pool, seg, tf, lag, flags, RADIUS)
    assert c["status"].tolist() == [0] and int(c["offsets"][-1]) == len(combined), (tag, c["offsets"].tolist(), len(combined))
    full = np.zeros_like(c["points"])
    full[:len(combined)] = combined
    differ, total = sc.check(full, c["offsets"], c, what=tag)      # keeps, order, columns 3-4 exact; xyz within the condition and the cap
    out = dict(points=pool, lengths=lengths, has_matrix=has, matrices=mats, time_lags=np.asarray(lags, np.float64), order=order,
               seed=np.int64(seed), combined=combined, seg_range=seg[0], seg_flags=flags[0])
    return out, c, differ


def scene(loading, tmp, tag, seed, n, nsweeps, pad=()):
    rng = np.random.default_rng(seed)
    frames = [cloud(rng, int(n * rng.uniform(0.8, 1.2))) for _ in range(nsweeps)]
    matrices = [None] + [None if i in pad else pose(rng) for i in range(1, nsweeps)]
    lags = [0.0] + [0.0 if i in pad else float(0.05 * i + rng.uniform(0, 0.004)) for i in range(1, nsweeps)]
    return drive(loading, tmp, tag, seed, frames, matrices, lags)


PLANTS = [  # (x, y, kept) at radius 1: dropped iff |x| < 1 and |y| < 1, both strict
    (f(1.0), f(0.5), True), (f(0.5), f(1.0), True), (f(-1.0), f(-0.5), True), (f(0.5), f(-1.0), True),
    (np.nextafter(f(1), f(0)), f(0.5), False), (np.nextafter(f(1), f(2)), f(0.5), True),
    (f(0.5), np.nextafter(f(1), f(0)), False), (f(0.5), np.nextafter(f(1), f(2)), True),
    (-np.nextafter(f(1), f(0)), f(-0.5), False), (-np.nextafter(f(1), f(2)), f(-0.5), True),
    (np.nextafter(f(1), f(0)), -np.nextafter(f(1), f(0)), False),
    (f(0.5), f(5.0), True), (f(5.0), f(0.5), True), (f(-0.25), f(-7.0), True),
    (f(-0.0), f(0.0), False), (f(0.0), f(-0.0), False), (f(0.3), f(-0.3), False),
    (f(np.nan), f(0.5), True), (f(0.5), f(np.nan), True), (f(np.nan), f(np.nan), True),
]


def case_plants(loading, tmp):
    from tests import cp_sweeps_contract as sc

    for seed in range(700, 760):
        rng = np.random.default_rng(seed)
        n = len(PLANTS)
        planted = np.stack([np.array([x for x, _, _ in PLANTS], f), np.array([y for _, y, _ in PLANTS], f), rng.uniform(-2, 0, n).astype(f),
                            np.arange(n, dtype=f) + f(0.5), np.zeros(n, f)], 1)
        m = pose(rng)
        # a row whose transformed x cancels: x = fp32(-(m01 y + m02 z + m03) / m00), the residue is the rounding of x
        y, z = f(3.25), f(-1.5)
        x = f(-(m[0, 1] * np.float64(y) + m[0, 2] * np.float64(z) + m[0, 3]) / m[0, 0])
        cancel = np.array([[x, y, z, 99.5, 0]], f)
        key = np.concatenate([planted, cloud(rng, 12)])                      # the key frame keeps every row, the planted ones included
        with_tf = np.concatenate([planted, cancel, cloud(rng, 12)])
        without = np.concatenate([cloud(rng, 6), planted])                   # a padding sweep: filtered, not transformed
        out, c, differ = drive(loading, tmp, "plants", seed, [key, with_tf, without], [None, m, None], [0.0, 0.05, 0.0])
        v, e = sc.transform(m[:3].reshape(12), cancel[:, :3])
        terms = abs(m[0, 0] * np.float64(x)) + abs(m[0, 1] * np.float64(y)) + abs(m[0, 2] * np.float64(z)) + abs(m[0, 3])
        assert abs(v[0, 0]) < 1e-6 * terms
        if f(v[0, 0] - e[0, 0]) != f(v[0, 0] + e[0, 0]) and differ == 0:
            break
    else:
        raise AssertionError("no seed gives a cancelling row with a non-degenerate interval")
    kept = np.array([k for _, _, k in PLANTS])
    got = out["combined"]
    ids = got[:, 3]
    n_key = len(key)
    assert same_ids(ids[:n_key], key[:, 3])                                  # quirk (a): the key frame is not filtered
    rest = ids[n_key:]
    for fr in ((with_tf, without) if out["order"].tolist() == [0, 1] else (without, with_tf)):
        want = fr[sc.keep_mask(fr, RADIUS), 3]
        assert same_ids(rest[:len(want)], want)
        rest = rest[len(want):]
        planted_ids = np.arange(n, dtype=f) + f(0.5)
        assert np.array_equal(np.isin(planted_ids, want), kept)               # the planted rows are decided as listed
    assert len(rest) == 0
    out["plant_kept"] = kept
    out["cancel_row"] = np.int32(n_key + n)                                  # its row in the pool
    print("plants: seed", int(out["seed"]), "order", out["order"].tolist(), "cancel v", v[0, 0], "+-", e[0, 0])
    return out


def same_ids(a, b):
    return len(a) == len(b) and np.array_equal(a, b)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    loading = reference_loading(sys.argv[1])
    z, samples = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        samples["small"] = [scene(loading, tmp, "small", 11, 200, 3)[0]]
        samples["pad"] = [scene(loading, tmp, "pad", 23, 90, 4, pad=(2, 3))[0]]
        for sd in range(31, 200):                                             # two samples whose draws differ
            two = [scene(loading, tmp, "batch0", 30, 100, 3)[0], scene(loading, tmp, "batch1", sd, 100, 3)[0]]
            if two[0]["order"].tolist() != two[1]["order"].tolist():
                break
        samples["batch"] = two
        samples["plants"] = [case_plants(loading, tmp)]
    for name, ss in samples.items():
        z[f"{name}_n"] = np.int32(len(ss))
        for i, s in enumerate(ss):
            z.update({f"{name}_{i}_{k}": v for k, v in s.items()})
        print(name, [(s["lengths"].tolist(), s["order"].tolist(), len(s["combined"])) for s in ss])
    z["cases"] = np.array(list(samples))
    z["radius"] = np.float32(RADIUS)
    z["numpy_version"] = np.array(np.__version__)
    out = os.path.join(HERE, "cp_sweeps_vectors.npz")
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 100 * 1000


if __name__ == "__main__":
    main()
