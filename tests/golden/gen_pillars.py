"""Generate tests/golden/pillar_vectors.npz FROM THE REFERENCE'S OWN points_to_voxel.

Run once in the build container (needs the reference checkout; never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_pillars.py <path of the reference checkout>

Source of truth: minddet/models/centerpoint/det3d_ms/ops/point_cloud/point_cloud_ops.py, loaded as a file under the same import-time
shim tests/golden/gen_golden.py uses (numba.jit -> identity: numba is not installed, and the jitted loop is plain Python).  Nothing of
the reference is copied: the fixture holds seeded clouds and what the reference returned for them, per sample, stacked over the batch
with the batch index in front of each voxel's (z, y, x).

Cases (all over x, y in [-6.4, 6.4) m):
  capped    F = 5, 0.2 m cells (64 x 64 x 1), max_points 5, max_voxels 700 < the cloud's cells; two samples of different length
  uncapped  the same clouds with max_voxels above the cloud's cells
  f4        F = 4, 0.4 m x 0.4 m x 2 m cells (32 x 32 x 4), max_points 3, capped
Plants of sample 0: points exactly on cell boundaries and their fp32 neighbours, on the range edges (the lower edge is inside, the
upper outside), -0.0 coordinates, a cell with many more than max_points points early in the cloud, points outside the range in each
axis and direction, and a dense cell that first appears after max_voxels other cells exist (dropped when capped, kept when not)."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def reference_points_to_voxel(ref_root):
    nb = types.ModuleType("numba")

    def _ident(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    nb.jit = nb.njit = _ident
    sys.modules["numba"] = nb
    path = os.path.join(ref_root, "minddet/models/centerpoint/det3d_ms/ops/point_cloud/point_cloud_ops.py")
    spec = importlib.util.spec_from_file_location("ref_point_cloud_ops", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.points_to_voxel


def cloud(rng, n, F, lo, hi, zlo, zhi, vs, dense_late):
    """a seeded cloud with the plants; x of the random part stays below 4.0 so that the late dense cell (x ~ 6.1) is new"""
    f32 = np.float32
    body = np.empty((n, F), f32)
    body[:, 0] = rng.uniform(lo - 0.5, 4.0, n)
    body[:, 1] = rng.uniform(lo - 0.5, hi + 0.5, n)
    body[:, 2] = rng.uniform(zlo - 0.3, zhi + 0.3, n)
    body[:, 3:] = rng.uniform(0, 1, (n, F - 3))
    plants = []
    # cell boundaries and their fp32 neighbours, in x and in y
    for k in range(0, int(round((hi - lo) / vs)) + 1):
        e = f32(lo) + f32(k) * f32(vs)
        for v in (e, np.nextafter(e, f32(-100)), np.nextafter(e, f32(100)), f32(lo + k * vs)):
            plants.append([v, f32(rng.uniform(lo, hi)), 0.0])
            plants.append([f32(rng.uniform(lo, 4.0)), v, 0.0])
    # range edges in z, -0.0, outside in each axis and direction
    plants += [[0.5, 0.5, zlo], [0.5, 0.5, zhi], [0.5, 0.5, np.nextafter(f32(zhi), f32(-100))], [-0.0, -0.0, -0.0], [-0.0, 1.0, 0.0],
               [lo - 1, 0, 0], [hi + 1, 0, 0], [0, lo - 1, 0], [0, hi + 1, 0], [0, 0, zlo - 1], [0, 0, zhi + 1]]
    pl = np.zeros((len(plants), F), f32)
    pl[:, :3] = np.asarray(plants, f32)
    pl[:, 3:] = rng.uniform(0, 1, (len(pl), F - 3))
    early = np.zeros((17, F), f32)                       # a dense cell at the start: more than max_points points, kept
    early[:, 0] = rng.uniform(1.01, 1.19, 17)
    early[:, 1] = rng.uniform(-2.19, -2.01, 17)
    early[:, 3:] = rng.uniform(0, 1, (17, F - 3))
    late = np.zeros((dense_late, F), f32)                # a dense cell that appears last
    late[:, 0] = rng.uniform(6.01, 6.19, dense_late)
    late[:, 1] = rng.uniform(3.01, 3.19, dense_late)
    late[:, 3:] = rng.uniform(0, 1, (dense_late, F - 3))
    mid = np.concatenate([body, pl])
    mid = mid[rng.permutation(len(mid))]
    # the early cell's points again in the middle: they arrive when the voxel is full
    return np.concatenate([early, mid[:len(mid) // 2], early[:3] + f32(0), mid[len(mid) // 2:], late]).astype(f32)


def run(p2v, samples, vs, rng_, max_points, max_voxels):
    vox, coo, num, cnt = [], [], [], []
    for b, pts in enumerate(samples):
        v, c, n = p2v(pts, vs, rng_, max_points=max_points, reverse_index=True, max_voxels=max_voxels)
        vox.append(v)
        coo.append(np.concatenate([np.full((max_voxels, 1), b, np.int32) * (n[:, None] > 0), c], 1).astype(np.int32))
        num.append(n)
        cnt.append(int((n > 0).sum()))                   # every voxel the loop opens gets its first point
    return np.stack(vox), np.stack(coo), np.stack(num), np.asarray(cnt, np.int32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_root = sys.argv[1]
    p2v = reference_points_to_voxel(ref_root)
    rng = np.random.default_rng(20240607)
    out = {}
    s5 = [cloud(rng, 3300, 5, -6.4, 6.4, -5.0, 3.0, 0.2, 24), cloud(rng, 500, 5, -6.4, 6.4, -5.0, 3.0, 0.2, 9)]
    s4 = [cloud(rng, 1400, 4, -6.4, 6.4, -5.0, 3.0, 0.4, 11)]
    cases = dict(capped=(s5, (0.2, 0.2, 8.0), (-6.4, -6.4, -5.0, 6.4, 6.4, 3.0), 5, 700),
                 uncapped=(s5, (0.2, 0.2, 8.0), (-6.4, -6.4, -5.0, 6.4, 6.4, 3.0), 5, 2600),
                 f4=(s4, (0.4, 0.4, 2.0), (-6.4, -6.4, -5.0, 6.4, 6.4, 3.0), 3, 900))
    out["cases"] = np.asarray(sorted(cases))
    for name, (samples, vs, rg, mp, mv) in cases.items():
        v, c, n, k = run(p2v, samples, vs, rg, mp, mv)
        if name != "uncapped":                            # (the same clouds as `capped`)
            out[name + "_points"] = np.concatenate(samples)
            out[name + "_offsets"] = np.cumsum([0] + [len(s) for s in samples]).astype(np.int32)
        out[name + "_voxel_size"], out[name + "_range"] = np.asarray(vs, np.float32), np.asarray(rg, np.float32)
        out[name + "_max_points"], out[name + "_max_voxels"] = np.int32(mp), np.int32(mv)
        out[name + "_voxels"], out[name + "_coors"], out[name + "_num_points"], out[name + "_voxel_num"] = v, c, n, k
        print(name, "voxel_num", k, "of", mv, "full voxels", int((n == mp).sum()))
    dst = os.path.join(HERE, "pillar_vectors.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
