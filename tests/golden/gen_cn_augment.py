"""Generate tests/golden/cn_augment_vectors.npz FROM THE REFERENCE'S OWN COCOHP.preprocess_fn AND color_aug.

Run once in the build container (needs the reference checkout; never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_cn_augment.py <path of the reference checkout>

Source of truth: minddet/models/centernet/src/dataset.py (COCOHP.preprocess_fn, training branch, color_aug=True) with src/image.py,
each loaded as a file under the import shim of gen_cn_targets.py.  cv2 is a stub (the project does not depend on cv2):
getAffineTransform is the float64 three-point solve of tests/cnaug_contract.py (recorded), cvtColor is the fp32 grey formula
(0.114 B + 0.587 G) + 0.299 R, imdecode returns a blank image of the wanted size and warpAffine returns a seeded uint8 image, which is
recorded.  So the matrix solve, the warp and the grey arithmetic are NOT pinned by this fixture; the random block (every draw, c, s,
the flip), the points handed to the solve, color_aug's chain and the normalisation are.  preprocess_fn itself runs, on an
object.__new__(COCOHP), under seeded np.random and random and a fresh RandomState; np.random.choice / randint / randn / random, the
RandomState's uniform / normal and random.shuffle are wrapped so that every drawn value and the shuffled order are recorded.  Nothing
of the reference is copied: the fixture holds seeded inputs and what the reference's code returned for them.  The arithmetic
recorded is the one of the NumPy that runs this script (>= 2: fp32 scalars stay fp32); the version is stored in the file.

Samples (input 24 x 40, down_ratio 4; each sample takes the first seed from its base on that gives the wanted flip, order and clips,
and whose grey mean passes the sensitivity check of tests/test_cn_augment_cpu.py):
  0  rand_crop, 120 x 200 (narrower than 2 x 128 on both axes: _get_border halves), flipped, order 0
  1  scale / shift, 480 x 640, the clip of c[0] and the clip of s active, the clip of c[1] inactive, not flipped, order 1
  2  rand_crop, 480 x 640, not flipped, order 2
  3  scale / shift, 333 x 500, flipped, order 3
  4  rand_crop, 64 x 64, order 4
  5  scale / shift, 500 x 375, order 5
  6  rand_crop, 427 x 640, color_aug False
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests import cnaug_contract as cc                      # noqa: E402
from tests.golden import gen_cn_targets as gt               # noqa: E402

f32 = np.float32
IN_HW, DOWN = (24, 40), 4
MEAN = np.array([0.40789654, 0.44719302, 0.47026115], f32)
STD = np.array([0.28863828, 0.27408164, 0.27809835], f32)
EIG_VAL = np.array([0.2141788, 0.01817699, 0.00341571], f32)
EIG_VEC = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408], [-0.56089297, 0.71832671, 0.41158938]], f32)
NAMES = ("brightness_", "contrast_", "saturation_")
REC = dict(draws=[], rng=[], order=None, points=[], matrices=[], cs=[], warped=None)


def _solve(src, dst):
    REC["points"].append((np.array(src, f32), np.array(dst, f32)))
    m = cc.three_point_solve(src, dst)
    REC["matrices"].append(m)
    return m


def _grey(image, code):
    return (f32(cc.GREY[0]) * image[..., 0] + f32(cc.GREY[1]) * image[..., 1]) + f32(cc.GREY[2]) * image[..., 2]


class RecordingRng:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def uniform(self, **kw):
        v = self.rng.uniform(**kw)
        REC["rng"].append(("uniform", np.asarray(v, np.float64)))
        return v

    def normal(self, **kw):
        v = self.rng.normal(**kw)
        REC["rng"].append(("normal", np.asarray(v, np.float64)))
        return v


def run_sample(ds, img_mod, seed, image_hw, rand_crop, color_aug):
    import random

    for k in ("draws", "rng", "points", "matrices", "cs"):
        del REC[k][:]
    REC["order"] = None
    np.random.seed(seed)
    random.seed(seed)
    REC["warped"] = np.random.default_rng(seed + 1000).integers(0, 256, IN_HW + (3,), dtype=np.uint8)
    cv2 = sys.modules["cv2"]
    cv2.getAffineTransform, cv2.cvtColor = _solve, _grey
    cv2.warpAffine = lambda img, m, size, flags=None: REC["warped"].copy()
    gt.STATE["image_hw"] = tuple(image_hw)

    real = {k: getattr(np.random, k) for k in ("choice", "randint", "randn", "random")}

    def wrap(name):
        def f(*a, **kw):
            v = real[name](*a, **kw)
            REC["draws"].append((name, float(v)))
            return v
        return f

    class Shuffle:
        @staticmethod
        def shuffle(fs):
            random.shuffle(fs)
            REC["order"] = [f.__name__ for f in fs]

    op = object.__new__(ds.COCOHP)
    op.run_mode = "train"
    op.data_opt = types.SimpleNamespace(max_objs=8, input_res_train=IN_HW, rand_crop=rand_crop, scale=0.4, shift=0.1, flip_prop=0.5,
                                        down_ratio=DOWN, num_classes=5, color_aug=color_aug, eig_val=EIG_VAL, eig_vec=EIG_VEC)
    op.net_opt = types.SimpleNamespace(mse_loss=False, dense_wh=False, cat_spec_wh=False, reg_offset=True)
    op.mean, op.std = MEAN.reshape(1, 1, 3), STD.reshape(1, 1, 3)
    op._data_rng = RecordingRng(seed)
    saved, inner = img_mod.random, ds.get_affine_transform

    def recording(center, scale, rot, output_size, **kw):      # the (c, s) preprocess_fn hands over: an fp32 pair and a float64
        REC["cs"].append((np.array(center, f32), np.float64(scale), float(rot)))
        return inner(center, scale, rot, output_size, **kw)

    try:
        ds.get_affine_transform = recording
        for k in real:
            setattr(np.random, k, wrap(k))
        img_mod.random = Shuffle
        inp = op.preprocess_fn(b"", 0, np.zeros((0, 4), f32), np.zeros((0,), np.int32))[0]
    finally:
        for k, v in real.items():
            setattr(np.random, k, v)
        img_mod.random, ds.get_affine_transform = saved, inner
    assert len(REC["cs"]) == 2 and all(r == 0.0 for _, _, r in REC["cs"]) and REC["cs"][0][1] == REC["cs"][1][1]
    assert np.array_equal(REC["cs"][0][0], REC["cs"][1][0]) and isinstance(s_py := REC["cs"][0][1], np.float64)
    names = [n for n, _ in REC["draws"]]
    assert names == (["choice", "randint", "randint", "random"] if rand_crop else ["randn", "randn", "randn", "random"]), names
    assert len(REC["matrices"]) == 2
    draws = np.array([v for _, v in REC["draws"]], np.float64)
    col = np.zeros(8)
    if color_aug:
        kinds = [k for k, _ in REC["rng"]]
        assert kinds == ["uniform"] * 3 + ["normal"] and sorted(REC["order"]) == sorted(NAMES)
        for fname, (_, v) in zip(REC["order"], REC["rng"][:3]):
            col[NAMES.index(fname)] = 1.0 + float(v)
        col[3:6] = np.dot(EIG_VEC, EIG_VAL * REC["rng"][3][1])                        # lighting_'s own expression
        col[6] = cc.ORDERS.index(tuple(NAMES.index(n) for n in REC["order"]))
    src_in, _ = REC["points"][0]
    return dict(size=np.array(image_hw, np.int32), draws=draws, colour=col, c=REC["cs"][0][0], s=s_py, flipped=bool(draws[3] < 0.5),
                trans_input=REC["matrices"][0], trans_output=REC["matrices"][1], src_points=src_in, warped=REC["warped"].copy(),
                inp=np.ascontiguousarray(inp.transpose(1, 2, 0)).astype(f32), rand_crop=rand_crop, color_aug=color_aug, seed=seed)


def sensitive(s):
    """the check of test_cn_augment_cpu.py's mean sensitivity on this sample: bf16 outputs that move when gs_mean is summed in reverse"""
    x32 = (s["warped"].astype(f32) / f32(255.0)).astype(f32)
    a = cc.bf16_bits(cc.colour(x32, s["colour"], MEAN, STD)["y"])
    b = cc.bf16_bits(cc.colour(x32, s["colour"], MEAN, STD, gs_mean=cc.reversed_sum(cc.grey(x32)) / x32[..., 0].size)["y"])
    return cc.bf16_differences(a, b)


def main():
    ds = gt.reference_dataset(sys.argv[1])
    img_mod = sys.modules["src.image"]
    wanted = [((120, 200), True, True, dict(flipped=True, order=0)),
              ((480, 640), False, True, dict(flipped=False, order=1, clips=(True, False, True))),
              ((480, 640), True, True, dict(flipped=False, order=2)),
              ((333, 500), False, True, dict(flipped=True, order=3)),
              ((64, 64), True, True, dict(order=4)),
              ((500, 375), False, True, dict(order=5)),
              ((427, 640), True, False, dict())]
    out = dict(numpy_version=np.array(np.__version__), input_hw=np.array(IN_HW, np.int32), down_ratio=np.int32(DOWN), mean=MEAN, std=STD,
               eig_val=EIG_VAL, eig_vec=EIG_VEC, scale=np.float64(0.4), shift=np.float64(0.1), flip_prop=np.float64(0.5))
    rows = []
    for i, (hw, rand_crop, color_aug, want) in enumerate(wanted):
        seed = 3000 + 100 * i
        while True:
            s = run_sample(ds, img_mod, seed, hw, rand_crop, color_aug)
            d = s["draws"]
            ok = ("flipped" not in want or s["flipped"] == want["flipped"]) and ("order" not in want or int(s["colour"][6]) == want["order"])
            if "clips" in want:
                ok = ok and (abs(d[0]) > 2.0, abs(d[1]) > 2.0, abs(d[2]) > 1.0) == want["clips"]
            if ok and color_aug:
                ndiff, _ = sensitive(s)
                ok = ndiff * 10000 <= s["inp"].size
            if ok:
                break
            seed += 1
        rows.append(s)
        print(i, "seed", seed, "size", hw, "rand_crop", rand_crop, "draws", s["draws"].tolist(), "flipped", s["flipped"], "order", int(s["colour"][6]))
    for k in rows[0]:
        out[k] = np.stack([np.asarray(r[k]) for r in rows])
    path = os.path.join(HERE, "cn_augment_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
