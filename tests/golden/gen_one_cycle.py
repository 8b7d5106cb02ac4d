"""Golden vectors for the OneCycle schedule, produced BY THE REFERENCE: OneCycle(...).get_lr() of
minddet/models/centerpoint/det3d_ms/solver/learning_schedules_fastai.py (the file imports only numpy, so it is loaded as it is, by
path, with no shim).  Run here only (needs the reference checkout; REFERENCE_ROOT names it, default /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/gen_one_cycle.py

Only inputs and outputs are stored: per case the five constructor arguments and the two float32 arrays."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
# name -> (total_step, lr_max, div_factor, pct_start, moms)
CASES = {"a": (100, 1e-3, 10, 0.4, [0.95, 0.85]), "b": (7, 3e-3, 25, 0.3, [0.9, 0.8])}


def main():
    root = os.environ.get("REFERENCE_ROOT", "/root/reference")
    path = os.path.join(root, "minddet", "models", "centerpoint", "det3d_ms", "solver", "learning_schedules_fastai.py")
    spec = importlib.util.spec_from_file_location("learning_schedules_fastai", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for name, (total, lr_max, div, pct, moms) in CASES.items():
        lrs, ms = mod.OneCycle(total, lr_max, div, pct, list(moms)).get_lr()
        assert lrs.dtype == ms.dtype == np.float32 and lrs.shape == ms.shape == (total,)
        out[name + "_args"] = np.array([total, lr_max, div, pct] + list(moms), np.float64)
        out[name + "_lrs"], out[name + "_moms"] = lrs, ms
    np.savez(os.path.join(HERE, "one_cycle_vectors.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
