"""-m gpu: a plain bench.py run (tiny Faster R-CNN config) -- its line carries the headline fields and none of those --full measures, and
--dump-outputs holds what the last timed step returned: the detections of one forward pass of the same model on the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]


def test_plain_run_dumps_the_last_timed_steps_outputs(tmp_path):
    cfg_path = os.path.join(ROOT, "configs", "faster_rcnn", "faster_rcnn_tiny.py")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
           "--config", cfg_path, "--dump-outputs", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-4000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "images/sec" and j["higher_is_better"] is True and j["dtype"] == "bf16"
    for k in ("roofline", "cpu_baseline", "from_uint8", "two_streams", "one_stream", "mask_paste", "nms_prefix", "host_enqueue_ms_single_step"):
        assert j[k] is None, k
    assert sorted(os.listdir(tmp_path)) == ["count.npy", "dets.npy"]
    d, c = np.load(tmp_path / "dets.npy"), np.load(tmp_path / "count.npy")
    assert d.dtype == np.float32 and c.dtype == np.float64 and d.shape[0] == 2 and c.shape == (2,)

    import torch

    from minddet.models import Config, build_detector
    from minddet_amd import nn_ops
    from minddet_amd.data import synthetic_images

    cfg = Config.fromfile(cfg_path)
    model = build_detector(cfg.model, cfg.train_cfg, cfg.test_cfg).to("cuda:0")
    H, W = cfg.data.input_hw
    x = synthetic_images(2, H, W, seed=20240317, device="cuda:0")
    if nn_ops.stem_layout_ok(H, W) and model.backbone.stem is not None:   # the input layout bench.py hands the model
        x = nn_ops.to_stem_layout(x)
    dets, count = model.forward(x)[:2]
    torch.cuda.synchronize()
    assert np.array_equal(d, dets.float().cpu().numpy()) and np.array_equal(c, count.cpu().numpy().astype(np.float64))
