"""md_pw_chain against the two md_conv2d launches it replaces (bit compare) + timing of both on ResNet stage 2 at the benchmark's shapes.

Usage: python tools/pw_chain_check.py [reps]      (batch 60 = one half of the benchmark step, batch 120 = the one-stream pass)
Algorithmic bytes per pixel: chain 2560 (t2 256 + residual 1024 + y 1024 + t1 256), two launches 3584 (y read back once more)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minddet_amd import graphs, nn_ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))[reps // 2]


def main(reps=20):
    st = graphs.ResNet(depth=50).to(DEV).stages[1]
    pc3, pc1 = st[1].conv3.packed, st[2].conv1.packed
    pk = nn_ops.pack_pw_chain(pc3, pc1)
    for n in (60, 120):
        g = torch.Generator().manual_seed(n)
        t2 = torch.randn((n, 100, 168, 128), generator=g).to(torch.bfloat16).to(DEV)
        res = torch.randn((n, 100, 168, 512), generator=g).to(torch.bfloat16).to(DEV)
        y_ref = nn_ops.conv2d(t2, pc3, residual=res)
        t1_ref = nn_ops.conv2d(y_ref, pc1)
        y, t1 = nn_ops.pw_chain(t2, res, pk)
        same = torch.equal(y, y_ref) and torch.equal(t1, t1_ref)
        del y, t1, t1_ref
        px = n * 100 * 168
        ms_c3 = timed(lambda: nn_ops.conv2d(t2, pc3, residual=res), reps)
        ms_c1 = timed(lambda: nn_ops.conv2d(y_ref, pc1), reps)
        ms_ch = timed(lambda: nn_ops.pw_chain(t2, res, pk), reps)
        print(f"b{n} 100x168: bit-identical {same} | conv3 + residual {ms_c3 * 1e3:7.1f} us ({px * 2304 / ms_c3 / 1e9:5.2f} TB/s)  conv1 {ms_c1 * 1e3:7.1f} us "
              f"({px * 1280 / ms_c1 / 1e9:5.2f} TB/s)  sum {1e3 * (ms_c3 + ms_c1):7.1f} us | md_pw_chain {ms_ch * 1e3:7.1f} us ({px * 2560 / ms_ch / 1e9:5.2f} TB/s)",
              flush=True)
        if not same:
            sys.exit(1)
        del t2, res, y_ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
