"""The grouped 3x3 convolutions of resnext50_32x4d (conv2 of every Bottleneck) at 256 images of 224 x 224: forward, input
gradient and weight gradient through csrc/gconv3x3.hip against stock torch.nn.functional.conv2d(groups=32) in bf16
channels_last (the reference's path) and against the HBM byte floor (input + output + weights once).

    python tools/bench_gconv.py [--batch 256] [--out profiles/gconv3x3_bench.txt]

Both run in one process, alternating, in device-synchronised windows after warm-up.  Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virtex_amd import _lib, ops  # noqa: E402

GROUPS = 32
SHAPES = [(56, 128, 1), (56, 256, 2), (28, 256, 1), (28, 512, 2), (14, 512, 1), (14, 1024, 2), (7, 1024, 1)]   # (H = W, C, stride)
HBM_BYTES_PER_S = 8.0e12                                                 # MI355X peak


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available() and _lib.backend() == "hip:gfx950", "needs an MI355X"
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    lines = [f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; bf16, batch {a.batch}, groups {GROUPS}; {a.repeats} alternating "
             f"windows of {a.iters} calls, host clock around a device synchronise; us per call, median (min); floor = (input + output "
             f"+ weights) bytes / {HBM_BYTES_PER_S / 1e12:.0f} TB/s; 'of floor' = floor / ours",
             f"{'shape':>22} {'op':>6} {'ours':>16} {'torch':>16} {'floor':>7} {'of floor':>8} {'vs torch':>9}"]
    for (H, C, stride) in SHAPES:
        g = torch.Generator().manual_seed(H * C)
        cg, OH = C // GROUPS, (H - 1) // stride + 1
        x = torch.randn(a.batch, H, H, C, generator=g).to(dev, dt)
        dy = torch.randn(a.batch, OH, OH, C, generator=g).to(dev, dt)
        w = (torch.randn(C, 3, 3, cg, generator=g) * (9 * cg) ** -0.5).to(dev, dt)
        dw = torch.zeros(C, 3, 3, cg, device=dev)
        xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)                        # NCHW views of channels_last storage
        wt = w.permute(0, 3, 1, 2)
        conv = lambda: F.conv2d(xt, wt, stride=stride, padding=1, groups=GROUPS)
        legs = {"fwd": (lambda: ops.conv2d_fwd(x, w, stride, 1, groups=GROUPS), conv),
                "dgrad": (lambda: ops.conv2d_dgrad(dy, w, x.shape, stride, 1, groups=GROUPS),
                          lambda: torch.ops.aten.convolution_backward(dyt, xt, wt, None, [stride] * 2, [1, 1], [1, 1], False, [0, 0],
                                                                      GROUPS, [True, False, False])),
                "wgrad": (lambda: ops.conv2d_wgrad(x, dy, dw, stride, 1, groups=GROUPS),
                          lambda: torch.ops.aten.convolution_backward(dyt, xt, wt, None, [stride] * 2, [1, 1], [1, 1], False, [0, 0],
                                                                      GROUPS, [False, True, False]))}
        err = (ops.conv2d_fwd(x, w, stride, 1, groups=GROUPS).float() - conv().permute(0, 2, 3, 1).float()).norm() / conv().float().norm()
        assert err < 1e-2, err                                                         # same results at the timed size
        floor = 2.0 * (x.numel() + dy.numel() + w.numel()) / HBM_BYTES_PER_S * 1e6
        for op, (ours, stock) in legs.items():
            for fn in (ours, stock):
                window(fn, 5)
            t = {"ours": [], "torch": []}
            for _ in range(a.repeats):
                t["ours"].append(window(ours, a.iters))
                t["torch"].append(window(stock, a.iters))
            mo, mt = statistics.median(t["ours"]), statistics.median(t["torch"])
            lines.append(f"{f'{H}x{H}x{C} s{stride} Cg{cg}':>22} {op:>6} {mo:8.1f} ({min(t['ours']):6.1f}) {mt:8.1f} ({min(t['torch']):6.1f}) "
                         f"{floor:7.1f} {floor / mo:8.2f} {mt / mo:8.2f}x" + ("   SLOWER than torch" if mo > mt else ""))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
