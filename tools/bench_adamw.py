"""The optimizer tail on the 202 tensors of the default bicaptioning model (R_50_L1_H1024, 69.48 M parameters): the fused AdamW
step, torch.optim.AdamW(foreach) through PretrainOptimizer, and the fused SGD step as the reference point.

    python tools/bench_adamw.py [--out profiles/adamw_step.txt]

All three run in one process, alternating, in device-synchronised windows after warm-up; gradients are fixed random values (the
arithmetic does not depend on them, the clip is active).  Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import virtex_amd.factories as vf  # noqa: E402
from virtex_amd import _lib, distributed as vd, ops  # noqa: E402
from virtex_amd.optim import FusedPretrainOptimizer, PretrainOptimizer  # noqa: E402

PEAK_HBM_TBS = 8.0                   # MI355X HBM3E, the figure bench.py's roofline uses


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available() and _lib.backend() == "hip:gfx950", "needs an MI355X"
    dev = torch.device("cuda:0")
    legs, fused = {}, {}
    for name, kind in (("fused adamw", "adamw"), ("fused sgd", "sgd"), ("torch foreach adamw", "adamw")):
        torch.manual_seed(0)
        model = vf.build_bicaptioning_model().to(dev).train()
        g = torch.Generator(device=dev).manual_seed(1)
        if name.startswith("fused"):
            buckets = vd.GradientBuckets(model)
            opt = fused[name] = FusedPretrainOptimizer(model, buckets, start_step=100, optimizer=kind)
            buckets.flat.copy_(torch.randn(buckets.flat.shape, generator=g, device=dev))
        else:
            opt = PretrainOptimizer(model, start_step=100, optimizer=kind)
            for p in model.parameters():
                p.grad = torch.randn(p.shape, generator=g, device=dev)
        legs[name] = opt.step
    n = fused["fused adamw"].n_elems
    for fn in legs.values():
        window(fn, 10)
    t = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, fn in legs.items():
            t[k].append(window(fn, a.iters))
    lines = [f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; optimizer.step() over {n} parameters in "
             f"{len(fused['fused adamw'].buckets.params)} tensors; {a.repeats} alternating windows of {a.iters} steps, host clock "
             f"around a device synchronise; ms per step, median (min)"]
    lines += [f"  {k:22s} {statistics.median(v):7.3f} ({min(v):7.3f})" for k, v in t.items()]
    ops.profile_start()                  # the update kernels alone: the dispatch's own timestamps, algorithmic bytes of the launcher
    for _ in range(50):
        legs["fused adamw"]()
    torch.cuda.synchronize()
    adamw = [r for r in ops.profile_stop() if "adamw_lookahead_kernel" in r["name"]]
    ops.profile_start()
    for _ in range(50):
        legs["fused sgd"]()
    torch.cuda.synchronize()
    sgd = [r for r in ops.profile_stop() if "sgd_lookahead_kernel" in r["name"]]
    for label, rec in (("adamw_lookahead_kernel", adamw), ("sgd_lookahead_kernel", sgd)):
        sec, by, launches = (sum(r[k] for r in rec) for k in ("seconds", "bytes", "launches"))
        lines.append(f"  {label} alone (k = 5: every fifth launch synchronises the slow weights): {sec / launches * 1e3:.3f} ms, "
                     f"{by / launches / 1e9:.3f} GB algorithmic per launch, {by / sec / 1e12:.2f} TB/s = "
                     f"{by / sec / 1e12 / PEAK_HBM_TBS:.2f} of the {PEAK_HBM_TBS:.0f} TB/s HBM peak")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
