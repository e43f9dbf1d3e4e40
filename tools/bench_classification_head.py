"""Time the classification head plus its loss, forward and backward (global average pool -> linear -> K-hot cross-entropy), in bf16:
the native path (csrc/classify.hip + the MFMA GEMMs) against the reference's formulation run through stock PyTorch under
autocast(bfloat16) -- nn.Linear on the mean-pooled grid, log_softmax, and the per-instance Python loop with .unique() and a
host-side membership test per label (virtex/models/classification.py:75-96 over LinearTextualHead).

Both run in ONE process on the same GPU, alternating after a warm-up; every repetition is timed with a host clock around work
that ends in a device synchronise (the stock path's cost IS its host syncs, which device events alone would not see).  Reports
the median and the spread (min, quartiles, max) of each and writes profiles/classification_head.json.

    python tools/bench_classification_head.py [--reps 30] [--warmup 5] [--out profiles/classification_head.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from virtex_amd import _lib, models  # noqa: E402
from virtex_amd.modules.textual_heads import LinearTextualHead  # noqa: E402

B, HW_SIDE, C, L = 256, 7, 2048, 30


def make_case(V, ignore, dev):
    g = torch.Generator().manual_seed(V)
    grid = torch.randn(B, HW_SIDE, HW_SIDE, C, generator=g).to(torch.bfloat16).to(dev).requires_grad_()     # NHWC memory
    labels = torch.randint(0, V, (B, L), generator=g)
    labels[:, L // 2:] = 0                                   # padding, as the datasets produce it
    labels[:, 0] = V - 1                                     # no empty set
    head = LinearTextualHead(C, V, compute_dtype=torch.bfloat16).to(dev)
    for p in head.parameters():
        p.grad = torch.zeros_like(p)
    stock = torch.nn.Linear(C, V).to(dev)
    stock.load_state_dict(head.output.state_dict())
    return grid, labels.to(dev), head, stock


def native_step(grid, labels, head, ignore):
    logits = head.padded_logits(grid.permute(0, 3, 1, 2))
    loss = models._KHotCrossEntropyFn.apply(logits, labels, ignore, head.vocab_size)
    loss.backward()
    return loss


def stock_step(grid, labels, linear, ignore):
    feats = grid.permute(0, 3, 1, 2)                         # logical NCHW, what a backbone hands over
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pooled = feats.reshape(B, C, -1).permute(0, 2, 1).mean(dim=1)
        logprobs = F.log_softmax(linear(pooled), dim=1)
        loss = torch.zeros((), device=grid.device)
        for b in range(B):
            keep = [v for v in labels[b].unique() if v not in ignore]        # one host sync per label
            loss = loss - logprobs[b, keep].mean()
        loss = loss / B
    loss.backward()
    return loss


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    loss = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, loss.item()


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "q1_ms": q[0], "q3_ms": q[2], "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classification_head.json"))
    a = ap.parse_args()
    assert a.reps >= 20, "the comparison wants at least 20 repetitions each"
    if not torch.cuda.is_available():
        sys.exit("bench_classification_head: needs an MI355X (a CPU run says nothing about speed)")
    assert _lib.backend() == "hip:gfx950", _lib.backend()
    dev = torch.device("cuda:0")
    result = {"backend": _lib.backend(), "device": torch.cuda.get_device_name(0), "shape": {"B": B, "hw": HW_SIDE, "C": C, "L": L},
              "dtype": "bfloat16", "timing": "host clock around forward + backward, device synchronised before and after", "cases": []}
    for V, ignore in ((10000, (0, 1, 2, 3)), (81, (0,))):
        grid, labels, head, stock = make_case(V, ignore, dev)
        runs = {"native": lambda: native_step(grid, labels, head, ignore),
                "stock_autocast": lambda: stock_step(grid, labels, stock, list(ignore))}
        ms = {k: [] for k in runs}
        losses = {}
        for i in range(a.warmup + a.reps):
            for name, fn in runs.items():                   # alternating
                t, losses[name] = timed(fn, dev)
                if i >= a.warmup:
                    ms[name].append(t)
        case = {"V": V, "ignore": list(ignore), "loss": losses, **{k: spread(v) for k, v in ms.items()}}
        case["speedup_median"] = case["stock_autocast"]["median_ms"] / case["native"]["median_ms"]
        # not slower beyond the measured spread: the native median against the stock path's fastest quartile
        case["native_not_slower"] = case["native"]["median_ms"] <= case["stock_autocast"]["q1_ms"]
        result["cases"].append(case)
        print(json.dumps(case))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not all(c["native_not_slower"] for c in result["cases"]):
        sys.exit("bench_classification_head: the native path is slower than the stock formulation")


if __name__ == "__main__":
    main()
