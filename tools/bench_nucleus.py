"""One nucleus-sampling selection step, given the logits: the torch operator chain of draw="torch" (sort, softmax, cumsum,
shift, two scatters, masked_fill, softmax, multinomial) against torch.rand + vtx_nucleus_step (draw="device").

    python tools/bench_nucleus.py [--rows 16 256] [--vocab 10000] [--out profiles/nucleus_step.txt]

Both run in one process, alternating, in device-synchronised windows after warm-up.  Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virtex_amd import _lib, ops  # noqa: E402

EOS, P = 2, 0.9


def torch_chain(logits, last):
    """The body of AutoRegressiveNucleusSampling.search's loop (draw="torch") after `step`."""
    logits = logits.clone()                        # the chain filters in place; the clone is timed separately and subtracted
    ordered, order = torch.sort(logits, descending=True)
    mass = torch.cumsum(torch.softmax(ordered, dim=-1), dim=-1)
    outside = mass > P
    outside = torch.cat([torch.zeros_like(outside[:, :1]), outside[:, :-1]], dim=1)
    drop = torch.zeros_like(outside).scatter_(1, order, outside)
    drop.scatter_(1, last.unsqueeze(1), True)
    logits.masked_fill_(drop, -1e12)
    nxt = torch.multinomial(torch.softmax(logits, dim=-1), 1).view(-1)
    return torch.where(last == EOS, torch.full_like(nxt, EOS), nxt)


def device_step(logits, last):
    u = torch.rand(logits.size(0), device=logits.device, dtype=torch.float32)
    return ops.nucleus_step(logits, last, u, EOS, P)[0]


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available() and _lib.backend() == "hip:gfx950", "needs an MI355X"
    dev = torch.device("cuda:0")
    lines = [f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; one selection step at V = {a.vocab}, p = {P}; "
             f"{a.repeats} alternating windows of {a.iters} steps, host clock around a device synchronise; us per step, median (min)"]
    for rows in a.rows:
        g = torch.Generator().manual_seed(rows)
        logits = (3.0 * torch.randn(rows, a.vocab, generator=g)).to(dev)
        last = torch.randint(0, a.vocab, (rows,), generator=g).to(dev)
        legs = {"clone only": lambda: logits.clone(), "torch chain + clone": lambda: torch_chain(logits, last),
                "torch.rand + vtx_nucleus_step": lambda: device_step(logits, last)}
        for fn in legs.values():
            window(fn, 50)
        t = {k: [] for k in legs}
        for _ in range(a.repeats):
            for k, fn in legs.items():
                t[k].append(window(fn, a.iters))
        u = torch.rand(rows, device=dev)
        ops.profile_start()                        # the kernel alone: the dispatch's own timestamps, 100 launches
        for _ in range(100):
            kept = ops.nucleus_step(logits, last, u, EOS, P)[1]
        torch.cuda.synchronize()
        rec = [r for r in ops.profile_stop() if "nucleus_step" in r["name"]]
        kernel_us = sum(r["seconds"] for r in rec) / sum(r["launches"] for r in rec) * 1e6
        lines.append(f"rows {rows:4d} (nucleus {int(kept.min())}..{int(kept.max())} tokens): " + "; ".join(
            f"{k} {statistics.median(v):8.1f} ({min(v):8.1f})" for k, v in t.items()) + f"; nucleus_step_kernel alone {kernel_us:.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
