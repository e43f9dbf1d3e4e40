"""bf16 cross-attention beyond the tuned tile, forward and backward, per key count S: this build against a baseline build of
the library (the parent commit's, where the same shapes run on the general LDS kernels or are refused).

    python tools/bench_attention_stream.py --baseline path/to/libvirtex_amd_parent.so [--out profiles/attention_stream.txt]

Both libraries are loaded into one process and timed in alternating, device-synchronised windows after warm-up; where both
serve a shape their results on the same inputs are compared.  Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virtex_amd import _lib, ops  # noqa: E402


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", required=True, help="the library to compare with (built from the parent commit)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--queries", type=int, default=30)
    ap.add_argument("--keys", type=int, nargs="+", default=[64, 100, 144, 196, 256])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    libs = {"baseline": a.baseline, "this build": _lib.DEFAULT_LIB}
    _lib.use_library(_lib.DEFAULT_LIB)
    assert torch.cuda.is_available() and _lib.backend() == "hip:gfx950", "needs an MI355X"
    dev = torch.device("cuda:0")
    B, A, T, Hd = a.batch, a.heads, a.queries, a.heads * 64
    lines = [f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; bf16 cross-attention, B = {B}, {A} heads, T = {T}; {a.repeats} "
             f"alternating windows of {a.iters} calls, host clock around a device synchronise; us per call, median (min); "
             "difference = relative L2 of this build's results against the baseline's on the same inputs"]
    for S in a.keys:
        g = torch.Generator().manual_seed(S)
        q = torch.randn(B * T, Hd, generator=g).to(torch.bfloat16).to(dev)
        kv = torch.randn(B * S, 2 * Hd, generator=g).to(torch.bfloat16).to(dev)
        dout = torch.randn(B * T, Hd, generator=g).to(torch.bfloat16).to(dev)
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        legs = {"forward": lambda: ops.attention_fwd(q, kv[:, :Hd], kv[:, Hd:], B, A, T, S, False, None),
                "backward": lambda: ops.attention_bwd(q, kv[:, :Hd], kv[:, Hd:], dout, dq, dkv[:, :Hd], dkv[:, Hd:], B, A, T, S, False, None)}
        for leg, fn in legs.items():
            served, results = {}, {}
            for name, path in libs.items():
                _lib.use_library(path)
                try:
                    out = fn()
                    results[name] = (out if leg == "forward" else torch.cat([dq.flatten(), dkv.flatten()])).clone()
                    window(fn, 5)
                    served[name] = []
                except _lib.VtxError as e:
                    served[name] = "refused (" + str(e).split(": ", 1)[-1].split(" (limit")[0] + ")"
            for _ in range(a.repeats):
                for name, path in libs.items():
                    if isinstance(served[name], list):
                        _lib.use_library(path)
                        served[name].append(window(fn, a.iters))
            cells = [f"{n} " + (f"{statistics.median(t):8.1f} ({min(t):8.1f})" if isinstance(t, list) else t) for n, t in served.items()]
            if len(results) == 2:
                cells.append(f"difference {rel(results['this build'], results['baseline']):.1e}")
            lines.append(f"S {S:4d} {leg:8s}: " + "; ".join(cells))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
