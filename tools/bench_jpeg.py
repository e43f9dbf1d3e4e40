"""JPEG decode throughput on the box: COCO-sized images (640 x 480, 4:2:0, quality 90) encoded with Pillow, decoded by
virtex_amd.jpeg.decode_jpeg_batch with 1 / 8 / 16 host threads, against Pillow's own decoder on one thread.
    python tools/bench_jpeg.py [--images 256] [--entropy host|device|both] [--subseq-bits 1024] [--repeats 3]
--entropy both alternates the host and the device Huffman decoder in the same process (same images, same warm-up); every
window is closed by a device synchronise; the best and the median of the repeats are printed."""
import argparse
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from virtex_amd import jpeg as vj  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--entropy", choices=("host", "device", "both"), default="host")
    ap.add_argument("--subseq-bits", type=int, default=vj.SUBSEQ_BITS)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16)
    a = ap.parse_args()
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:480, 0:640]
    blobs = []
    for i in range(16):
        img = np.stack([127 + 90 * np.sin(xx / (9.0 + i) + c) * np.cos(yy / (6.0 + c) - i) for c in range(3)], -1) + rng.normal(0, 10, (480, 640, 3))
        buf = io.BytesIO(); Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    blobs = [blobs[i % 16] for i in range(a.images)]
    dev = torch.device("cuda", 0)
    info0 = vj.jpeg_info(blobs[0])
    ref = np.asarray(Image.open(io.BytesIO(blobs[0])).convert("RGB"))
    got = vj.decode_jpeg(blobs[0], dev).cpu().numpy()
    print(f"{a.images} images of 640x480 4:2:0 q90, {sum(map(len, blobs)) / a.images / 1e3:.0f} KB each; bit-exact with Pillow: {np.array_equal(ref, got)}; "
          f"host CPUs {os.cpu_count()}")
    paths = ("host", "device") if a.entropy == "both" else (a.entropy,)
    kw = {"host": {}, "device": {"entropy": "device", "subseq_bits": a.subseq_bits}}
    if "device" in paths:
        got = vj.decode_jpeg(blobs[0], dev, entropy="device", subseq_bits=a.subseq_bits).cpu().numpy()
        d = vj._describe(blobs[0], a.subseq_bits)
        print(f"device entropy decoder, {a.subseq_bits}-bit subsequences: bit-exact with Pillow: {np.array_equal(ref, got)}; image 0: "
              f"{d[2]} subsequences in {d[3]} workgroups; PCIe bytes per image: host path {info0['blocks'] * 128 + 512} "
              f"(coefficients + quantisation tables), device path {d[0] + d[1]} (scan bytes + descriptor)")
        work = vj.entropy_decode_device(blobs[:a.chunk], dev, a.subseq_bits)[5]
        c = work[-4:].cpu().tolist()
        tot = max(1, sum(c[:3]))
        print(f"synchronisation, first {a.chunk} images: {100 * c[0] / tot:.1f} % of the subsequences final after one decode, "
              f"{100 * c[1] / tot:.1f} % after two, {100 * c[2] / tot:.1f} % after more; {c[3]} decodes in the passes across workgroups")
    for threads in (1, 8, 16):
        rates = {p: [] for p in paths}
        for p in paths:
            vj.decode_jpeg_batch(blobs[:16], dev, threads=threads, chunk=a.chunk, **kw[p])
        torch.cuda.synchronize()
        for _ in range(max(3, a.repeats)):
            for p in paths:                                   # alternate the paths inside every repeat
                t0 = time.perf_counter()
                out = vj.decode_jpeg_batch(blobs, dev, threads=threads, chunk=a.chunk, **kw[p])
                torch.cuda.synchronize()
                rates[p].append(a.images / (time.perf_counter() - t0))
                del out
        for p in paths:
            r = sorted(rates[p])
            print(f"virtex_amd decode_jpeg_batch, entropy={p:6s} {threads:2d} host threads: best {r[-1]:8.0f}  median {r[len(r) // 2]:8.0f} images/s  ({len(r)} repeats)")
    t0 = time.perf_counter()
    for b in blobs[:64]:
        np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    print(f"Pillow (libjpeg-turbo), one thread, host memory:      {64 / (time.perf_counter() - t0):8.0f} images/s")
    # device part alone: coefficients already on the device
    info = vj.jpeg_info(blobs[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    outs = vj.decode_jpeg_batch(blobs[:32], dev, threads=8)
    torch.cuda.synchronize()
    print(f"(device kernels: idct over {info['blocks']} blocks + colour conversion per image; see rocprofv3 for their time)")


if __name__ == "__main__":
    main()
