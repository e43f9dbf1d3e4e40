"""JPEG decode + the COCO Captions reader: the part of the reference's dataset item in front of the
image transform -- `cv2.imread` + `cvtColor(BGR2RGB)` (/root/reference/virtex/data/datasets/coco_captions.py:56-63) and the
annotation bookkeeping of `CocoCaptionsDataset.__init__` (:22-52).

`decode_jpeg(data, device)` returns the decoder's uint8 (H, W, 3) RGB pixels ON THE DEVICE -- what
`virtex_amd.data.augment_batch` / `vtx_image_augment_u8` read; the file's bytes are the only thing that crosses PCIe besides
the int16 coefficients.  Host: marker parsing + Huffman decoding (C++, thread-safe, releases the GIL); device: dequantise,
inverse DCT, chroma upsampling, colour conversion -- bit-exact with libjpeg-turbo's defaults (csrc/jpeg.hip; pinned against
Pillow's libjpeg-turbo in tests/test_jpeg.py, CPU restatement in oracle/jpeg.py).  There is no fallback decoder: a stream the
kernels do not take (progressive, CMYK, ...) raises VtxError -- convert such files once, offline.

`entropy="device"` moves the Huffman decoding onto the device as well (csrc/jpeg_entropy.hip: a self-synchronising parallel
decoder, one lane per `subseq_bits` bits of the scan): the host parses markers, the file's scan bytes and a small descriptor
cross PCIe, and no coefficient ever exists in host memory.  The coefficients are the host decoder's, bit for bit.  The default
stays `"host"`."""
import ctypes
import json
import os
import threading
import unicodedata
from collections import defaultdict
from typing import Dict, List, Tuple

import torch

from . import _lib
from ._lib import ptr, stream_ptr


def jpeg_info(data: bytes) -> Dict[str, int]:
    info = (ctypes.c_int * 8)()
    _lib.call("vtx_jpeg_info", data, len(data), info)
    keys = ("width", "height", "components", "luma_h", "luma_v", "orientation", "blocks", "plane_bytes")
    return dict(zip(keys, [int(v) for v in info]))


SUBSEQ_BITS = 512       # default subsequence length of the device entropy decoder (256 / 512 / 1 024 / 2 048 swept)
_STATUS_REASON = {1: "corrupt Huffman code", 2: "corrupt DC code", 3: "corrupt AC run", 4: "coefficient count does not match the frame"}


def _check_entropy(entropy: str):
    if entropy not in ("host", "device"):
        raise ValueError(f"entropy must be 'host' or 'device', not {entropy!r}")


def _describe(data: bytes, subseq_bits: int):
    dinfo = (ctypes.c_int * 8)()
    _lib.call("vtx_jpeg_describe", data, len(data), subseq_bits, dinfo, None, 0, None, 0, None)
    return [int(v) for v in dinfo]


def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


def entropy_decode_device(blobs, device, subseq_bits: int = SUBSEQ_BITS, pool=None, host=None):
    """Huffman-decode a chunk of streams on the device in ONE launch sequence.  Returns (coef, coef_offs, chunk, qt_offs, status,
    work): the int16 coefficients of all images in one device tensor with each image's first element, the chunk buffer on the
    device (descriptors, scan bytes) with the byte offset of every image's quantisation tables, the status pairs (still on the
    device: nothing is read back here) and the scratch whose last four ints are the synchronisation counters.  `host`: a pinned
    uint8 staging tensor to reuse; `pool`: an executor for the per-image marker parsing."""
    device = torch.device(device)
    n = len(blobs)
    run = (lambda f, it: list(pool.map(f, it))) if pool is not None else (lambda f, it: [f(i) for i in it])
    dinfos = run(lambda i: _describe(blobs[i], subseq_bits), range(n))
    n_wg = sum(d[3] for d in dinfos)
    pos = _align(4 * n_wg)                                                # int wg_desc[n_wg], int img_desc[n]
    img_table_off, pos = pos, _align(pos + 4 * n)
    desc_offs, scan_offs, coef_offs, first_wg, wg, co = [], [], [], [], 0, 0
    for d in dinfos:
        desc_offs.append(pos); pos = _align(pos + d[0])
    for d in dinfos:
        scan_offs.append(pos); pos = _align(pos + d[1])
        first_wg.append(wg); wg += d[3]
        coef_offs.append(co); co += d[5] * 64                             # (64 int16 per block: 128-byte slices)
    if host is None or host.numel() < pos:
        host = torch.empty(pos, dtype=torch.uint8, pin_memory=(device.type == "cuda"))
    tables = host[:img_table_off + 4 * n].view(torch.int32)
    tables[:n_wg] = torch.repeat_interleave(torch.tensor(desc_offs, dtype=torch.int32), torch.tensor([d[3] for d in dinfos]))
    tables[img_table_off // 4:] = torch.tensor(desc_offs, dtype=torch.int32)
    base = host.data_ptr()

    def fill(i):
        place = (ctypes.c_long * 4)(scan_offs[i], first_wg[i], coef_offs[i], i)
        _lib.call("vtx_jpeg_describe", blobs[i], len(blobs[i]), subseq_bits, (ctypes.c_int * 8)(), base + desc_offs[i],
                  dinfos[i][0], base + scan_offs[i], dinfos[i][1], place)

    run(fill, range(n))
    chunk = torch.empty(pos, dtype=torch.uint8, device=device)
    chunk.copy_(host[:pos], non_blocking=True)                            # the ONE copy of the chunk: file bytes + descriptors
    coef = torch.empty(max(co, 8), dtype=torch.int16, device=device)
    status = torch.empty(2 * n, dtype=torch.int32, device=device)
    work = torch.empty((4 * dinfos[0][6] + 2) * n_wg + 4, dtype=torch.int32, device=device)
    _lib.call("vtx_jpeg_entropy_decode_device", ptr(chunk), 0, img_table_off, n, n_wg, max(d[3] for d in dinfos), ptr(coef),
              coef.numel(), ptr(status), ptr(work), work.numel(), stream_ptr(coef))
    return coef, coef_offs, chunk, [desc_offs[i] + dinfos[i][7] for i in range(n)], status, work


def _raise_failed(status: torch.Tensor, first_index: int = 0):
    """the chunk's status pairs, read back once: VtxError naming the first failed image"""
    st = status.cpu().view(-1, 2)
    bad = torch.nonzero(st[:, 0]).flatten()
    if bad.numel():
        i = int(bad[0])
        raise _lib.VtxError(f"vtx_jpeg_entropy_decode_device failed ({int(st[i, 0])}): jpeg: image {first_index + i}: "
                            f"{_STATUS_REASON.get(int(st[i, 1]), 'corrupt scan')}")


def _reconstruct_chunk(blobs, infos, coef, coef_offs, chunk, qt_offs, planes, apply_orientation, device):
    out = []
    for i, (data, info) in enumerate(zip(blobs, infos)):
        swap = apply_orientation and info["orientation"] >= 5
        H, W = (info["width"], info["height"]) if swap else (info["height"], info["width"])
        rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
        _lib.call("vtx_jpeg_reconstruct", data, len(data), ptr(coef[coef_offs[i]:]), ptr(chunk[qt_offs[i]:]), ptr(planes),
                  ptr(rgb), 1 if apply_orientation else 0, stream_ptr(rgb))
        out.append(rgb)
    return out


def decode_jpeg(data: bytes, device, apply_orientation: bool = True, entropy: str = "host", subseq_bits: int = SUBSEQ_BITS) -> torch.Tensor:
    """bytes of one baseline JPEG -> uint8 (H, W, 3) RGB on `device` (EXIF orientation applied like cv2.imread).
    entropy: where the Huffman decoding runs, "host" (default) or "device"."""
    _check_entropy(entropy)
    device = torch.device(device)
    if entropy == "device":
        info = jpeg_info(data)
        coef, coef_offs, chunk, qt_offs, status, _ = entropy_decode_device([data], device, subseq_bits)
        planes = torch.empty(info["plane_bytes"], dtype=torch.uint8, device=device)
        rgb = _reconstruct_chunk([data], [info], coef, coef_offs, chunk, qt_offs, planes, apply_orientation, device)[0]
        _raise_failed(status)
        return rgb
    info = jpeg_info(data)
    pin = device.type == "cuda"
    coef = torch.empty(info["blocks"] * 64, dtype=torch.int16, pin_memory=pin)
    qt = torch.empty(4 * 64, dtype=torch.int16, pin_memory=pin)                 # uint16 values: same bits
    _lib.call("vtx_jpeg_entropy_decode", data, len(data), coef.data_ptr(), coef.numel(), qt.data_ptr())
    coef_d, qt_d = coef.to(device, non_blocking=True), qt.to(device, non_blocking=True)
    planes = torch.empty(info["plane_bytes"], dtype=torch.uint8, device=device)
    swap = apply_orientation and info["orientation"] >= 5
    H, W = (info["width"], info["height"]) if swap else (info["height"], info["width"])
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
    _lib.call("vtx_jpeg_reconstruct", data, len(data), ptr(coef_d), ptr(qt_d), ptr(planes), ptr(rgb),
              1 if apply_orientation else 0, stream_ptr(rgb))
    return rgb


_staging = {}        # device -> [pinned int16 buffer, event recorded after the last copy out of it]: ONE staging area per device, grown on demand
_staging_lock = threading.Lock()      # ... used by one decode_jpeg_batch call at a time (calls from several threads take turns)


def _staging_area(device, n16: int):
    """A pinned int16 buffer of at least n16 elements, reused from call to call (allocating page-locked memory costs
    milliseconds).  The previous call's copies out of it must have finished before a new decode writes into it."""
    ent = _staging.get(device)
    if ent is not None and ent[1] is not None:
        ent[1].synchronize()
    if ent is None or ent[0].numel() < n16:
        ent = _staging[device] = [torch.empty(max(n16, 1 << 20), dtype=torch.int16, pin_memory=(device.type == "cuda")), None]
    return ent


def decode_jpeg_batch(blobs, device, threads: int = 8, apply_orientation: bool = True, chunk: int = 16, entropy: str = "host",
                      subseq_bits: int = SUBSEQ_BITS) -> List[torch.Tensor]:
    """Many files at once.  The serial Huffman decoding of the images runs on `threads` host threads (the C entry points hold no
    Python state and ctypes releases the GIL), each writing its int16 coefficients into ITS slice of one page-locked staging
    buffer; the main thread follows in input order: as soon as the next `chunk` images are decoded, their slice crosses PCIe in ONE
    asynchronous copy and the per-image device work (inverse DCT, upsampling, colour conversion: two launches per image, all
    images sharing one plane scratch in stream order) is enqueued on the caller's stream.  Per image the main thread issues one C
    call and one small allocation (round 5 allocated page-locked memory and issued two copies per image: 7 400-9 900 images/s
    whatever the thread count; this form scales with the host threads).  Returns the uint8 (H, W, 3) tensors in input order.
    entropy="device": per chunk the host threads only parse markers; the chunk's scan bytes and descriptors cross PCIe in one
    copy, ONE call Huffman-decodes the chunk on the device, the per-image reconstruct launches read the device coefficients, and
    the chunk's status words are read back once behind them (VtxError names the first failed image)."""
    _check_entropy(entropy)
    device = torch.device(device)
    if len(blobs) == 0:
        return []
    with _staging_lock:
        if entropy == "device":
            return _decode_jpeg_batch_device(blobs, device, threads, apply_orientation, chunk, subseq_bits)
        return _decode_jpeg_batch(blobs, device, threads, apply_orientation, chunk)


def _decode_jpeg_batch_device(blobs, device, threads, apply_orientation, chunk, subseq_bits):
    from concurrent.futures import ThreadPoolExecutor
    n = len(blobs)
    out = []
    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        infos = list(pool.map(jpeg_info, blobs))
        planes = torch.empty(max(i["plane_bytes"] for i in infos), dtype=torch.uint8, device=device)
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            stage = _staging_area(device, 1 << 20)                        # (waits for the previous chunk's copy out of it)
            coef, coef_offs, chunk_d, qt_offs, status, _ = entropy_decode_device(blobs[c0:c1], device, subseq_bits, pool,
                                                                                 stage[0].view(torch.uint8))   # (a chunk it cannot hold stages in a buffer of its own)
            if device.type == "cuda":
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(device))
                stage[1] = ev
            out += _reconstruct_chunk(blobs[c0:c1], infos[c0:c1], coef, coef_offs, chunk_d, qt_offs, planes, apply_orientation, device)
            _raise_failed(status, c0)
    return out


def _decode_jpeg_batch(blobs, device, threads, apply_orientation, chunk):
    from concurrent.futures import ThreadPoolExecutor
    n = len(blobs)
    infos = [jpeg_info(b) for b in blobs]
    QT = 4 * 64
    sizes = [i["blocks"] * 64 + QT for i in infos]                       # coefficients, then the four quantisation tables
    offs = [0]
    for sz in sizes:
        offs.append(offs[-1] + ((sz + 7) // 8) * 8)                       # 16-byte aligned slices
    stage = _staging_area(device, offs[-1])
    host = stage[0]
    base = host.data_ptr()

    def work(i):
        data = blobs[i]
        _lib.call("vtx_jpeg_entropy_decode", data, len(data), base + 2 * offs[i], infos[i]["blocks"] * 64,
                  base + 2 * (offs[i] + infos[i]["blocks"] * 64))
        return i

    dev_all = torch.empty(offs[-1], dtype=torch.int16, device=device)
    planes = torch.empty(max(i["plane_bytes"] for i in infos), dtype=torch.uint8, device=device)   # shared: the images' kernels run in stream order
    out = []
    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        done = pool.map(work, range(n))
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            for _ in range(c0, c1):
                next(done)                                                # (raises here what a worker raised)
            dev_all[offs[c0]:offs[c1]].copy_(host[offs[c0]:offs[c1]], non_blocking=True)
            for i in range(c0, c1):
                info, data = infos[i], blobs[i]
                swap = apply_orientation and info["orientation"] >= 5
                H, W = (info["width"], info["height"]) if swap else (info["height"], info["width"])
                rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
                nb = info["blocks"] * 64
                _lib.call("vtx_jpeg_reconstruct", data, len(data), ptr(dev_all[offs[i]:offs[i] + nb]),
                          ptr(dev_all[offs[i] + nb:offs[i] + nb + QT]), ptr(planes), ptr(rgb), 1 if apply_orientation else 0,
                          stream_ptr(rgb))
                out.append(rgb)
    if device.type == "cuda":
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        stage[1] = ev
    return out


def normalize_caption(caption: str) -> str:
    """The reference's caption normalisation (coco_captions.py:33-38): lowercase, NFKD, combining marks stripped."""
    caption = unicodedata.normalize("NFKD", caption.lower())
    return "".join(ch for ch in caption if not unicodedata.combining(ch))


class CocoCaptionsReader:
    """`CocoCaptionsDataset` of the reference (coco_captions.py:11-63) with the image decoded on the device:
    item = {"image_id": int, "image": uint8 (H, W, 3) RGB tensor on `device`, "captions": [str]} -- same keys, same instance
    order (annotation order of first appearance), same caption normalisation.  `read_bytes(idx)` / `instances` give the raw
    pieces to loaders that decode a whole batch from a thread pool."""

    def __init__(self, data_root: str, split: str, device="cuda", entropy: str = "host"):
        _check_entropy(entropy)
        self.entropy = entropy
        image_dir = os.path.join(data_root, f"{split}2017")
        with open(os.path.join(data_root, "annotations", f"captions_{split}2017.json")) as fh:
            captions = json.load(fh)
        per_image: Dict[int, List[str]] = defaultdict(list)
        for ann in captions["annotations"]:
            per_image[ann["image_id"]].append(normalize_caption(ann["caption"]))
        paths = {im["id"]: os.path.join(image_dir, im["file_name"]) for im in captions["images"]}
        self.instances: List[Tuple[int, str, List[str]]] = [(i, paths[i], per_image[i]) for i in per_image.keys()]
        self.device = torch.device(device)

    def __len__(self) -> int:
        return len(self.instances)

    def read_bytes(self, idx: int) -> bytes:
        with open(self.instances[idx][1], "rb") as fh:
            return fh.read()

    def __getitem__(self, idx: int):
        image_id, _, captions = self.instances[idx]
        return {"image_id": image_id, "image": decode_jpeg(self.read_bytes(idx), self.device, entropy=self.entropy), "captions": captions}
