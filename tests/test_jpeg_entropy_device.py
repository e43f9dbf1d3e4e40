"""Huffman decoding of JPEG scans on the device (csrc/jpeg_entropy.hip, `entropy="device"` of virtex_amd/jpeg.py): its int16
coefficients against the host decoder's (vtx_jpeg_entropy_decode) and its pixels against the committed fixture / Pillow --
every comparison exact."""
import ctypes

import numpy as np
import pytest
import torch

from backends import BACKENDS, select
from test_jpeg import GOLDEN, _encode, _image, _pil_decode


def _fixture():
    z = np.load(GOLDEN)
    return [z[f"jpeg_{i}"].tobytes() for i in range(int(z["count"]))], [z[f"rgb_{i}"] for i in range(int(z["count"]))]


def _host_coefficients(vj, data):
    from virtex_amd import _lib
    coef, qt = torch.empty(vj.jpeg_info(data)["blocks"] * 64, dtype=torch.int16), torch.empty(256, dtype=torch.int16)
    _lib.call("vtx_jpeg_entropy_decode", ctypes.c_char_p(data), ctypes.c_long(len(data)), ctypes.c_void_p(coef.data_ptr()),
              ctypes.c_long(coef.numel()), ctypes.c_void_p(qt.data_ptr()))
    return coef.numpy()


def _device_coefficients(vj, data, dev, bits):
    coef, _, _, _, status, _ = vj.entropy_decode_device([data], dev, bits)
    assert not status.cpu().any()
    return coef[:vj.jpeg_info(data)["blocks"] * 64].cpu().numpy()


@pytest.mark.parametrize("bits", [128, None])
@pytest.mark.parametrize("backend", BACKENDS)
def test_device_coefficients_and_pixels_equal_the_host_decoders(backend, bits):
    from virtex_amd import jpeg as vj
    dev = select(backend)
    bits = bits or vj.SUBSEQ_BITS
    blobs, rgbs = _fixture()
    assert len(blobs) == 13
    spans = [vj._describe(b, 128)[2] for b in blobs]
    assert max(spans) >= 24 and min(spans) == 1           # dozens of subsequences down to less than one (the 1 x 1 frame)
    for i, data in enumerate(blobs):
        assert np.array_equal(_device_coefficients(vj, data, dev, bits), _host_coefficients(vj, data)), i
        assert np.array_equal(vj.decode_jpeg(data, dev, entropy="device", subseq_bits=bits).cpu().numpy(), rgbs[i]), i


@pytest.mark.parametrize("backend", BACKENDS)
def test_one_batch_of_mixed_streams_equals_the_single_decodes(backend):
    from virtex_amd import jpeg as vj
    dev = select(backend)
    blobs, rgbs = _fixture()
    with pytest.raises(ValueError):
        vj.decode_jpeg_batch(blobs, dev, entropy="gpu")
    outs = vj.decode_jpeg_batch(blobs, dev, threads=3, chunk=5, entropy="device", subseq_bits=128)    # 13 = 5 + 5 + 3
    assert len(outs) == len(blobs)
    for i, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), rgbs[i]), i


@pytest.mark.parametrize("restart", [0, 3])
@pytest.mark.parametrize("backend", BACKENDS)
def test_scan_across_workgroups_with_stuffed_bytes(backend, restart):
    """96 x 128 noise at quality 95, 4:2:0: more than a byte per pixel.  A workgroup has 256 lanes of 128 bits = 4 096 bytes of
    scan, so a scan of more than 2 * 4 096 bytes reaches a third workgroup; restart intervals of 3 MCU rows (24 MCUs, about
    3 KB) make segments begin and end in the middle of workgroups."""
    pytest.importorskip("PIL")
    from virtex_amd import jpeg as vj
    dev = select(backend)
    data = _encode(_image(96, 128, np.random.default_rng(11), smooth=False), quality=95, subsampling=2, restart_marker_rows=restart)
    dinfo = vj._describe(data, 128)
    assert dinfo[1] > 2 * 4096 and dinfo[3] >= 3 and dinfo[6] == 256 and dinfo[4] == (1 if restart == 0 else 2)
    scan = data[data.index(b"\xff\xda"):]
    assert scan.count(b"\xff\x00") > 0
    assert np.array_equal(_device_coefficients(vj, data, dev, 128), _host_coefficients(vj, data))
    assert np.array_equal(vj.decode_jpeg(data, dev, entropy="device", subseq_bits=128).cpu().numpy(), _pil_decode(data))


@pytest.mark.parametrize("backend", BACKENDS)
def test_truncated_scan_is_refused_and_the_next_decode_succeeds(backend):
    from virtex_amd import _lib, jpeg as vj
    dev = select(backend)
    blobs, rgbs = _fixture()
    good = blobs[0]
    sos = good.index(b"\xff\xda")
    scan0 = sos + 2 + int.from_bytes(good[sos + 2:sos + 4], "big")
    cut = good[:scan0 + (len(good) - 2 - scan0) // 3] + b"\xff\xd9"
    with pytest.raises(_lib.VtxError, match="image 0"):
        vj.decode_jpeg(cut, dev, entropy="device", subseq_bits=128)
    with pytest.raises(_lib.VtxError, match="image 1"):
        vj.decode_jpeg_batch([good, cut, good], dev, entropy="device")
    assert np.array_equal(vj.decode_jpeg(good, dev, entropy="device").cpu().numpy(), rgbs[0])
