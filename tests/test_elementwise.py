"""The contraction kernels held to a float64 reference ELEMENT BY ELEMENT at tile and K edges (tests/elementwise.py), where the
relative L2 norm of the whole tensor (backends.rel_err < 1e-2) cannot see a wrong corner, a dropped K tail or a scaled last
column; plus guard bands around every strided output, and the tiles only the picker reaches.

Shapes: vtx_gemm_nt refuses N % 4 != 0 and vtx_gemm_tn_acc (bf16) M % 8 / N % 8 != 0 (test_entry_points_refuse_ragged_columns),
so 'one column short of a tile' is one 4-element store short of it here: N = 252 (gemm_nt), M, N = 120, 248 (gemm_tn_acc)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import elementwise as ew
from backends import BACKENDS, rel_err, select
from elementwise import assert_elementwise
from test_kernels import _bn_bwd_reference, _generation, _pack_mask_bits, _set_dma_late

from virtex_amd import _lib, ops

BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 12345.0
GM, GN = 257, 252                       # one row past a 256 / 128 / 64 tile, one 4-wide store short of one
K32, K64 = (40, 200), (72, 200, 448)    # ragged tail, odd and even K-tile counts, a single K tile -- per K-step depth
TN_SHAPE = (513, 120, 248)              # (K, M, N) of the weight-gradient products
FLAVOURS = {"plain": dict(),
            "gelu": dict(alpha=0.5, bias=True, act=ew.ACT_GELU, residual=True, want_preact=True),
            "relu": dict(bias=True, act=ew.ACT_RELU),
            "f32": dict(bias=True, out_f32=True)}
CONV_CASES = [(3, 9, 11, 32, 64, 3, 3, 1, 1), (3, 10, 12, 64, 32, 3, 3, 2, 1), (3, 9, 11, 64, 64, 3, 3, 2, 1),
              (3, 8, 10, 128, 64, 1, 1, 2, 0), (2, 22, 26, 8, 64, 7, 7, 2, 3), (2, 5, 7, 64, 64, 2, 3, 1, 1)]


def _cdiv(a, b):
    return (a + b - 1) // b


def _tile_params(cands):
    """backend x tile override; the generation-3 tiles (20, 21) also with the emulator's late LDS-DMA (GEN3_PARAMS of test_kernels)."""
    out = []
    for c in cands:
        for late in ((0, 1) if c >= 20 else (0,)):
            out.append(pytest.param("emu", late, c, marks=pytest.mark.emu, id=f"emu-late{late}-tile{c}"))
        out.append(pytest.param("gpu", 0, c, marks=pytest.mark.gpu, id=f"gpu-tile{c}"))
    return out


class _tile:
    """with _tile(backend, cand, late): the override (and the emulator's DMA timing) for the block, put back afterwards."""

    def __init__(self, backend, cand, late=0):
        self.backend, self.cand, self.late = backend, cand, late

    def __enter__(self):
        _set_dma_late(self.backend, self.late)
        _lib.lib().vtx_set_tile_override(ctypes.c_int(self.cand))

    def __exit__(self, *exc):
        _lib.lib().vtx_set_tile_override(ctypes.c_int(-1))
        _set_dma_late(self.backend, 0)


# ------------------------------------------------------------------------------------------ operands and references (shared)
@functools.lru_cache(maxsize=None)
def _gemm_operands(M, N, K):
    g = torch.Generator().manual_seed(1000 * M + N + K)
    return dict(a=torch.randn(M, K, generator=g).to(BF), b=torch.randn(N, K, generator=g).to(BF),
                bias=torch.randn(N, generator=g), res=torch.randn(M, N, generator=g).to(BF))


def _flavour_args(t, fl):
    f = FLAVOURS[fl]
    return dict(bias=t["bias"] if f.get("bias") else None, residual=t["res"] if f.get("residual") else None,
                act=f.get("act", ew.ACT_NONE), alpha=f.get("alpha", 1.0), out_dtype=F32 if f.get("out_f32") else BF)


@functools.lru_cache(maxsize=None)
def _gemm_model(M, N, K, fl):
    t = _gemm_operands(M, N, K)
    return ew.gemm_nt_model(t["a"], t["b"], **_flavour_args(t, fl))


@functools.lru_cache(maxsize=None)
def _tn_operands(K, M, N):
    g = torch.Generator().manual_seed(K + 7 * M + N)
    t = dict(a=torch.randn(K, M, generator=g).to(BF), b=torch.randn(K, N, generator=g).to(BF), c0=torch.randn(M, N, generator=g))
    t["ref"], t["bound"] = ew.gemm_tn_acc_model(t["a"], t["b"], t["c0"], 2.0)
    return t


@functools.lru_cache(maxsize=None)
def _conv_operands(case):
    N, H, W, C, KO, R, S, stride, pad = case
    g = torch.Generator().manual_seed(sum(case))
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    t = dict(x=torch.randn(N, H, W, C, generator=g).to(BF), w=(torch.randn(KO, R, S, C, generator=g) / (R * S * C) ** 0.5).to(BF),
             dy=torch.randn(N, OH, OW, KO, generator=g).to(BF), dw0=torch.randn(KO, R, S, C, generator=g))
    t["wt"] = t["w"].permute(3, 1, 2, 0).contiguous()
    t["fwd"] = ew.conv_fwd_model(t["x"], t["w"], stride, pad, BF)
    t["dgrad"] = ew.conv_dgrad_model(t["dy"], t["w"], t["x"].shape, stride, pad, BF)
    t["wgrad"] = ew.conv_wgrad_model(t["x"], t["dy"], t["dw0"], stride, pad)
    return t


def _guarded(rows, cols, dtype, dev, fill=None, row_pad=8, ld_extra=24, col_off=8):
    """(buffer, view): a rows x cols column slice of a wider sentinel buffer (row stride cols + ld_extra, first column col_off:
    16-byte aligned in bf16 and fp32), with row_pad sentinel rows above and below."""
    buf = torch.full((rows + 2 * row_pad, cols + ld_extra), SENTINEL, dtype=dtype, device=dev)
    view = buf[row_pad:row_pad + rows, col_off:col_off + cols]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _assert_guard_intact(buf, view_rows, view_cols, what, row_pad=8, col_off=8):
    chk = buf.clone()
    chk[row_pad:row_pad + view_rows, col_off:col_off + view_cols] = SENTINEL
    bad = (chk != SENTINEL).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements outside the output were written, first at buffer index {bad[0].tolist()}"


def _slice_of_wider(t, dev, extra=8, col_off=8):
    """t as a column slice of a buffer whose rows are `extra` elements longer (the rest: a finite junk value a kernel must not use)."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), 3.0, dtype=t.dtype, device=dev)
    view = buf[:, col_off:col_off + t.shape[1]] if extra >= col_off else buf[:, :t.shape[1]]
    view.copy_(t)
    return view


def _run_gemm_flavour(dev, M, N, K, fl, gen, strided=False):
    t, f, m = _gemm_operands(M, N, K), FLAVOURS[fl], _gemm_model(M, N, K, fl)
    odt = F32 if f.get("out_f32") else BF
    a, b = t["a"].to(dev), t["b"].to(dev)
    res = t["res"].to(dev) if f.get("residual") else None
    kw = dict(bias=t["bias"].to(dev) if f.get("bias") else None, act=f.get("act", ops.ACT_NONE), alpha=f.get("alpha", 1.0),
              want_preact=f.get("want_preact", False), out_f32=f.get("out_f32", False))
    buf = None
    if strided:
        a, b = _slice_of_wider(a, dev), _slice_of_wider(b, dev)                 # row stride K + 8, first column 8
        if res is not None:
            res = _slice_of_wider(res, dev, extra=24)                           # row stride N + 24
        buf, kw["out"] = _guarded(M, N, odt, dev)
        assert a.stride(0) == K + 8 and kw["out"].stride(0) == N + 24 and kw["out"].data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0
    got = ops.gemm_nt(a, b, residual=res, **kw)
    assert _generation() == gen, (fl, K, _generation())
    what = f"gemm_nt {M}x{N}x{K} {fl}{' strided' if strided else ''}"
    if kw["want_preact"]:
        got, pre = got
        assert_elementwise(pre, m["pre_ref"], m["pre_bound"], what + " (pre-activation)")
    assert_elementwise(got, m["ref"], m["bound"], what)
    if strided:
        assert got.data_ptr() == kw["out"].data_ptr()
        _assert_guard_intact(buf.cpu(), M, N, what)


# ---------------------------------------------------------------------------------------------- the comparator itself (CPU)
def test_comparator_reports_count_worst_element_and_bounding_box():
    ref = torch.zeros(6, 8, dtype=torch.float64)
    bound = torch.full_like(ref, 0.5)
    got = ref.clone().float()
    assert_elementwise(got, ref, bound, "clean")
    got[5, 2], got[5, 7], got[4, 7] = 1.0, -3.0, float("nan")
    with pytest.raises(AssertionError) as e:
        assert_elementwise(got, ref, bound, "planted")
    msg = str(e.value)
    assert "3 of 48 elements" in msg and "m 4..5, n 2..7" in msg and "(m=4, n=7)" in msg, msg          # the NaN is the worst
    got[4, 7] = 0.0
    with pytest.raises(AssertionError, match=r"2 of 48 elements.*\(m=5, n=7\): got -3, ref 0, \|diff\| 3 > bound 0.5; violations span m 5..5, n 2..7"):
        assert_elementwise(got, ref, bound, "planted")
    with pytest.raises(AssertionError, match=r"n 1..1, h 0..0, w 2..2, c 3..3"):
        g4 = torch.zeros(2, 1, 3, 4); g4[1, 0, 2, 3] = 1
        assert_elementwise(g4, torch.zeros(2, 1, 3, 4, dtype=torch.float64), torch.full((2, 1, 3, 4), 0.5, dtype=torch.float64), "nhwc")


@pytest.mark.parametrize("fl", sorted(FLAVOURS))
@pytest.mark.parametrize("K", sorted(set(K32 + K64)))
def test_bound_admits_plain_fp32_gemm(K, fl):
    """The bound is not too tight: torch's own fp32 evaluation on the same rounded operands, rounded once, has no violation."""
    t, m = _gemm_operands(GM, GN, K), _gemm_model(GM, GN, K, fl)
    out, pre = ew.gemm_nt_fp32(t["a"], t["b"], **_flavour_args(t, fl))
    assert_elementwise(out, m["ref"], m["bound"], f"torch fp32 {fl} K={K}")
    assert_elementwise(pre, m["pre_ref"], m["pre_bound"], f"torch fp32 {fl} K={K} (pre-activation)")


def test_bound_admits_plain_fp32_weight_gradient_products():
    for shape in (TN_SHAPE, (1000, 64, 224), (1000, 40, 248)):
        t = _tn_operands(*shape)
        assert_elementwise(t["c0"] + 2.0 * (t["a"].float().t() @ t["b"].float()), t["ref"], t["bound"], f"torch fp32 tn {shape}")


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bound_admits_plain_fp32_convolutions(case):
    N, H, W, C, KO, R, S, stride, pad = case
    t = _conv_operands(case)
    xr = t["x"].float().permute(0, 3, 1, 2).requires_grad_()
    wr = t["w"].float().permute(0, 3, 1, 2).requires_grad_()
    y = F.conv2d(xr, wr, stride=stride, padding=pad)
    y.backward(t["dy"].float().permute(0, 3, 1, 2))
    assert_elementwise(y.detach().permute(0, 2, 3, 1).to(BF), *t["fwd"], "torch fp32 conv fwd")
    assert_elementwise(xr.grad.permute(0, 2, 3, 1).to(BF), *t["dgrad"], "torch fp32 conv dgrad")
    assert_elementwise(t["dw0"] + wr.grad.permute(0, 2, 3, 1), *t["wgrad"], "torch fp32 conv wgrad")


def _planted(got, ref, bound, what):
    """The defect fails the element-wise bound while the whole-tensor criterion of the older tests still passes: the gap."""
    with pytest.raises(AssertionError, match="elements outside their bound"):
        assert_elementwise(got, ref, bound, what)
    assert rel_err(got.float(), ref) < 1e-2, what


def test_planted_defects_fail_elementwise_and_pass_the_l2_norm():
    K = 40
    t, m = _gemm_operands(GM, GN, K), _gemm_model(GM, GN, K, "plain")
    clean = ew.gemm_nt_fp32(t["a"], t["b"])[0]
    assert_elementwise(clean, m["ref"], m["bound"], "clean")
    # 1. one element of the last row takes its right neighbour's value (a strip epilogue that is one column off at a tile corner)
    # (of the places an edge guard owns -- the start of the last row, the top of the last column, the last tile's corner --
    #  each defect sits where it moves the value most; a 257 x 252 tensor is small enough that the single LARGEST element
    #  difference of a whole row would show in the L2 norm too)
    got = clean.clone()
    m_, n_ = max([(GM - 1, 0), (0, GN - 2), (GM - 1, GN - 2)], key=lambda p: abs(float(clean[p[0], p[1] + 1]) - float(clean[p])))
    got[m_, n_] = clean[m_, n_ + 1]
    _planted(got, m["ref"], m["bound"], "neighbour's value")
    # 2. one element lacks its largest product of the K tail (k = 32..39: what a 32-deep step leaves over)
    tail = lambda p: t["a"][p[0], 32:].double() * t["b"][p[1], 32:].double()
    m_, n_ = max([(GM - 1, 0), (0, GN - 1), (GM - 1, GN - 1)], key=lambda p: float(tail(p).abs().max()))
    got = clean.clone()
    got[m_, n_] = (m["ref"][m_, n_] - tail((m_, n_))[tail((m_, n_)).abs().argmax()]).float().to(BF)
    _planted(got, m["ref"], m["bound"], "K tail product")
    # 4. the ragged last column scaled by 1.05
    got = clean.clone()
    got[:, -1] = (clean[:, -1].float() * 1.05).to(BF)
    _planted(got, m["ref"], m["bound"], "last column x 1.05")
    # 3. the last border pixel of a convolution output lacks one halo tap (the one that weighs most, over all channels)
    case = CONV_CASES[0]
    c = _conv_operands(case)
    ref, bound = c["fwd"]
    x64, w64 = c["x"].double(), c["w"].double()
    Nb, H, W = case[0], case[1], case[2]
    taps = torch.stack([(w64[:, r, s, :] * x64[Nb - 1, H - 2 + r, W - 2 + s, :]).sum(1) for r in range(2) for s in range(2)])   # valid taps x KO
    tap, ko = divmod(int(taps.abs().argmax()), taps.shape[1])
    got = ref.float().to(BF)
    assert_elementwise(got, ref, bound, "clean conv")
    got[Nb - 1, -1, -1, ko] = (ref[Nb - 1, -1, -1, ko] - taps[tap, ko]).float().to(BF)
    _planted(got, ref, bound, "halo tap")


@pytest.mark.parametrize("backend", BACKENDS)
def test_entry_points_refuse_ragged_columns(backend):
    """Why the shapes above stop one 4-element store short of a tile, not one column: the entry points refuse the rest by rule."""
    dev = select(backend)
    a, b = torch.zeros(16, 32, dtype=BF, device=dev), torch.zeros(255, 32, dtype=BF, device=dev)
    with pytest.raises(_lib.VtxError, match="multiples of"):
        ops.gemm_nt(a, b)
    at, bt = torch.zeros(64, 129, dtype=BF, device=dev), torch.zeros(64, 255, dtype=BF, device=dev)
    with pytest.raises(_lib.VtxError, match="multiples of"):
        ops.gemm_tn_acc(at, bt, torch.zeros(129, 255, device=dev))


# --------------------------------------------------------------------------------------------------------- matrix products
@pytest.mark.parametrize("backend,late,cand", _tile_params([0, 1, 2, 3, 4, 5, 6, 11, 12, 20, 21]))
def test_gemm_nt_elementwise_every_tile(backend, late, cand):
    dev = select(backend)
    with _tile(backend, cand, late):
        for K in (K64 if cand >= 10 else K32):
            for fl in FLAVOURS:
                _run_gemm_flavour(dev, GM, GN, K, fl, 3 if cand >= 20 else 2)


@pytest.mark.parametrize("backend,late,cand", _tile_params([1, 12, 20]))
def test_gemm_nt_strided_operands_and_guard_bands(backend, late, cand):
    """a, b, residual and out as column slices of wider buffers (row strides K + 8 / N + 24, first column 8), the output buffer
    pre-filled with a sentinel: the view passes the element-wise bound and not one element outside it changes."""
    dev = select(backend)
    with _tile(backend, cand, late):
        for fl in FLAVOURS:
            _run_gemm_flavour(dev, GM, GN, 72, fl, 3 if cand >= 20 else 2, strided=True)


def _run_tn(dev, shape, split, guarded, gen=None):
    K, M, N = shape
    t = _tn_operands(*shape)
    if guarded:
        buf, out = _guarded(M, N, F32, dev, fill=t["c0"].to(dev))
    else:
        out = t["c0"].clone().to(dev)
    got = ops.gemm_tn_acc(t["a"].to(dev), t["b"].to(dev), out, alpha=2.0, split_k=split)
    if gen is not None:
        assert _generation() == gen, (shape, split, _generation())
    what = f"gemm_tn_acc K, M, N = {shape} split_k {split}{' guarded' if guarded else ''}"
    assert_elementwise(got, t["ref"], t["bound"], what)
    if guarded:
        _assert_guard_intact(buf.cpu(), M, N, what)


@pytest.mark.parametrize("backend,late,cand", _tile_params([0, 1, 2, 3, 4, 5, 6, 20, 21]))
def test_gemm_tn_acc_elementwise_every_tile(backend, late, cand):
    """alpha = 2 into a random gradient, one / chosen / three K slices (K = 513: nine 64-deep K tiles split into exactly three, the
    condition `slices_ok` of launch_auto for generation 3), the output a guarded slice of a sentinel buffer."""
    dev = select(backend)
    with _tile(backend, cand, late):
        for split in (0, 1, 3):
            _run_tn(dev, TN_SHAPE, split, guarded=True, gen=3 if cand >= 20 else 2)
        _run_tn(dev, TN_SHAPE, 3, guarded=False, gen=3 if cand >= 20 else 2)


def _kernel_names(records):
    return [r["name"] for r in records if r["launches"] > 0]


def _is_tile(name, bm, bn):
    return f"BM = {bm}, BN = {bn}," in name


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(1000, 64, 224), (1000, 40, 248)], ids=["64x224", "40x248"])
def test_picker_only_tile_64x256(backend, shape):
    """The 64 x 256 k-major tile (M <= 64, 128 < N <= 256: the stem's weight gradient) is reached through the picker alone: the
    profiler record names the instantiation that ran; with the switch off another one runs, under the same bound."""
    dev = select(backend)
    try:
        for on in (1, 0):
            _lib.call("vtx_set_switch", b"tile64x256", on)
            ops.profile_start()
            try:
                _run_tn(dev, shape, 0, guarded=True, gen=2)
            finally:
                names = _kernel_names(ops.profile_stop())
            assert any(_is_tile(n, 64, 256) for n in names) == bool(on), (on, names)
    finally:
        _lib.call("vtx_set_switch", b"tile64x256", 1)


# ------------------------------------------------------------------------------------------------------------ convolutions
def _conv_generations(case, cand):
    """(forward, input gradient) generation a bf16 case runs on under a tile: the loaders' buf_ok rules (gemm_kernel.h) for the
    32-deep (generation 2) and 64-deep (generation 3, forced by 20 / 21) K steps; neither: the register-staged generation 1."""
    N, H, W, C, KO, R, S, stride, pad = case
    parity = stride == 2 and H % 2 == 0 and W % 2 == 0 and R <= 4 and S <= 4
    def gen(ok):
        return 3 if cand >= 20 and ok(64) else 2 if ok(32) else 1
    return (gen(lambda bk: C % bk == 0 and R * S <= 32),
            gen(lambda bk: KO % bk == 0 and R * S <= 32 and (stride == 1 or parity)))


def _wgrad_generation(case, cand, split):
    """gemm_kernel.h:1834 (`slices_ok`): generation 3 only when the 64-deep K tiles split into exactly the slices the caller sized."""
    if cand < 20 or split <= 0:
        return 3 if cand >= 20 else 2
    N, H, W, C, KO, R, S, stride, pad = case
    Kd = N * ((H + 2 * pad - R) // stride + 1) * ((W + 2 * pad - S) // stride + 1)
    nkt32, nkt64 = _cdiv(Kd, 32), _cdiv(Kd, 64)
    s = min(split, nkt32)
    s = _cdiv(nkt32, _cdiv(nkt32, s))
    return 3 if s == 1 or (s <= nkt64 and _cdiv(nkt64, _cdiv(nkt64, s)) == s) else 2


CONV_PARAMS = [pytest.param(b.values[0], 0, c, case, marks=b.marks, id=f"{b.values[0]}-tile{c}-" + "x".join(map(str, case)))
               for case in CONV_CASES for c in (-1, 2) for b in BACKENDS] + \
              [pytest.param(p.values[0], p.values[1], p.values[2], case, marks=p.marks, id=p.id + "-" + "x".join(map(str, case)))
               for case in CONV_CASES if _conv_generations(case, 20)[0] == 3 for p in _tile_params([20, 21])]


@pytest.mark.parametrize("backend,late,cand,case", CONV_PARAMS)
def test_convolutions_elementwise(backend, late, cand, case):
    """Forward, input gradient and weight gradient (one / chosen / two / three K slices, into a guarded slice of a flat sentinel
    buffer) on the automatic tile, the 128 x 128 tile and, where the channel counts admit 64-deep K steps, generation 3."""
    dev = select(backend)
    N, H, W, C, KO, R, S, stride, pad = case
    t = _conv_operands(case)
    gf, gd = _conv_generations(case, cand)
    with _tile(backend, cand, late):
        y = ops.conv2d_fwd(t["x"].to(dev), t["w"].to(dev), stride, pad)
        assert _generation() == gf, ("fwd", _generation(), gf)
        assert_elementwise(y, *t["fwd"], f"conv2d_fwd {case} tile {cand}")
        dx = ops.conv2d_dgrad(t["dy"].to(dev), t["wt"].to(dev), t["x"].shape, stride, pad)
        assert _generation() == gd, ("dgrad", _generation(), gd)
        assert_elementwise(dx, *t["dgrad"], f"conv2d_dgrad {case} tile {cand}")
        n, guard = t["dw0"].numel(), 1024
        for split in (0, 2, 3):
            buf = torch.full((n + 2 * guard,), SENTINEL, device=dev)
            dw = buf[guard:guard + n].view(KO, R, S, C)
            dw.copy_(t["dw0"])
            got = ops.conv2d_wgrad(t["x"].to(dev), t["dy"].to(dev), dw, stride, pad, split_k=split)
            assert _generation() == _wgrad_generation(case, cand, split), ("wgrad", split, _generation())
            assert_elementwise(got, *t["wgrad"], f"conv2d_wgrad {case} tile {cand} split_k {split}")
            host = buf.cpu()
            assert bool((host[:guard] == SENTINEL).all()) and bool((host[guard + n:] == SENTINEL).all()), f"conv2d_wgrad {case}: wrote outside dw"


BN_CASE, BN_SEED = (3, 9, 11, 32, 64, 3, 3, 1, 1), 5


@functools.lru_cache(maxsize=None)
def _bn_dgrad_operands():
    N, H, W, C, KO, R, S, stride, pad = BN_CASE
    g = torch.Generator().manual_seed(BN_SEED)
    t = dict(x=(0.7 * torch.randn(N, H, W, C, generator=g) + 0.3).to(BF), w=(torch.randn(KO, R, S, C, generator=g) / (R * S * C) ** 0.5).to(BF),
             dy=torch.randn(N, H, W, KO, generator=g).to(BF), res=torch.randn(N, H, W, C, generator=g).to(BF),
             gamma=0.5 + torch.rand(C, generator=g), beta=0.2 * torch.randn(C, generator=g),
             ymask=torch.relu(torch.randn(N, H, W, C, generator=g)).to(BF))
    xf = t["x"].float().view(-1, C)
    t["mean"], t["rstd"] = xf.mean(0), (xf.var(0, unbiased=False) + 1e-5).rsqrt()
    t["wt"] = t["w"].permute(3, 1, 2, 0).contiguous()
    dx, S_, K = ew.conv_dgrad_terms(t["dy"], t["w"], t["x"].shape, stride, pad)
    z = dx + t["res"].double()
    # the kernels round the accumulator to bf16 on its way through the LDS strip (gemm_kernel.h:1407) before stats_math adds the
    # residual to it (gemm_kernel.h:698) and rounds again for the store (gemm_kernel.h:736): one extra bf16 rounding of dx
    t["z"], t["zbound"] = z, ew.contraction_bound(z, S_ + t["res"].double().abs(), K, BF, e_epi=ew.U_OUT[BF] * dx.abs())
    return t


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cand", [-1, 2])
@pytest.mark.parametrize("mode", ["remask", "ybits"])
def test_dgrad_with_fused_batchnorm_backward_elementwise(backend, cand, mode):
    """dz = mask(dgrad + residual), element by element against _bn_bwd_reference's formula in float64.  `remask` recomputes the
    ReLU mask as xhat * gamma + beta > 0 in fp32: where the float64 value of that expression lies within its fp32 evaluation
    error of zero the kernel may decide either way, and that element's bound grows by |dz unmasked|.  Seed 5 (chosen on the
    CPU, from the float64 reference alone): 0 of the 9504 elements are such -- asserted below to be < 1 %, so the escape cannot
    swallow a failure.  `ybits` takes the mask as bits: no decision is in doubt."""
    dev = select(backend)
    t = _bn_dgrad_operands()
    N, H, W, C, KO, R, S, stride, pad = BN_CASE
    x64, mean, rstd, gamma, beta = (t[k].double() for k in ("x", "mean", "rstd", "gamma", "beta"))
    z, bound = t["z"].view(-1, C), t["zbound"].view(-1, C).clone()
    if mode == "remask":
        ref = _bn_bwd_reference(z, x64.view(-1, C), mean, rstd, gamma, beta, None, "remask")[0]
        xs, ms = x64.view(-1, C) * rstd, mean * rstd
        xh = xs - ms
        arg = xh * gamma + beta
        # fp32 evaluation of  (x * rstd + fl(-mean * rstd)) * gamma + beta  (stats_math, gemm_kernel.h:730-731; par[] at :1315):
        e_arg = ew.U32 * (gamma.abs() * (ms.abs()              # fl(-mean * rstd), once per channel
                                         + xs.abs()            # the product x * rstd
                                         + xh.abs())           # its sum with the shift
                          + (xh * gamma).abs()                 # the product with gamma
                          + arg.abs())                         # the sum with beta
        undecided = arg.abs() <= e_arg
        assert int(undecided.sum()) == 0 and undecided.float().mean().item() < 0.01, int(undecided.sum())
        bound = bound + torch.where(undecided, z.abs(), torch.zeros_like(z))
        bn = ops.BnBwd(t["x"].to(dev), t["mean"].to(dev), t["rstd"].to(dev), gamma=t["gamma"].to(dev), beta=t["beta"].to(dev))
    else:
        ref = _bn_bwd_reference(z, x64.view(-1, C), mean, rstd, gamma, beta, t["ymask"].double().view(-1, C), "ymask")[0]
        bn = ops.BnBwd(t["x"].to(dev), t["mean"].to(dev), t["rstd"].to(dev), ybits=_pack_mask_bits(t["ymask"]).to(dev))
    with _tile(backend, cand):
        dz, st = ops.conv2d_dgrad(t["dy"].to(dev), t["wt"].to(dev), t["x"].shape, stride, pad, residual=t["res"].to(dev), bn=bn)
    assert st is not None and st.strips > 0
    assert_elementwise(dz, ref.view(N, H, W, C), bound.view(N, H, W, C), f"conv2d_dgrad + BatchNorm backward ({mode}, tile {cand})")


# ---------------------------------------------------------------------------------------------------- streaming MFMA kernels
@pytest.mark.parametrize("backend", BACKENDS)
def test_expand1x1_elementwise(backend):
    import os
    if os.environ.get("VIRTEX_AMD_EXPAND1X1", "1") == "0":
        pytest.skip("the streaming kernel is switched off (VIRTEX_AMD_EXPAND1X1=0; read once per process)")
    dev = select(backend)
    M, K, N = 4111, 128, 512
    g = torch.Generator().manual_seed(M + K + N)
    a = torch.randn(M, K, generator=g).to(BF); w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
    m = ew.gemm_nt_model(a, w)
    ops.profile_start()
    try:
        y, st = ops.gemm_nt(a.to(dev), w.to(dev), bn_shift=torch.zeros(N, device=dev))
    finally:
        names = _kernel_names(ops.profile_stop())
    assert any("expand1x1" in n for n in names) and st is not None, names
    assert_elementwise(y, m["ref"], m["bound"], "expand1x1 4111x512x128")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", [(2, 9, 9, 32, 32), (1, 12, 45, 64, 64)], ids=["2x9x9x32x32", "1x12x45x64x64"])
def test_conv3x3_shared_tile_kernel_elementwise(backend, shape):
    dev = select(backend)
    N, H, W, C, KO = shape
    t = _conv_operands((N, H, W, C, KO, 3, 3, 1, 1))
    _lib.call("vtx_set_switch", b"conv3x3_shared", 2)
    try:
        ops.profile_start()
        try:
            y = ops.conv2d_fwd(t["x"].to(dev), t["w"].to(dev), 1, 1)
            dx = ops.conv2d_dgrad(t["dy"].to(dev), t["wt"].to(dev), t["x"].shape, 1, 1)
        finally:
            recs = ops.profile_stop()
    finally:
        _lib.call("vtx_set_switch", b"conv3x3_shared", 1)
    assert sum(r["launches"] for r in recs if "Conv3x3SharedA" in r["name"]) == 2, _kernel_names(recs)
    assert_elementwise(y, *t["fwd"], f"conv3x3 shared tile fwd {shape}")
    assert_elementwise(dx, *t["dgrad"], f"conv3x3 shared tile dgrad {shape}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_grouped_conv3x3_elementwise(backend):
    """The smallest group configuration of test_grouped_conv.py: 32 groups of 4 channels, stride 1."""
    dev = select(backend)
    N, H, W, Cg, G, stride = 2, 9, 9, 4, 32, 1
    C = Cg * G
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, H, W, C, generator=g).to(BF); w = (torch.randn(C, 3, 3, Cg, generator=g) / (9 * Cg) ** 0.5).to(BF)
    dy = torch.randn(N, H, W, C, generator=g).to(BF); dw0 = torch.randn(C, 3, 3, Cg, generator=g)
    y = ops.conv2d_fwd(x.to(dev), w.to(dev), stride, 1, groups=G)
    assert_elementwise(y, *ew.conv_fwd_model(x, w, stride, 1, BF, groups=G), "gconv3x3 fwd")
    dx = ops.conv2d_dgrad(dy.to(dev), w.to(dev), x.shape, stride, 1, groups=G)
    assert_elementwise(dx, *ew.conv_dgrad_model(dy, w, x.shape, stride, 1, BF, groups=G), "gconv3x3 dgrad")
    dw = ops.conv2d_wgrad(x.to(dev), dy.to(dev), dw0.clone().to(dev), stride, 1, groups=G)
    assert_elementwise(dw, *ew.conv_wgrad_model(x, dy, dw0, stride, 1, groups=G), "gconv3x3 wgrad")
