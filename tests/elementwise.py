"""Element-by-element comparison of a contraction kernel's output with a float64 reference, under a bound derived from the
arithmetic the kernel is allowed to do -- never from what a kernel returned.

    bound = u_out * |ref|  +  L * (K + 8) * 2^-24 * S  +  e_epi

* S      the float64 sum of the ABSOLUTE values of every term of the element (|alpha| |a| @ |b|^T + |bias| + |residual| ...):
         the scale every fp32 rounding of the sum is relative to.
* (K + 8) * 2^-24 * S   the worst case of an fp32 sum of K exact products in ANY order (bf16 x bf16 is exact in fp32; K - 1
         additions of at most half an fp32 ulp of a partial sum that never exceeds S): the MFMA order, split-K slices and
         their reduction are all orders of that one sum.  The + 8 pays for the fp32 roundings around it: the alpha product,
         the bias add, the residual / accumulator add, the split-K reduction's add into the gradient (each <= 2^-24 * S).
* u_out  the store: 2^-8 for bf16 (twice the half-ulp 2^-9: a hardware convert and ties), 2^-23 for fp32.
* L      Lipschitz constant of the epilogue function: what the error of its argument is multiplied by.
* e_epi  the fp32 evaluation error of the epilogue itself, and roundings the kernels are documented to make on the way.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                    # half an ulp of fp32, relative: one rounding of an fp32 operation
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
L_GELU = 1.13                       # max |d/dx gelu_erf(x)| = 1.1289 (at x = sqrt(2)): csrc/vtx_common.h:350
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2


def _box(idx, names):
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    return ", ".join(f"{n} {a}..{b}" for n, a, b in zip(names, lo, hi))


def assert_elementwise(got, ref64, bound, what, names=None):
    """Fails when ANY element has |got - ref64| > bound (bound: per-element float64 tensor).  The message gives the number of
    violating elements, the worst one (index, got, ref, bound) and the bounding box of all of them, in (n, h, w, c) terms for a
    4-D tensor and (m, n) for a matrix: 'the last row of tiles' reads differently from 'everywhere'."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape == bound.shape, (what, got.shape, ref64.shape, bound.shape)
    assert ref64.dtype == torch.float64 and bound.dtype == torch.float64
    err = (got - ref64).abs()
    bad = ~(err <= bound)                                # a NaN anywhere is a violation
    count = int(bad.sum())
    if count == 0:
        return
    names = names or {4: "nhwc", 2: "mn"}.get(got.dim(), [f"d{i}" for i in range(got.dim())])
    idx = bad.nonzero()
    excess = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    excess = torch.where(torch.isnan(excess), torch.full_like(excess, float("inf")), excess)
    w = tuple(int(i) for i in idx[excess[bad].argmax()])
    raise AssertionError(
        f"{what}: {count} of {got.numel()} elements outside their bound; worst at ({', '.join(f'{n}={i}' for n, i in zip(names, w))}): "
        f"got {got[w].item():.9g}, ref {ref64[w].item():.9g}, |diff| {err[w].item():.3g} > bound {bound[w].item():.3g}; "
        f"violations span {_box(idx, names)} of shape {tuple(got.shape)}")


def contraction_bound(ref64, S, K, out_dtype, L=1.0, e_epi=0.0):
    """The bound of the module docstring."""
    return U_OUT[out_dtype] * ref64.abs() + L * (K + 8) * U32 * S + e_epi


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_eval_error(x64):
    """fp32 evaluation error of gelu_erf(x) = 0.5f * x * (1.f + erff(x * c)), c = fl(1/sqrt 2)  (csrc/vtx_common.h:350), for an
    exact argument x, term by term with E = erf(x / sqrt 2), |E| <= 1:"""
    ax = x64.abs()
    e = 0.3 * 2 * U32               # x * c: one product rounding + c's own rounding move erff's argument by <= 2^-23 |x| / sqrt 2;
    #                                 through erf' <= 2/sqrt(pi) exp(-x^2/2) and the factor 0.5 |x|: 0.5 * 0.798 * max(x^2 exp(-x^2/2) = 0.736) < 0.3
    e = e + 0.5 * ax * 4 * U32      # erff itself: 4 ulp (the HIP math API's documented accuracy), an ulp of |E| <= 1 is <= 2^-24 ...
    e = e + 0.5 * ax * 2 * U32      # ... and 1.f + E rounds once, at a magnitude <= 2: both enter through the factor 0.5 |x|
    e = e + U32 * gelu64(x64).abs()  # the final product (0.5f * x is exact) rounds once, relative to the result
    return e


def gemm_nt_model(a, b, bias=None, residual=None, act=ACT_NONE, alpha=1.0, out_dtype=torch.bfloat16):
    """Reference and bounds of ops.gemm_nt on ALREADY ROUNDED operands.  Returns a dict: ref / bound (the output) and
    pre_ref / pre_bound (the pre-activation alpha a b^T + bias, stored in the output type)."""
    K = a.shape[1]
    a64, b64 = a.double(), b.double()
    pre = alpha * (a64 @ b64.t())
    S = abs(alpha) * (a64.abs() @ b64.abs().t())
    if bias is not None:
        pre = pre + bias.double()
        S = S + bias.double().abs()
    if act == ACT_GELU:
        t, L, e_act = gelu64(pre), L_GELU, gelu_eval_error(pre)
    elif act == ACT_RELU:
        t, L, e_act = torch.relu(pre), 1.0, 0.0          # fmaxf is exact
    else:
        t, L, e_act = pre, 1.0, 0.0
    ref, e_epi = t, e_act
    if residual is not None:
        ref = t + residual.double()
        S = S + residual.double().abs()                  # the residual joins the sum: one more fp32 add, relative to S
        if out_dtype == torch.bfloat16:
            # the tiled kernels hand act(...) to the store stage through an LDS strip IN THE OUTPUT TYPE (gemm_kernel.h:1407,
            # st4v<TO> into the strip) and add the residual to that rounded value (EpiStore::finish, gemm_kernel.h:662,
            # add16<bf16_t>): one more bf16 rounding, of the value before the residual
            e_epi = e_epi + U_OUT[torch.bfloat16] * t.abs()
    return dict(ref=ref, bound=contraction_bound(ref, S, K, out_dtype, L, e_epi),
                pre_ref=pre, pre_bound=contraction_bound(pre, S if residual is None else S - residual.double().abs(), K, out_dtype))


def gemm_nt_fp32(a, b, bias=None, residual=None, act=ACT_NONE, alpha=1.0, out_dtype=torch.bfloat16):
    """The same operation in plain torch fp32 on the same rounded operands, rounded ONCE to the output type: what the bound must
    let through.  Returns (out, pre)."""
    pre = alpha * (a.float() @ b.float().t())
    if bias is not None:
        pre = pre + bias
    t = F.gelu(pre) if act == ACT_GELU else torch.relu(pre) if act == ACT_RELU else pre
    out = t + residual.float() if residual is not None else t
    return out.to(out_dtype), pre.to(out_dtype)


def gemm_tn_acc_model(a, b, c0, alpha):
    """out = c0 + alpha * a[K, M]^T @ b[K, N], fp32 output."""
    K = a.shape[0]
    a64, b64 = a.double(), b.double()
    ref = c0.double() + alpha * (a64.t() @ b64)
    S = c0.double().abs() + abs(alpha) * (a64.abs().t() @ b64.abs())
    return ref, contraction_bound(ref, S, K, torch.float32)


# ---- convolutions, NHWC tensors as the kernels take them: x (N, H, W, C), w (KO, R, S, C / groups), dy (N, OH, OW, KO)
def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_fwd_model(x, w, stride, pad, out_dtype, groups=1):
    y = F.conv2d(_nchw(x), _nchw(w), stride=stride, padding=pad, groups=groups)
    S = F.conv2d(_nchw(x).abs(), _nchw(w).abs(), stride=stride, padding=pad, groups=groups)
    K = w.shape[1] * w.shape[2] * w.shape[3]             # taps x channels of one group: the longest sum (interior pixels)
    return _nhwc(y), contraction_bound(_nhwc(y), _nhwc(S), K, out_dtype)


def conv_dgrad_terms(dy, w, x_shape, stride, pad, groups=1):
    """(dx, S, K) of the input gradient, NHWC float64."""
    N, H, W, C = x_shape
    size = (N, C, H, W)
    dx = torch.nn.grad.conv2d_input(size, _nchw(w), _nchw(dy), stride=stride, padding=pad, groups=groups)
    S = torch.nn.grad.conv2d_input(size, _nchw(w).abs(), _nchw(dy).abs(), stride=stride, padding=pad, groups=groups)
    K = w.shape[1] * w.shape[2] * (w.shape[0] // groups)  # taps x output channels of one group
    return _nhwc(dx), _nhwc(S), K


def conv_dgrad_model(dy, w, x_shape, stride, pad, out_dtype, groups=1):
    dx, S, K = conv_dgrad_terms(dy, w, x_shape, stride, pad, groups)
    return dx, contraction_bound(dx, S, K, out_dtype)


def conv_wgrad_model(x, dy, dw0, stride, pad, groups=1):
    """dw = dw0 + weight gradient, fp32 output; the sum runs over every output pixel of the batch."""
    wsize = (dw0.shape[0], dw0.shape[3], dw0.shape[1], dw0.shape[2])
    g = torch.nn.grad.conv2d_weight(_nchw(x), wsize, _nchw(dy), stride=stride, padding=pad, groups=groups)
    S = torch.nn.grad.conv2d_weight(_nchw(x).abs(), wsize, _nchw(dy).abs(), stride=stride, padding=pad, groups=groups)
    ref = dw0.double() + _nhwc(g)
    K = dy.shape[0] * dy.shape[1] * dy.shape[2]
    return ref, contraction_bound(ref, dw0.double().abs() + _nhwc(S), K, torch.float32)
