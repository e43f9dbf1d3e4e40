"""optimizer="adamw": the fused HIP tail (csrc/optim.hip) and the unfused torch.optim.AdamW chain against the reference's chain in
float64 on the CPU.  Tolerance per tensor: MARGIN x the maximum absolute distance of the SAME chain by stock float32 torch on the
CPU from the float64 result (the kernel folds the clip into the gradient and the bias correction into the step size: a few more
fp32 roundings than torch's order) + one fp32 ulp of the tensor's largest magnitude.  Measured: profiles/adamw_step.txt."""
import functools

import numpy as np
import pytest
import torch

from backends import BACKENDS, select
from oracle import bicaptioning as port
from virtex_amd import _lib, distributed as vd, ops
from virtex_amd.optim import FusedPretrainOptimizer, PretrainOptimizer

MARGIN = 4.0
SCHED = dict(total_steps=50, warmup_steps=10, start_step=3)
WORDS, ZERO_ROWS = "textual.embedding.words.weight", slice(8, 24)     # rows no caption touches: zero gradient on every step


class _Toy(torch.nn.Module):
    """In flat-buffer order (text, then the CNN reversed): an embedding with zero-gradient rows (decayed), a NO_DECAY LayerNorm,
    a weight of 29 full 4096-element chunks and a partial one, a 7-element bias that misaligns every chunk behind it (scalar
    loop), then the cnn-LR tensors with the channels-last 4-D weight."""

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.visual = torch.nn.Module()
        self.visual.cnn = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, bias=False), torch.nn.BatchNorm2d(16))
        self.textual = torch.nn.Module()
        self.textual.embedding = torch.nn.Module()
        self.textual.embedding.words = torch.nn.Embedding(40, 24)
        self.textual.embedding.layer_norm = torch.nn.LayerNorm(24)
        self.textual.transformer = torch.nn.Linear(24, 5000)
        self.textual.output = torch.nn.Linear(24, 7)
        w = self.visual.cnn[0].weight
        w.data = w.data.contiguous(memory_format=torch.channels_last)


def _grads(model, seed):
    g = torch.Generator().manual_seed(seed)
    grads = {n: 3.0 * torch.randn(p.shape, generator=g) for n, p in model.named_parameters()}
    grads[WORDS][ZERO_ROWS] = 0.0
    return list(grads.values())


@functools.lru_cache(maxsize=None)
def _reference_chain(dtype, k):
    """clip_grad_norm_ -> torch.optim.AdamW over the reference's groups -> Lookahead (lookahead.py:82-102) -> lr_multiplier,
    twelve steps on the CPU in `dtype`; computed once per (dtype, k) and only read afterwards."""
    model = _Toy().to(dtype)
    params = list(model.parameters())
    opt = torch.optim.AdamW(port.param_groups(model.named_parameters()))
    base = [g["lr"] for g in opt.param_groups]
    slow, kc = [p.detach().clone() for p in params], 0
    for it in range(12):
        mult = port.lr_multiplier(SCHED["start_step"] + it, SCHED["total_steps"], SCHED["warmup_steps"])
        for grp, lr in zip(opt.param_groups, base):
            grp["lr"] = lr * mult
        for p, g in zip(params, _grads(model, it)):
            p.grad = g.to(dtype)
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        opt.step()
        kc += 1
        if k is not None and kc >= k:
            kc = 0
            with torch.no_grad():
                for p, s in zip(params, slow):
                    p.mul_(0.5).add_(s, alpha=0.5)
                    s.copy_(p)
    return {n: p.detach().double() for n, p in model.named_parameters()}


def _steps(model, opt, dev, its, scale=1.0):
    for it in its:
        for p, g in zip(model.parameters(), _grads(model, it)):
            p.grad = torch.zeros_like(p) if p.grad is None else p.grad        # fused: a view of the gradient buckets
            p.grad.copy_(g.to(dev) / scale)
        opt.step(grad_scale=scale)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("variant", ["fused-host", "fused-device", "unfused"])
@pytest.mark.parametrize("k", [5, None])
def test_adamw_chain_against_fp64(backend, variant, k):
    if backend == "emu" and variant == "unfused":
        pytest.skip("torch foreach optimizer needs no emulator")
    dev = select(backend)
    model = _Toy().to(dev)
    if variant == "unfused":
        opt = PretrainOptimizer(model, optimizer="adamw", lookahead_k=k, **SCHED)
    else:
        opt = FusedPretrainOptimizer(model, vd.GradientBuckets(model, bucket_mb=0.01), optimizer="adamw", lookahead_k=k, **SCHED)
    if variant == "fused-device":
        opt.enable_device_schedule()
    try:
        _steps(model, opt, dev, range(12), scale=0.5)       # doubled gradients, scale 1/2: a 2-rank SUM
        if variant == "fused-device":
            opt.sync_host()
            assert (opt.step_idx, opt.t, opt.kc) == (15, 12, 2 if k else 12)
    finally:
        if variant == "fused-device":
            opt.disable_device_schedule()
    ref, yard = _reference_chain(torch.float64, k), _reference_chain(torch.float32, k)
    failed = []                          # the zero-gradient rows are held to their tensor's bound ... and moved: the decay acted
    for n, p in model.named_parameters():
        got = p.detach().cpu().double()
        yardstick = (yard[n] - ref[n]).abs().max().item()
        bound = MARGIN * yardstick + float(np.spacing(np.float32(ref[n].abs().max().item())))
        err = (got - ref[n]).abs().max().item()
        print(f"adamw {backend} {variant} k={k} {n}: yardstick {yardstick:.3e} bound {bound:.3e} error {err:.3e}")
        failed += [(n, err, bound)] if not err <= bound else []
        if n == WORDS:
            assert not torch.equal(got[ZERO_ROWS], _Toy().textual.embedding.words.weight.detach().double()[ZERO_ROWS])
    assert not failed, failed


@pytest.mark.parametrize("backend", BACKENDS)
def test_adamw_checkpoints_resume_and_interchange(backend, tmp_path):
    dev = select(backend)
    kw = dict(total_steps=40, warmup_steps=4, optimizer="adamw")
    model_a = _Toy(1).to(dev)
    buckets_a = vd.GradientBuckets(model_a, bucket_mb=0.01)
    opt_a = FusedPretrainOptimizer(model_a, buckets_a, **kw)
    _steps(model_a, opt_a, dev, range(5))                             # k = 5: slow == fast right now
    torch.save({"model": model_a.state_dict(), "optimizer": opt_a.state_dict()}, tmp_path / "checkpoint_5.pth")
    loaded = torch.load(tmp_path / "checkpoint_5.pth", map_location="cpu")
    sd = loaded["optimizer"]
    model_b = _Toy(2).to(dev)
    model_b.load_state_dict(loaded["model"])
    opt_b = FusedPretrainOptimizer(model_b, vd.GradientBuckets(model_b, bucket_mb=0.01), **kw)
    opt_b.load_state_dict(sd)
    assert (opt_b.step_idx, opt_b.t, opt_b.kc) == (5, 5, 0)
    _steps(model_a, opt_a, dev, range(5, 12))
    _steps(model_b, opt_b, dev, range(5, 12))
    for (n, p), (_, q) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert torch.equal(p, q), n
    # the reference side: a stock AdamW over the reference's one-group-per-tensor layout takes the file as it is
    model_c = _Toy(3)
    model_c.load_state_dict(loaded["model"])
    stock = torch.optim.AdamW(port.param_groups(model_c.named_parameters()))
    stock.load_state_dict({key: sd[key] for key in ("state", "param_groups")})
    for i, p in enumerate(model_c.parameters()):
        assert float(stock.state[p]["step"]) == 5.0 and stock.state[p]["exp_avg_sq"].abs().max() > 0
        for key in ("exp_avg", "exp_avg_sq"):
            assert tuple(stock.state[p][key].shape) == tuple(p.shape) and torch.equal(stock.state[p][key], sd["state"][i][key])
    fresh = torch.optim.AdamW(port.param_groups(_Toy(3).named_parameters())).state_dict()["param_groups"]
    for got, want, saved in zip(stock.param_groups, fresh, sd["param_groups"]):
        assert set(saved) == set(want) | {"initial_lr"} and all(got[key] == want[key] for key in want if key not in ("lr", "params"))
    # ... and so does the unfused optimizer, whose own state dict loads back into the fused one
    opt_c = PretrainOptimizer(model_c, **kw)
    opt_c.load_state_dict(sd)
    sd_c = opt_c.state_dict()
    assert opt_c.step_idx == 5 and set(sd_c["state"]) == set(sd["state"])
    opt_b.load_state_dict(sd_c)
    # the other optimizer's file is refused
    sgd = FusedPretrainOptimizer(model_a, buckets_a, total_steps=40, warmup_steps=4)
    with pytest.raises(ValueError, match="sgd.*adamw"):
        opt_b.load_state_dict(sgd.state_dict())
    with pytest.raises(ValueError, match="adamw.*sgd"):
        sgd.load_state_dict(sd)


@pytest.mark.parametrize("backend", BACKENDS)
def test_adamw_arguments(backend):
    dev = select(backend)
    model = _Toy().to(dev)
    buckets = vd.GradientBuckets(model, bucket_mb=0.01)
    for build in (lambda: FusedPretrainOptimizer(model, buckets, optimizer="nope"), lambda: PretrainOptimizer(model, optimizer="nope")):
        with pytest.raises(KeyError):
            build()
    o = FusedPretrainOptimizer(model, buckets, optimizer="adamw", lookahead_k=None)
    for helper in (o.load_slow_weights, o.restore_fast_weights):
        with pytest.raises(RuntimeError, match="lookahead_k=None"):
            helper()
    before = o.flat_p.clone()
    for bad in (dict(t=0), dict(eps=0.0), dict(betas=(0.9, 1.0)), dict(look=True)):      # look: a Lookahead step without slow weights
        a = {"t": 1, "eps": 1e-8, "betas": (0.9, 0.999), "look": False, **bad}
        with pytest.raises(_lib.VtxError):
            ops.adamw_lookahead_step(o.flat_p, buckets.flat, o.flat_m, o.flat_v, None, o.chunk_off, o.chunk_len, o.chunk_seg,
                                     o.seg_lr, o.seg_wd, 1.0, a["betas"], a["eps"], a["t"], 1.0, o.sumsq, 10.0, a["look"], 0.5)
    assert torch.equal(o.flat_p, before)                              # a refused call launches nothing
