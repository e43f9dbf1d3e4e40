"""Masked language modelling on the labelled rows only: compaction, pack / unpack (csrc/masked_ce.hip), the compacted tied
projection + cross-entropy, non-causal ragged self-attention and MaskedLMModel.  Every reference is float64 torch written here."""
import types

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from backends import BACKENDS, rel_err, select
from test_classification import StubVisual
from virtex_amd import factories, models, ops
from virtex_amd.modules import textual_heads

DTYPES = [torch.float32, torch.bfloat16]
PAD = 0


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def spread_labels(R, V, count, seed):
    """(R,) int64 with exactly `count` labelled rows (first and last among them), padding elsewhere"""
    g = torch.Generator().manual_seed(seed)
    pick = torch.cat([torch.tensor([0, R - 1]), 1 + torch.randperm(R - 2, generator=g)[: count - 2]])
    labels = torch.zeros(R, dtype=torch.int64)
    labels[pick] = torch.randint(1, V, (count,), generator=g)
    return labels


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["mixed", "none", "all"])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 90, 1024, 1025, 2100])
def test_label_compact(backend, R, kind):
    """row 0 and R-1, a run over a wave boundary (60-70) and over the strip boundary (1020-1030), an out-of-range and a negative label"""
    dev, V = select(backend), 50
    labels = torch.full((R,), PAD if kind != "all" else 7, dtype=torch.int64)
    if kind == "mixed":
        labels[[0, R - 1]] = 3
        labels[60:71] = 5
        labels[1020:1031] = V - 1
        if R > 3:
            labels[R // 2], labels[R // 3] = V, -3
    mask = (labels != PAD) & (labels >= 0) & (labels < V)
    rows, slot, count = (t.cpu() for t in ops.label_compact(labels.to(dev), PAD, V))
    n = int(mask.sum())
    assert count.item() == n and rows.dtype == slot.dtype == torch.int32
    assert torch.equal(rows[:n].long(), torch.nonzero(mask).flatten())
    assert torch.equal(slot.long(), torch.where(mask, mask.cumsum(0) - 1, torch.tensor(-1)))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 64, 136])
@pytest.mark.parametrize("cap", [5, 13, 20])
def test_rows_pack_and_unpack(backend, dtype, H, cap):
    """13 labelled rows of 90, capacity below / equal / above; both directions with row strides larger than H; bit-equal copies"""
    dev, R, n = select(backend), 90, 13
    g = torch.Generator().manual_seed(H + cap)
    labels = spread_labels(R, 40, n, seed=H)
    where = torch.nonzero(labels != PAD).flatten()
    wide = torch.randn(R, H + 16, generator=g).to(dtype)
    rows, slot, count = ops.label_compact(labels.to(dev), PAD, 40)
    packed, targets = (t.cpu() for t in ops.rows_pack(wide.to(dev)[:, :H], labels.to(dev), rows, count, cap, PAD))
    m = min(n, cap)
    first = 1 if n > cap else 0                                 # the batch exceeds the capacity: row 0 is poisoned
    assert torch.equal(bits(packed[first:m]), bits(wide[where[first:m], :H])) and torch.equal(targets[:m], labels[where[:m]])
    assert torch.isnan(packed[0].float()).all() == (n > cap)
    assert (bits(packed[m:]) == 0).all() and (targets[m:] == PAD).all()
    dpacked = torch.randn(cap, H, generator=g).to(dtype)
    out = torch.full((R, H + 16), float("nan")).to(dtype).to(dev)
    ops.rows_unpack(dpacked.to(dev), slot, out=out[:, :H])
    want = torch.zeros(R, H, dtype=dtype)
    want[where[:m]] = dpacked[:m]
    assert torch.equal(bits(out.cpu()[:, :H]), bits(want)) and torch.isnan(out.cpu()[:, H:].float()).all()


def masked_loss(dev, dtype, h, w, b, labels, cap="exact", gout=1.7):
    """loss and (d hidden, d weight, d bias) of the compacted path: hidden in `dtype`, fp32 master weight and bias"""
    hd = h.to(dtype).to(dev)[None].requires_grad_()
    wp, bp = nn.Parameter(w.to(dev)), nn.Parameter(b.to(dev))
    if cap == "exact":
        cap = max(1, -(-int((labels != PAD).sum()) // models.MASKED_CE_GRANULE)) * models.MASKED_CE_GRANULE
    loss = models._MaskedTiedCrossEntropyFn.apply(hd, wp, bp, labels.to(dev)[None], PAD, cap, None)
    (loss * gout).backward()
    return loss.item(), [t.grad.float().cpu() for t in (hd, wp, bp)]


def dense_loss(dtype, h, w, b, labels, gout=1.7):
    """F.cross_entropy(h @ W^T + b) in float64 on the operands as the kernels see them (rounded to `dtype`)"""
    h64, w64, b64 = (t.double().requires_grad_() for t in (h.to(dtype), w.to(dtype), b))
    loss = F.cross_entropy(h64 @ w64.t() + b64, labels, ignore_index=PAD)
    (loss * gout).backward()
    return loss.item(), [h64.grad, w64.grad, b64.grad]


def operands(R, V, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, H, generator=g), 0.3 * torch.randn(V, H, generator=g), 0.2 * torch.randn(V, generator=g)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V,H,count", [(150, 1000, 64, 25), (70, 304, 128, 12), (1100, 200, 64, 128), (1100, 200, 64, 129)])
def test_compacted_tied_cross_entropy(backend, dtype, R, V, H, count):
    """Bounds of test_tied_projection_cross_entropy_without_logits.  Measured on the MI355X (loss, d hidden, d weight, d bias),
    worst of the four cases: fp32 7.2e-8, 6.4e-7, 4.8e-7, 5.1e-7; bf16 9.4e-8, 2.4e-3, 1.7e-3, 1.8e-3."""
    dev = select(backend)
    h, w, b = operands(R, V, H, R + V)
    labels = spread_labels(R, V, count, seed=count)
    ref, gref = dense_loss(dtype, h, w, b, labels)
    loss, grads = masked_loss(dev, dtype, h, w, b, labels)
    errs = [abs(loss - ref) / abs(ref)] + [rel_err(a, r) for a, r in zip(grads, gref)]
    print(f"MEASURED {backend} {dtype} R={R} count={count}: loss {errs[0]:.2e} dh {errs[1]:.2e} dW {errs[2]:.2e} db {errs[3]:.2e}")
    assert errs[0] < (2e-5 if dtype == torch.float32 else 2e-4)
    assert max(errs[1:]) < (2e-5 if dtype == torch.float32 else 1e-2), errs
    assert (grads[0][0][labels == PAD] == 0).all()             # exact zeros at the unlabelled rows


@pytest.mark.parametrize("backend", BACKENDS)
def test_label_capacity(backend):
    dev = select(backend)
    h, w, b = operands(150, 200, 64, 9)
    labels = spread_labels(150, 200, 25, seed=1)
    exact, _ = masked_loss(dev, torch.float32, h, w, b, labels)
    roomy, _ = masked_loss(dev, torch.float32, h, w, b, labels, cap=40)
    assert abs(roomy - exact) < 2e-5 * abs(exact)
    assert torch.isnan(torch.tensor(masked_loss(dev, torch.float32, h, w, b, labels, cap=24)[0]))      # one row too many
    nothing = torch.zeros(150, dtype=torch.int64)
    assert all(torch.isnan(torch.tensor(masked_loss(dev, torch.float32, h, w, b, nothing, cap=c)[0])) for c in ("exact", 8))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [12, 30])
def test_noncausal_self_attention_with_ragged_keys(backend, dtype, T):
    """causal = 0 with key_lengths and T = S <= 32: what masked LM issues and bicaptioning never does"""
    dev, B, A = select(backend), 3, 2
    g = torch.Generator().manual_seed(T)
    Hd = A * 64
    qkv, dout = torch.randn(B * T, 3 * Hd, generator=g).to(dtype), torch.randn(B * T, Hd, generator=g).to(dtype)
    lengths = torch.tensor([T, 1, T // 2 + 1])
    q, k, v = (qkv[:, i * Hd:(i + 1) * Hd].double().reshape(B, T, A, 64).transpose(1, 2).requires_grad_() for i in range(3))
    mask = torch.zeros(B, 1, 1, T, dtype=torch.float64).masked_fill((torch.arange(T)[None] >= lengths[:, None])[:, None, None], -1e300)
    oref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0 + mask, -1) @ v).transpose(1, 2).reshape(B * T, Hd)
    oref.backward(dout.double())
    qd, dqkv = qkv.to(dev), torch.empty(B * T, 3 * Hd, dtype=dtype, device=dev)
    parts, dparts = [qd[:, i * Hd:(i + 1) * Hd] for i in range(3)], [dqkv[:, i * Hd:(i + 1) * Hd] for i in range(3)]
    o = ops.attention_fwd(*parts, B, A, T, T, False, lengths.to(dev))
    e = 2e-5 if dtype == torch.float32 else 1e-2
    assert rel_err(o.float().cpu(), oref.detach()) < e
    ops.attention_bwd(*parts, dout.to(dev), *dparts, B, A, T, T, False, lengths.to(dev))
    for got, ref in zip(dparts, (q, k, v)):
        assert rel_err(got.float().cpu(), ref.grad.transpose(1, 2).reshape(B * T, Hd)) < 2 * e


class Restatement(nn.Module):
    """The reference's head under its state-dict keys (textual_heads.py:98-278, embedding.py:8-86) on stock torch modules"""

    def __init__(self, C, V, H, F_, norm_first):
        super().__init__()
        self.visual_projection = nn.Linear(C, H)
        self.embedding = nn.Module()
        self.embedding.words, self.embedding.positions = nn.Embedding(V, H, padding_idx=PAD), nn.Embedding(30, H)
        self.embedding.layer_norm = nn.LayerNorm(H, eps=1e-8)
        layer = nn.TransformerDecoderLayer(H, 1, F_, dropout=0.0, activation="gelu", batch_first=True, norm_first=norm_first)
        self.transformer = nn.TransformerDecoder(layer, 1, norm=nn.LayerNorm(H) if norm_first else None)
        self.output = nn.Linear(H, V)
        self.output.weight = self.embedding.words.weight

    def forward(self, grid, tokens, lengths):
        B, T = tokens.shape
        x = self.embedding.words(tokens) + self.embedding.positions(torch.arange(T))[None]
        x = self.embedding.layer_norm(x) * (tokens != PAD)[..., None]
        memory = self.visual_projection(grid.reshape(B, -1, grid.shape[-1]))
        padded = torch.arange(T)[None] >= lengths[:, None]
        return self.output(self.transformer(x, memory, tgt_key_padding_mask=padded))          # no causal mask


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("norm_first", [False, True])
def test_masked_lm_model(backend, norm_first):
    dev = select(backend)
    B, T, C, V, H = 3, 12, 32, 200, 64
    torch.manual_seed(V + norm_first)
    head = textual_heads.TransformerDecoderTextualHead(C, V, H, 1, 1, 128, dropout=0.0, norm_first=norm_first,
                                                       mask_future_positions=False, compute_dtype=torch.float32)
    lengths = torch.tensor([T, 5, 9])
    tokens = torch.randint(5, V, (B, T)) * (torch.arange(T)[None] < lengths[:, None])
    labels = torch.zeros_like(tokens)
    for b_, t_ in ((0, 0), (0, 11), (1, 3), (2, 1), (2, 8)):
        labels[b_, t_], tokens[b_, t_] = tokens[b_, t_], 4       # [MASK]
    ref = Restatement(C, V, H, 128, norm_first)
    ref.load_state_dict(head.state_dict())
    ref = ref.double().train()
    model = factories.PretrainingModelFactory.create("masked_lm", StubVisual(B, C, 2, 2, seed=3), head).to(dev).train()
    assert type(model) is models.MaskedLMModel and model.padding_idx == PAD and isinstance(model.loss, nn.CrossEntropyLoss)
    grid64 = model.visual.grid.detach().cpu().double().requires_grad_()
    logits64 = ref(grid64, tokens, lengths)
    loss64 = F.cross_entropy(logits64.view(-1, V), labels.view(-1), ignore_index=PAD)
    loss64.backward()
    batch = {"image": None, "caption_tokens": tokens.to(dev), "caption_lengths": lengths.to(dev), "masked_labels": labels.to(dev)}
    out = model(batch)
    out["loss"].backward()
    assert set(out) == {"loss", "loss_components"} and set(out["loss_components"]) == {"masked_lm"}
    assert abs(out["loss"].item() - loss64.item()) < 1e-5 * abs(loss64.item())
    want = dict(ref.named_parameters())
    errs = {n: rel_err(p.grad.cpu(), want[n].grad) for n, p in head.named_parameters()}
    errs["grid"] = rel_err(model.visual.grid.grad.cpu(), grid64.grad)
    print({n: f"{e:.1e}" for n, e in errs.items()})
    assert set(errs) == set(want) | {"grid"} and max(errs.values()) < 1e-3, errs
    with torch.no_grad():
        pred = model.eval()(batch)["predictions"].cpu()
    assert torch.equal(pred, torch.where(labels != PAD, logits64.argmax(-1), torch.tensor(PAD)))


def test_register_installs_masked_lm_on_request():
    fake = types.SimpleNamespace(**{n: type(n, (), {"PRODUCTS": {}}) for n in (
        "VisualBackboneFactory", "TextualHeadFactory", "PretrainingModelFactory", "CaptionDecoderFactory")})
    assert "PretrainingModelFactory.masked_lm" not in factories.register(fake) and "masked_lm" not in fake.PretrainingModelFactory.PRODUCTS
    assert "PretrainingModelFactory.masked_lm" in factories.register(fake, masked_lm=True)
    assert fake.PretrainingModelFactory.PRODUCTS["masked_lm"] is models.MaskedLMModel
