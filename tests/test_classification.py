"""The classification pretraining head: global average pool, K-hot cross-entropy (csrc/classify.hip), LinearTextualHead and
ClassificationModel.  Every reference below is the mathematical definition with a dense K-hot matrix in float64 torch."""
import pytest
import torch
from torch import nn

from backends import BACKENDS, rel_err, select, tol
from virtex_amd import _lib, factories, models, ops
from virtex_amd.modules import textual_heads

DTYPES = [torch.float32, torch.bfloat16]
IGNORE = [0, 1, 2, 3]


def khot(labels, V, ignore):
    """Dense (R, V) float64 membership matrix of the label sets; out-of-range labels are dropped."""
    k = torch.zeros(labels.shape[0], V, dtype=torch.float64)
    for r, row in enumerate(labels.tolist()):
        k[r, [v for v in row if 0 <= v < V and v not in ignore]] = 1.0
    return k


def khot_loss(logits64, k):
    """mean_r ( -(1/K_r) sum_{v in S_r} log_softmax(logits)[r][v] )"""
    return -((torch.log_softmax(logits64, 1) * k).sum(1) / k.sum(1)).mean()


def draw_labels(g, R, V, L):
    """(R, L) int64: duplicates, zero padding, one V-1 per row; indices 0..3 are ignored by the callers."""
    labels = torch.randint(0, V, (R, L), generator=g)
    labels[:, L // 2:] = labels[:, : L - L // 2]            # duplicates
    labels[:, -1] = V - 1
    labels[:, -2] = 0                                        # padding
    labels[::2, 0] = 2
    return labels


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C", [(3, 49, 2048), (2, 1, 64), (5, 12, 72), (1, 49, 8)])
def test_gap(backend, dtype, B, HW, C):
    dev = select(backend)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, HW, C, generator=g).to(dtype)
    y = ops.gap_fwd(x.to(dev)).cpu()
    ref = x.double().mean(1)
    if dtype == torch.float32:
        assert rel_err(y, ref) < 1e-5
    else:
        assert torch.allclose(y.double(), ref, **tol(dtype))
    dy = torch.randn(B, C, generator=g).to(dtype)
    dx = ops.gap_bwd(dy.to(dev), HW).cpu()
    want = (dy.float() / HW).to(dtype)[:, None, :].expand(B, HW, C)
    assert dx.shape == (B, HW, C)
    assert torch.equal(dx, want) if dtype == torch.float32 else torch.allclose(dx.float(), want.float(), **tol(dtype))


@pytest.mark.parametrize("backend", BACKENDS)
def test_gap_rejects_ragged_channels(backend):
    dev = select(backend)
    with pytest.raises(_lib.VtxError):
        ops.gap_fwd(torch.zeros(2, 4, 12, device=dev))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V,ld,L", [(5, 81, 88, 18), (3, 32, 32, 4), (4, 1000, 1000, 30), (9, 10000, 10000, 30)])
def test_khot_ce(backend, dtype, R, V, ld, L):
    dev = select(backend)
    g = torch.Generator().manual_seed(V + L)
    labels = draw_labels(g, R, V, L)
    k = khot(labels, V, IGNORE)
    assert (k.sum(1) >= 1).all() and (k[:, V - 1] == 1).all()
    logits = torch.full((R, ld), 1e30)
    logits[:, :V] = 3 * torch.randn(R, V, generator=g)
    lr = logits[:, :V].double().requires_grad_()
    ref = khot_loss(lr, k)
    (ref * 1.7).backward()
    loss, lse, kcount = ops.khot_ce_fwd(logits.to(dev), labels.to(dev), IGNORE, V)
    print(f"loss {loss.item():.8f} ref {ref.item():.8f}")
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item()) + 1e-6
    assert torch.equal(kcount.cpu().double(), k.sum(1))
    d = ops.khot_ce_bwd(logits.to(dev), labels.to(dev), lse, kcount, torch.tensor([1.7], device=dev), dtype, IGNORE, V).cpu()
    err = rel_err(d[:, :V].float(), lr.grad)
    print(f"dlogits rel err {err:.3e}")
    assert err < (1e-5 if dtype == torch.float32 else 1e-2)
    assert d.shape == (R, ld) and (d[:, V:] == 0).all()


@pytest.mark.emu
def test_khot_ce_empty_set_is_nan():
    dev = select("emu")
    labels = torch.tensor([[5, 7, 5], [0, 3, 1]])
    loss, _, kcount = ops.khot_ce_fwd(torch.randn(2, 40).to(dev), labels.to(dev), IGNORE)
    assert kcount.tolist() == [2.0, 0.0] and torch.isnan(loss).all()


class StubVisual(nn.Module):
    """A (B, C, h, w) feature map as a parameter: logical NCHW over NHWC memory, like the backbone's output."""

    def __init__(self, B, C, h, w, seed):
        super().__init__()
        self.grid = nn.Parameter(torch.randn(B, h, w, C, generator=torch.Generator().manual_seed(seed)))

    def forward(self, image):
        return self.grid.permute(0, 3, 1, 2)


def dense_step(grid, weight, bias, labels, V):
    """float64 loss and gradients (weight, bias, grid) of the head + K-hot loss"""
    x, W, b = (t.detach().double().requires_grad_() for t in (grid, weight, bias))
    logits = x.mean((1, 2)) @ W.t() + b
    loss = khot_loss(logits, khot(labels, V, IGNORE))
    loss.backward()
    return loss.detach(), logits.detach(), (W.grad, b.grad, x.grad)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,V", [(64, 81), (128, 200)])
def test_classification_model(backend, dtype, C, V):
    """The forward projection is fp32 in both compute dtypes (loss to 1e-7, top-10 gap 0); the dtype is the operand type of the
    backward GEMMs: gradients 5e-8 .. 2.4e-7 in fp32, 2.2e-3 (weight), 1.0e-3 (bias), 3.3e-3 (features) in bf16."""
    dev = select(backend)
    B, L = 4, 9
    torch.manual_seed(V)
    head = textual_heads.LinearTextualHead(C, V, compute_dtype=dtype)
    model = models.MultiLabelClassificationModel(StubVisual(B, C, 3, 3, seed=C), head, IGNORE).to(dev)
    batch = {"image": None, "labels": draw_labels(torch.Generator().manual_seed(C + V), B, V, L).to(dev)}
    loss64, logits64, grads64 = dense_step(model.visual.grid.cpu(), head.output.weight.cpu(), head.output.bias.cpu(),
                                           batch["labels"].cpu(), V)
    out = model.train()(batch)
    out["loss"].backward()
    with torch.no_grad():
        pred = model.eval()(batch)["predictions"].cpu()
    got = (head.output.weight.grad, head.output.bias.grad, model.visual.grid.grad)
    errs = [rel_err(a.float().cpu(), r) for a, r in zip(got, grads64)]
    lp = torch.log_softmax(logits64, 1)
    top_gap = (lp.gather(1, pred).sort(1, descending=True)[0] - lp.topk(10, 1)[0]).abs().max().item()
    print(f"loss {out['loss'].item():.8f} ref {loss64.item():.8f}; grad rel err weight {errs[0]:.3e} bias {errs[1]:.3e} "
          f"features {errs[2]:.3e}; top-10 log-prob gap {top_gap:.3e}")
    assert set(out) == {"loss", "loss_components"} and set(out["loss_components"]) == {"classification"}
    assert got[0].shape == (V, C) and got[1].shape == (V,) and pred.shape == (B, 10)
    assert max(errs) < (2e-5 if dtype == torch.float32 else 2e-2), errs
    assert abs(out["loss"].item() - loss64.item()) < 1e-5 * abs(loss64.item()) + 1e-6
    assert top_gap < 1e-5
    plain = nn.Module()
    plain.output = nn.Linear(C, V)
    plain.load_state_dict(head.state_dict())
    assert torch.equal(plain.output.weight, head.output.weight.cpu())


def test_factories_build_classification():
    stub = StubVisual(2, 64, 1, 1, seed=0)
    head = factories.TextualHeadFactory.create("none", visual_feature_size=64, vocab_size=81)
    assert type(head) is textual_heads.LinearTextualHead and head.hidden_size == head.textual_feature_size == 64
    assert sorted(head.state_dict()) == ["output.bias", "output.weight"] and head.output.weight.shape == (81, 64)
    m = factories.PretrainingModelFactory.create("multilabel_classification", stub, head, ignore_indices=[0])
    assert type(m) is models.MultiLabelClassificationModel and m.visual is stub and m.textual is head and m.ignore_indices == [0]
    t = factories.PretrainingModelFactory.create("token_classification", stub, head, ignore_indices=IGNORE)
    assert type(t) is models.TokenClassificationModel and isinstance(t, models.ClassificationModel)
    assert hasattr(t, "log_predictions") and hasattr(m, "log_predictions")


@pytest.mark.reference
@pytest.mark.emu
def test_reference_classification_parity():
    """The reference's own ClassificationModel over its LinearTextualHead, fed the native head's state dict."""
    from oracle import reference_import
    reference_import.import_reference()
    from virtex.models.classification import ClassificationModel
    from virtex.modules.textual_heads import LinearTextualHead

    dev = select("emu")
    B, C, V = 4, 64, 81
    torch.manual_seed(5)
    head = textual_heads.LinearTextualHead(C, V, compute_dtype=torch.float32)
    native = models.ClassificationModel(StubVisual(B, C, 3, 3, seed=1), head, IGNORE).to(dev).train()
    ref_head = LinearTextualHead(C, V)
    ref_head.load_state_dict(head.state_dict())
    ref = ClassificationModel(StubVisual(B, C, 3, 3, seed=1), ref_head, IGNORE).train()
    batch = {"image": None, "labels": draw_labels(torch.Generator().manual_seed(3), B, V, 9)}
    a, r = native(batch)["loss"], ref(batch)["loss"]
    a.backward()
    r.backward()
    assert abs(a.item() - r.item()) < 1e-5 * abs(r.item()) + 1e-6
    for x, y in ((head.output.weight, ref_head.output.weight), (head.output.bias, ref_head.output.bias),
                 (native.visual.grid, ref.visual.grid)):
        assert rel_err(x.grad, y.grad) < 2e-5
