"""The device nucleus-sampling step (csrc/nucleus.hip, `draw="device"`) against an fp64 restatement of its contract."""
import pytest
import torch

from backends import BACKENDS, select
from oracle import decoding_cases as dc
from virtex_amd import ops
from virtex_amd.decoding import AutoRegressiveNucleusSampling

EOS = 2
TAU = 1e-5      # exp(x - max) with |x - max| <~ 40 carries a few 1e-6 relative from the fp32 exponent argument, a sum of them no more


def reference(x, last, u, p):
    """One row in fp64 -> (order, cum over the order, rank of every token)."""
    x = x.double()
    order = torch.sort(-x, stable=True).indices                # descending logit, ties by ascending index
    e = torch.exp(x - x.max())[order]
    cum = torch.cumsum(e / e.sum(), 0)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(x.numel())
    return order, cum, rank


def check_row(x, last, u, p, token, k):
    V = x.numel()
    order, cum, rank = reference(x, last, u, p)
    assert 1 <= k <= V
    if k > 1:
        assert cum[k - 2] <= p + TAU                           # the last kept token's predecessors stay under the threshold
    if k < V:
        assert cum[k - 1] > p - TAU                            # ... and it crosses it
    if last == EOS:
        assert token == EOS
        return
    cand = order[:k][order[:k] != last]
    if cand.numel() == 0:
        assert token == min(int(float(u) * V), V - 1)          # u is fp32: the product is exact in a double
        return
    assert rank[token] < k and token != last
    mass = torch.exp(x.double() - x.double().max())[cand]
    C, M = torch.cumsum(mass, 0), mass.sum()
    j = int((cand == token).nonzero())
    assert (C[j - 1] if j else 0.0) - TAU * M <= float(u) * M < C[j] + TAU * M


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("V,p,scale,q,pad", [(1, .9, 3, None, 0), (7, .9, 3, None, 0), (64, .5, 3, None, 0), (255, .9, 3, None, 1),
                                             (257, .9, 3, None, 0), (1000, .9, 1, .5, 0), (1000, .99, 3, None, 0),
                                             (10007, .9, .5, .25, 2), (40000, .9, 1, None, 0)])   # 40000: above the LDS-resident bound
def test_step_against_fp64_reference(backend, V, p, scale, q, pad):
    dev = select(backend)
    g = torch.Generator().manual_seed(V)
    rows = 8
    store = scale * torch.randn(rows, V + pad, generator=g)    # pad: an odd row stride (and rows off the 16-byte grid)
    if q:
        store = torch.round(store / q) * q
    x = store[:, :V]
    u = torch.rand(rows, generator=g)
    last = torch.randint(0, V, (rows,), generator=g)
    last[::2] = x[::2].argmax(1)
    if V > EOS:
        last[3] = EOS
    token, kept = ops.nucleus_step(store.to(dev)[:, :V], last.to(dev), u.to(dev), EOS, p)
    assert token.dtype == torch.int64 and kept.dtype == torch.int32
    for r in range(rows):
        check_row(x[r], int(last[r]), u[r], p, int(token[r]), int(kept[r]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_edge_rows_exact(backend):
    dev = select(backend)
    top = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))

    def run(x, last, u, p=.9):
        t, k = ops.nucleus_step(x.to(dev), torch.tensor(last).to(dev), torch.tensor(u, dtype=torch.float32).to(dev), EOS, p)
        return t.tolist(), k.tolist()
    assert run(torch.zeros(2, 1), [0, 5], [.3, .7]) == ([0, 0], [1, 1])                   # V = 1: uniform branch / the only token
    peaked = torch.zeros(4, 10)
    peaked[:, 7] = 20.0                                                                   # token 7 alone holds more than p
    assert run(peaked, [7, 7, 7, 1], [0.0, .55, top, .5]) == ([0, 5, 9, 7], [1, 1, 1, 1])  # last = 7: uniform over V; else 7
    flat = torch.full((4, 10), 1.5)                                                       # all equal: ranks are token indices
    tok, kept = run(flat, [0, 9, 3, 3], [0.0, top, 0.0, top], p=.75)
    assert kept == [8, 8, 8, 8] and tok == [1, 7, 0, 7]                                   # floor(.75 * 10) + 1 kept; last is skipped
    with pytest.raises(RuntimeError, match="outside"):
        run(flat, [0] * 4, [.5] * 4, p=1.0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_decoder_with_device_draw(backend):
    dev = select(backend)
    step_cpu = dc.make_step(4)
    start = torch.full((6,), dc.SOS, dtype=torch.long, device=dev)
    dec = AutoRegressiveNucleusSampling(dc.EOS, max_steps=8, nucleus_size=.9, draw="device")

    def sample(seed):
        torch.manual_seed(seed)
        tokens, lp = dec.search(start, lambda partial: step_cpu(partial.cpu()).to(dev))
        return tokens.cpu()
    a, b, c = sample(1), sample(1), sample(2)
    assert a.dtype == torch.long and a.shape[0] == 6 and 1 <= a.shape[1] <= 8
    full = torch.cat([torch.full((6, 1), dc.SOS), a], 1)
    ended = (full[:, :-1] == dc.EOS)
    assert (full[:, 1:][ended] == dc.EOS).all()                 # eos is absorbing
    assert (full[:, 1:] != full[:, :-1])[~ended].all()          # and nothing else repeats its predecessor
    assert torch.equal(a, b) and (a.shape != c.shape or not torch.equal(a, c))
    with pytest.raises(ValueError):
        AutoRegressiveNucleusSampling(dc.EOS, draw="bogus")
