"""Time masked language modelling at the base configuration (bf16, B = 256, T = 30, V = 10 000, H = 1 024, 5 labelled positions
per caption -- the bound of the reference's dataset, virtex/data/datasets/masked_lm.py:73-76):

  (a) head + loss, forward and backward: the tied projection + cross-entropy on the labelled rows only (csrc/masked_ce.hip),
      exact capacity (count read back on a side stream) and static capacity, against the dense fused path over all B*T rows;
  (b) the whole eager step: MaskedLMModel against the reference's formulation on the same native modules -- `textual(...)`
      logits (B, T, V) in fp32 plus torch's cross_entropy -- which is what MODEL.NAME masked_lm ran before.

All variants of a part run in ONE process, alternating after a warm-up; every repetition is timed with a host clock around work
that ends in a device synchronise (the exact mode's cost includes a host wait, which device events alone would not see).
`dense_fused_again` is the dense path measured a second time in the same rotation: the distance of its median from
`dense_fused` is the run-to-run spread that a difference has to beat.  Writes profiles/masked_lm.json.

    python tools/bench_masked_lm.py [--reps 30] [--warmup 5] [--part a|b|ab] [--out profiles/masked_lm.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from virtex_amd import _lib, factories, models  # noqa: E402

B, T, V, H, PER_CAPTION, PAD = 256, 30, 10000, 1024, 5, 0
DT = torch.bfloat16


def draw_labels(tokens, g):
    """PER_CAPTION labelled positions per caption, never the first or the last one; the token there becomes [MASK] = 3"""
    labels = torch.zeros_like(tokens)
    for b in range(tokens.shape[0]):
        pos = 1 + torch.randperm(T - 2, generator=g)[:PER_CAPTION]
        labels[b, pos] = tokens[b, pos]
        tokens[b, pos] = 3
    return labels


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    loss = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, loss.item()


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "q1_ms": q[0], "q3_ms": q[2], "max_ms": max(ms), "reps": len(ms)}


def rotate(runs, reps, warmup, dev):
    ms, losses = {k: [] for k in runs}, {}
    for i in range(warmup + reps):
        for name, fn in runs.items():                       # alternating
            t, losses[name] = timed(fn, dev)
            if i >= warmup:
                ms[name].append(t)
    return {"loss": losses, **{k: spread(v) for k, v in ms.items()}}


def head_loss_part(dev, reps, warmup):
    g = torch.Generator().manual_seed(1)
    hidden = torch.randn(B, T, H, generator=g).to(DT).to(dev).requires_grad_()
    weight = torch.nn.Parameter((0.02 * torch.randn(V, H, generator=g)).to(dev))
    bias = torch.nn.Parameter(torch.zeros(V, device=dev))
    weight.grad, bias.grad = torch.zeros_like(weight), torch.zeros_like(bias)
    labels = draw_labels(torch.randint(4, V, (B, T), generator=g), g).to(dev)

    def step(cap, exact=False):
        parts = None
        if exact:
            parts, count = models._LabelCount(labels.view(-1), PAD, V).get()
            cap = max(1, -(-count // models.MASKED_CE_GRANULE)) * models.MASKED_CE_GRANULE
        loss = models._MaskedTiedCrossEntropyFn.apply(hidden, weight, bias, labels, PAD, cap, parts)
        loss.backward()
        return loss

    runs = {"dense_fused": lambda: step(None), "compact_exact": lambda: step(None, exact=True),
            "compact_static": lambda: step(B * PER_CAPTION), "dense_fused_again": lambda: step(None)}
    res = rotate(runs, reps, warmup, dev)
    noise = abs(res["dense_fused"]["median_ms"] - res["dense_fused_again"]["median_ms"])
    res["run_to_run_spread_ms"] = noise
    res["labelled_rows"], res["rows"] = B * PER_CAPTION, B * T
    for k in ("compact_exact", "compact_static"):
        res[k + "_faster_beyond_spread"] = res[k]["median_ms"] + noise < min(res["dense_fused"]["median_ms"], res["dense_fused_again"]["median_ms"])
    return res


def whole_step_part(dev, reps, warmup):
    g = torch.Generator().manual_seed(2)
    vb = factories.VisualBackboneFactory.create("torchvision", "resnet50", visual_feature_size=2048, compute_dtype=DT)
    th = factories.TextualHeadFactory.create("transdec_postnorm", visual_feature_size=2048, vocab_size=V, hidden_size=H, num_layers=1,
                                             attention_heads=H // 64, feedforward_size=4 * H, dropout=0.1, mask_future_positions=False,
                                             max_caption_length=T, padding_idx=PAD, compute_dtype=DT)
    model = factories.PretrainingModelFactory.create("masked_lm", vb, th).to(dev).train()
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    tokens = torch.randint(4, V, (B, T), generator=g)
    labels = draw_labels(tokens, g)
    batch = {"image": torch.randn(B, 3, 224, 224, generator=g).to(dev), "caption_tokens": tokens.to(dev),
             "caption_lengths": torch.full((B,), T, dtype=torch.int64).to(dev), "masked_labels": labels.to(dev)}

    def native():
        loss = model(batch)["loss"]
        loss.backward()
        return loss

    def reference_formulation():
        logits = model.textual(model.visual(batch["image"]), batch["caption_tokens"], batch["caption_lengths"])
        loss = F.cross_entropy(logits.view(-1, V), batch["masked_labels"].view(-1), ignore_index=PAD)
        loss.backward()
        return loss

    res = rotate({"masked_lm_model": native, "logits_plus_torch_ce": reference_formulation, "masked_lm_model_again": native},
                 reps, warmup, dev)
    res["run_to_run_spread_ms"] = abs(res["masked_lm_model"]["median_ms"] - res["masked_lm_model_again"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--part", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_lm.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_masked_lm: needs an MI355X (a CPU run says nothing about speed)")
    assert _lib.backend() == "hip:gfx950", _lib.backend()
    dev = torch.device("cuda:0")
    result = {"backend": _lib.backend(), "device": torch.cuda.get_device_name(0), "dtype": "bfloat16",
              "shape": {"B": B, "T": T, "V": V, "H": H, "labelled_per_caption": PER_CAPTION},
              "timing": "host clock around forward + backward, device synchronised before and after; variants alternate in one process"}
    if "a" in a.part:
        result["head_and_loss"] = head_loss_part(dev, a.reps, a.warmup)
        print(json.dumps(result["head_and_loss"]))
    if "b" in a.part:
        result["whole_eager_step"] = whole_step_part(dev, a.reps, a.warmup)
        print(json.dumps(result["whole_eager_step"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
