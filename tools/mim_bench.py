"""What masked spectrum modelling costs: the masked embedding kernels beside their plain twins, the two loss kernels against the
bytes they must move, and the ViT-B 'mim' training step beside the full-row regression step.

    python tools/mim_bench.py [--runs 30] [--warmup 3] [--steps 40] [--out profiles/mim_bench.json]

One process, hipEvents, every shape warmed up first, medians with min / max and the 10 % .. 90 % width.
Kernels (B = 256, N = 196, D = 768, P = 256, mask ratio 0.6 in blocks of 4): a round launches the plain form and then the masked
form at the same shape, so both see the same minutes of a shared box.  The expectation to confirm: the masked forms cost no more
than their plain twins beyond that width (`within_spread`).  The masked backward writes a second plane of partial sums
(min(B, 16) * T * D floats) and reduces it, which the plain one does not.
Loss kernels: pred f32 [B * T, P] (what the engine hands them) and bf16; dpred bf16.  `must_move_bytes` counts the signal and
pred of the masked windows once, the mask, the per-window partials written and read (forward), every row of dpred (backward).
Steps: ViT-B/16 geometry, B = 256, bf16-mixed, forward + backward + AdamW, eager, in alternating blocks of 4 steps: the 'mim' step
at ratio 0.6 and the regression step with `cls_tail` off -- the same engine running the last layer over every row, the path a
'mim' step extends by the three decoder products (M x 256 x 768), the loss kernels and the mask.  The regression step with the
CLS tail on (the benchmarked path) is timed in the same rounds for scale."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, P, D, LAYERS, HEADS, N = 256, 50176, 256, 768, 12, 12, 196
RATIO, SPAN = 0.6, 4
SEED = 0x1234567


def stats(ts, unit, nd):
    s = sorted(ts)
    mid = s[int(0.9 * (len(s) - 1))] - s[int(0.1 * (len(s) - 1))]
    return {f"median_{unit}": round(statistics.median(ts), nd), f"min_{unit}": round(s[0], nd), f"max_{unit}": round(s[-1], nd),
            f"p10_p90_{unit}": round(mid, nd)}


def time_calls(torch, fns, runs, warmup):
    """Per function of `fns` (launched in turn within each round): the list of its times in microseconds."""
    for _ in range(max(1, warmup)):
        for f in fns:
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(runs):
        for f, acc in zip(fns, out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3)
    return out


def kernels(runs, warmup):
    import torch
    import vit_amd.functional as vf
    from vit_amd._cabi import LOSS_L1
    from vit_amd.config import mim_blocks

    dev = torch.device("cuda", 0)
    T = N + 1
    i32, bf = torch.int32, torch.bfloat16
    nb, kb = mim_blocks(N, SPAN, RATIO)
    keep, slot = torch.empty(B, kb, dtype=i32, device=dev), torch.empty(B, nb, dtype=i32, device=dev)
    mask = torch.empty(B, N, dtype=i32, device=dev)
    vf.patch_select(B, nb, kb, SEED, 49, keep, slot)
    vf.mim_mask(slot, SPAN, mask)
    m = int(mask.sum())
    tok, cls, pos, mtok = torch.randn(B, T, D, device=dev), torch.randn(D, device=dev), torch.randn(T, D, device=dev), torch.randn(D, device=dev)
    dcls, dpos, dmt = torch.empty(D, device=dev), torch.empty(T, D, device=dev), torch.empty(D, device=dev)
    dpa = torch.empty(B * N, D, dtype=bf, device=dev)
    drop = (0.1, SEED, 0)
    rows = []
    for name, plain, masked in (
            ("embed_finish", lambda: vf.embed_finish(tok, cls, pos, dropout=drop),
             lambda: vf.embed_finish_masked(tok, cls, mask, mtok, pos, dropout=drop)),
            ("embed_finish_bwd", lambda: vf.embed_finish_bwd(tok, dcls, dpos, dropout=drop, dpatch=dpa),
             lambda: vf.embed_finish_masked_bwd(tok, mask, dcls, dmt, dpos, dropout=drop, dpatch=dpa))):
        tp, tm = time_calls(torch, (plain, masked), runs, warmup)
        sp, sm = stats(tp, "us", 1), stats(tm, "us", 1)
        rows.append({"kernel": name, "rows": B * T, "masked_rows": m, **{"plain_" + k: v for k, v in sp.items()},
                     **{"masked_" + k: v for k, v in sm.items()},
                     "within_spread": bool(sm["median_us"] <= sp["median_us"] + max(sp["p10_p90_us"], sm["p10_p90_us"]))})
    x = torch.randn(B, L, device=dev)
    dloss = torch.ones(1, device=dev)
    loss, count = torch.empty((), device=dev), torch.empty((), dtype=i32, device=dev)
    dpred = torch.empty(B * T, P, dtype=bf, device=dev)
    for pdt in (torch.float32, bf):
        pred = torch.randn(B * T, P, device=dev).to(pdt)
        pb = pred.element_size()
        fwd = lambda: vf.mim_loss_fwd(x, pred, mask, P, P, LOSS_L1, False, loss=loss, count=count)
        bwd = lambda: vf.mim_loss_bwd(x, pred, mask, count, dloss, P, P, LOSS_L1, False, dpred=dpred)
        tf, tb = time_calls(torch, (fwd, bwd), runs, warmup)
        need = {"mim_loss_fwd": m * P * (4 + pb) + 2 * B * N * 4 + 2 * B * N * 4,
                "mim_loss_bwd": m * P * (4 + pb) + B * N * 4 + B * T * P * dpred.element_size()}
        for name, ts in (("mim_loss_fwd", tf), ("mim_loss_bwd", tb)):
            st = stats(ts, "us", 1)
            rows.append({"kernel": name, "pred": str(pdt).split(".")[-1], "masked_windows": m, "must_move_bytes": need[name], **st,
                         "achieved_GBps": round(need[name] / (st["median_us"] * 1e-6) / 1e9, 1)})
    for (name, f) in (("patch_select+mim_mask", lambda: (vf.patch_select(B, nb, kb, SEED, 49, keep, slot), vf.mim_mask(slot, SPAN, mask))),):
        rows.append({"kernel": name, "blocks": B * nb, **stats(time_calls(torch, (f,), runs, warmup)[0], "us", 1)})
    return rows


def make_module(torch, task, tail=True):
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    model = dict(name="vit", task_type=task, image_size=L, patch_size=P, hidden_size=D, num_hidden_layers=LAYERS,
                 num_attention_heads=HEADS, stride_size=P, proj_fn="SW")
    config = {"model": model, "train": dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=False), "loss": {"name": "mae"},
              "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0},
              "mim": dict(mask_ratio=RATIO, span=SPAN, loss="l1")}
    seed_everything(42)
    module = ViTLModule(config=config)
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.train()
    module.model.engine.cls_tail = tail
    return module, trainer


def steps(torch, n_steps, warmup, block=4):
    g = torch.Generator(device="cpu").manual_seed(1234)
    batch = tuple(t.to("cuda:0") for t in (torch.randn((B, L), generator=g), 0.1 * torch.randn((B, L), generator=g).abs(),
                                          torch.rand((B,), generator=g)))
    keep, steppers = [], {}
    for label, task, tail in (("reg_full_rows", "reg", False), ("mim", "mim", True), ("reg_cls_tail", "reg", True)):
        module, trainer = make_module(torch, task, tail)
        keep.append((module, trainer))
        steppers[label] = (lambda m, t: (lambda: t.training_step(m, batch, 0)))(module, trainer)
    for _ in range(max(2, warmup)):
        for f in steppers.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in steppers}
    for start in range(0, n_steps, block):
        for label, f in steppers.items():
            n = min(block, n_steps - start)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            ev[0].record()
            for i in range(n):
                f()
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[label] += [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]
    doc = {k: stats(ts, "ms", 3) for k, ts in times.items()}
    doc["mim_minus_reg_full_rows_ms"] = round(doc["mim"]["median_ms"] - doc["reg_full_rows"]["median_ms"], 3)
    # the three decoder products: 2 * M * P * D flops each
    doc["decoder_products_gflop"] = round(3 * 2 * B * (N + 1) * P * D / 1e9, 2)
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mim_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, HERE)
    import torch
    from vit_amd import build as vb

    if not torch.cuda.is_available():
        raise SystemExit("mim_bench needs an MI355X: there is nothing to time without one")
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup, "steps_per_variant": a.steps,
           "source_stamp": vb.source_stamp()[:16], "workload": "vit_b16_224", "batch": B, "precision": "bf16-mixed",
           "mask_ratio": RATIO, "span": SPAN}
    doc["kernels"] = kernels(a.runs, a.warmup)
    doc["steps"] = steps(torch, a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc["kernels"]:
        print(json.dumps(r))
    print(json.dumps(doc["steps"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
