"""What global average pooling costs: the two pooling kernels beside the parent's streaming kernels over the same bytes, and the
ViT-B `global_pool: avg` training step beside the `token` step on the same engine path.

    python tools/pool_bench.py [--runs 30] [--warmup 3] [--steps 40] [--out profiles/pool_bench.json]

One process, hipEvents, every shape warmed up first, medians with min / max and the 10 % .. 90 % width.
Kernels (B = 256, T = 197, D = 768, f32: 155 MB): a round launches the yardstick and then the pooling kernel, so both see the same
minutes of a shared box.  Forward: vit_token_pool_fwd reads x [B, T, D] once; the yardstick is vit_colsum over the same tensor as
[B * T, D], the library's reduction over the same bytes.  Backward: vit_token_pool_bwd writes dx [B, T, D] once and reads
[B, D]; the yardstick is torch's copy_ of a [B * T, D] f32 tensor (which reads and writes those bytes).  The expectation to
confirm: the pooling kernel is no slower than its yardstick beyond the width measured here (`within_spread`).  155 MB fits
the 256 MiB Infinity Cache, for every kernel of a round alike: the rates are what a step sees behind the final LayerNorm, which
has just written x, not DRAM rates.
Steps: ViT-B/16 geometry, B = 256, bf16-mixed, forward + backward + AdamW, eager, in alternating blocks of 4 steps: the `avg`
regression step and the `token` step with `cls_tail` off -- the same engine running the last layer over every row, which `avg`
extends by the two kernels above.  The `token` step with the CLS tail on (the benchmarked path) is timed in the same rounds: the
difference is the price of reading every row of the last layer."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, P, D, LAYERS, HEADS, N = 256, 50176, 256, 768, 12, 12, 196


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

    dev = torch.device("cuda", 0)
    T = N + 1
    x = torch.randn(B, T, D, device=dev)
    src = torch.randn(B * T, D, device=dev)
    pooled, sums, g = torch.empty(B, D, device=dev), torch.empty(D, device=dev), torch.randn(B, D, device=dev)
    dx = torch.empty(B, T, D, device=dev)
    nbytes = x.numel() * 4
    rows = []
    for name, yard_name, yard, mine, moved in (
            ("token_pool_fwd", "colsum", lambda: vf.colsum(x.view(B * T, D), out=sums), lambda: vf.token_pool_fwd(x, 1, out=pooled),
             nbytes + B * D * 4),
            ("token_pool_bwd", "copy_", lambda: dx.view(B * T, D).copy_(src), lambda: vf.token_pool_bwd(g, dx, 1),
             nbytes + B * D * 4)):
        ty, tm = time_calls(torch, (yard, mine), runs, warmup)
        sy, sm = stats(ty, "us", 1), stats(tm, "us", 1)
        rows.append({"kernel": name, "yardstick": yard_name, "B": B, "T": T, "D": D, "must_move_bytes": moved,
                     **{"yardstick_" + k: v for k, v in sy.items()}, **sm,
                     "achieved_TBps": round(moved / (sm["median_us"] * 1e-6) / 1e12, 2),
                     "within_spread": bool(sm["median_us"] <= sy["median_us"] + max(sy["p10_p90_us"], sm["p10_p90_us"]))})
    return rows


def make_module(torch, pool, tail=True):
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    model = dict(name="vit", task_type="reg", image_size=L, patch_size=P, hidden_size=D, num_hidden_layers=LAYERS,
                 num_attention_heads=HEADS, stride_size=P, proj_fn="SW", global_pool=pool)
    config = {"model": model, "train": dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=False), "loss": {"name": "mae"},
              "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0}}
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
    for label, pool, tail in (("token_full_rows", "token", False), ("avg", "avg", True), ("token_cls_tail", "token", True)):
        module, trainer = make_module(torch, pool, tail)
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
    doc["avg_minus_token_full_rows_ms"] = round(doc["avg"]["median_ms"] - doc["token_full_rows"]["median_ms"], 3)
    doc["token_full_rows_minus_cls_tail_ms"] = round(doc["token_full_rows"]["median_ms"] - doc["token_cls_tail"]["median_ms"], 3)
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pool_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, HERE)
    import torch
    from vit_amd import build as vb

    if not torch.cuda.is_available():
        raise SystemExit("pool_bench needs an MI355X: there is nothing to time without one")
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup, "steps_per_variant": a.steps,
           "source_stamp": vb.source_stamp()[:16], "workload": "vit_b16_224", "batch": B, "precision": "bf16-mixed"}
    doc["kernels"] = kernels(a.runs, a.warmup)
    doc["steps"] = steps(torch, a.steps, a.warmup)
    # the expectation for the step: avg - token_full_rows = the two kernels, within the steps' spread
    two = sum(r["median_us"] for r in doc["kernels"]) / 1e3
    spread = max(doc["steps"]["avg"]["p10_p90_ms"], doc["steps"]["token_full_rows"]["p10_p90_ms"])
    doc["steps"]["two_kernels_ms"] = round(two, 3)
    doc["steps"]["difference_is_the_two_kernels_within_spread"] = bool(
        abs(doc["steps"]["avg_minus_token_full_rows_ms"] - two) <= spread)
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
