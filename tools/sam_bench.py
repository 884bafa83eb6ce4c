"""What sharpness-aware minimisation costs: its three kernels beside the weight-averaging kernels that move the same bytes, and the
ViT-B two-pass training step beside the plain step, eager and captured.

    python tools/sam_bench.py [--runs 30] [--warmup 3] [--steps 24] [--out profiles/sam_bench.json]

One process, hipEvents, every shape warmed up first, medians with min / max and the 10 % .. 90 % width; variants alternate within
the process, so they see the same minutes of a shared box.
Kernels (the 85.3 M trainable elements of ViT-B/16's flat buffer, f32 + bf16 shadow):
  vit_sam_ascend (reads p and g, writes backup, p and the shadow: 16 (+2) B per parameter) against vit_ema_swap over the same
    buffers, which moves the same bytes.  Expectation: no slower beyond the run-to-run spread.
  vit_sam_descend (8 (+2) B per parameter) against vit_ema_update with w = 0.1 (12 B per parameter).  Expectation: no slower.
  vit_sam_sqnorm, plain and adaptive (4 / 8 B per parameter), reported beside them.
Steps: ViT-B/16 geometry, B = 256, bf16-mixed, forward + backward + clip + AdamW, in alternating blocks of 4 steps: the plain and
the `train.sam_rho` step, eager and captured (`train.hip_graph`).  Expectation, each form: the two-pass step takes no more than
twice the plain step of the same run plus the three launches above (forward and backward double, the optimizer step does not),
beyond the steps' spread.  Every expectation is written as holds / fails, whatever the outcome."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, P, D, LAYERS, HEADS = 256, 50176, 256, 768, 12, 12
RHO = 0.05


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


def verdict(ok: bool) -> str:
    return "holds" if ok else "fails"


def kernels(n, runs, warmup):
    import torch
    import vit_amd.functional as vf

    dev = torch.device("cuda", 0)
    p = 0.02 * torch.randn(n, device=dev)
    g = 1e-3 * torch.randn(n, device=dev)
    other, shadow = p.clone(), torch.empty(n, dtype=torch.bfloat16, device=dev)
    sq = vf.sam_sqnorm(g)
    pairs = (
        ("vit_sam_ascend", 18, lambda: vf.sam_ascend(p, g, other, shadow, RHO, sq),
         "vit_ema_swap", 18, lambda: vf.ema_swap(p, other, shadow)),
        ("vit_sam_descend", 10, lambda: vf.sam_descend(p, other, shadow),
         "vit_ema_update(w=0.1)", 12, lambda: vf.ema_update(other, p, 0.1)),
    )
    rows = []
    for name, nbytes, mine, yard_name, ybytes, yard in pairs:
        ty, tm = time_calls(torch, (yard, mine), runs, warmup)
        sy, sm = stats(ty, "us", 1), stats(tm, "us", 1)
        ok = sm["median_us"] <= sy["median_us"] + max(sy["p10_p90_us"], sm["p10_p90_us"])
        rows.append({"kernel": name, "n": n, "bytes_per_parameter": nbytes, **sm,
                     "achieved_TBps": round(n * nbytes / (sm["median_us"] * 1e-6) / 1e12, 2),
                     "yardstick": yard_name, "yardstick_bytes_per_parameter": ybytes,
                     **{"yardstick_" + k: v for k, v in sy.items()},
                     "expectation": f"no slower than {yard_name} beyond the spread", "expectation_verdict": verdict(ok)})
        p.copy_(other)  # whatever the rounds left: finite weights for the next pair
    for name, nbytes, f in (("vit_sam_sqnorm", 4, lambda: vf.sam_sqnorm(g, out=sq)),
                            ("vit_sam_sqnorm(adaptive)", 8, lambda: vf.sam_sqnorm(g, p, adaptive=True, out=sq))):
        (t,) = time_calls(torch, (f,), runs, warmup)
        sm = stats(t, "us", 1)
        rows.append({"kernel": name, "n": n, "bytes_per_parameter": nbytes, **sm,
                     "achieved_TBps": round(n * nbytes / (sm["median_us"] * 1e-6) / 1e12, 2)})
    return rows


def make_module(torch, sam: bool, graph: bool):
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    model = dict(name="vit", task_type="reg", image_size=L, patch_size=P, hidden_size=D, num_hidden_layers=LAYERS,
                 num_attention_heads=HEADS, stride_size=P, proj_fn="SW")
    train = dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=graph)  # train.grad_clip: the default 0.5
    if sam:
        train["sam_rho"] = RHO
    config = {"model": model, "train": train, "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-4},
              "data": {"param": "log_g"}, "noise": {"noise_level": 0}}
    seed_everything(42)
    module = ViTLModule(config=config)
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.train()
    return module, trainer


def steps(torch, n_steps, warmup, block=4):
    g = torch.Generator(device="cpu").manual_seed(1234)
    batch = tuple(t.to("cuda:0") for t in (torch.randn((B, L), generator=g), 0.1 * torch.randn((B, L), generator=g).abs(),
                                          torch.rand((B,), generator=g)))
    keep, steppers = [], {}
    for label, sam, graph in (("plain_eager", False, False), ("sam_eager", True, False), ("plain_graph", False, True),
                              ("sam_graph", True, True)):
        module, trainer = make_module(torch, sam, graph)
        keep.append((module, trainer))
        steppers[label] = (lambda m, t: (lambda: t.training_step(m, batch, 0)))(module, trainer)
    for _ in range(max(2, warmup)):
        for f in steppers.values():
            f()
    torch.cuda.synchronize()
    for (module, trainer), label in zip(keep, steppers):
        if label.endswith("_graph") and not trainer.use_graph:
            raise SystemExit(f"sam_bench: the {label} step fell back to eager launches; nothing to report for it")
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
    return {k: stats(ts, "ms", 3) for k, ts in times.items()}, keep[0][0].model.engine.layout.n_trainable


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sam_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, HERE)
    import torch
    from vit_amd import build as vb

    if not torch.cuda.is_available():
        raise SystemExit("sam_bench needs an MI355X: there is nothing to time without one")
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup, "steps_per_variant": a.steps,
           "source_stamp": vb.source_stamp()[:16], "workload": "vit_b16_224", "batch": B, "precision": "bf16-mixed", "rho": RHO}
    step_doc, n = steps(torch, a.steps, a.warmup)
    torch.cuda.empty_cache()
    doc["kernels"] = kernels(n, a.runs, a.warmup)
    by = {r["kernel"]: r for r in doc["kernels"]}
    three = (by["vit_sam_sqnorm"]["median_us"] + by["vit_sam_ascend"]["median_us"] + by["vit_sam_descend"]["median_us"]) / 1e3
    step_doc["three_launches_ms"] = round(three, 3)
    for form in ("eager", "graph"):
        plain, sam = step_doc[f"plain_{form}"], step_doc[f"sam_{form}"]
        bound = 2 * plain["median_ms"] + three
        step_doc[f"{form}_ratio"] = round(sam["median_ms"] / plain["median_ms"], 3)
        step_doc[f"{form}_bound_ms"] = round(bound, 3)
        step_doc[f"{form}_expectation"] = "sam step <= 2 x plain step + the three launches, beyond the spread"
        step_doc[f"{form}_expectation_verdict"] = verdict(sam["median_ms"] <= bound + max(plain["p10_p90_ms"], sam["p10_p90_ms"]))
    doc["steps"] = step_doc
    doc["not_measured"] = ["multi-GPU runs", "accuracy on real spectra"]
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
