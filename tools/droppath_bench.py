"""What stochastic depth costs: the path forms of the two LayerNorm passes beside their plain forms, and one training step.

    python tools/droppath_bench.py [--runs 30] [--warmup 5] [--steps 12] [--out profiles/droppath_bench.json]

One process, hipEvents around single launches, every shape warmed up first.  Per shape (ViT-B: 256 x 197 rows, D = 768; ViT-L:
32 x 577 rows, D = 1024) and per pass (forward with the residual sum; fused backward, hidden dropout 0.1) a round launches the
plain form and then the path form at rate 0.1, so both see the same minutes of a shared box.  Reported per pair: the medians,
the plain form's spread (max - min and the 10 % .. 90 % width over the rounds), the difference of the medians, and whether the
path form is within plain + that 10 % .. 90 % width.  The path form adds scalar work per row and skips the delta rows of
dropped samples (forward: about rate x a third of the pass's reads).

`--steps N` (0 = skip): N eager ViT-B training steps (B = 256, bf16-mixed, forward + backward + AdamW) at rate 0 and N at rate
0.1, in alternating blocks of the same process and model (`cfg.drop_path_rate` is read on every forward); medians and the
spread of the rate-0 steps."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"vit_b16_224": (256, 197, 768), "vit_l16_384": (32, 577, 1024)}
RATE, SEED, SITE, DSITE = 0.1, 0x1234567, 4 + 4 * 7, 1 + 4 * 7 + 2


def spread(ts):
    s = sorted(ts)
    return s[-1] - s[0], s[int(0.9 * (len(s) - 1))] - s[int(0.1 * (len(s) - 1))]


def time_pair(torch, plain, path, runs, warmup):
    for _ in range(max(1, warmup)):
        plain(); path()
    torch.cuda.synchronize()
    tp, tq = [], []
    for _ in range(runs):
        for f, acc in ((plain, tp), (path, tq)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3)
    mp, mq = statistics.median(tp), statistics.median(tq)
    full, mid = spread(tp)
    return {"plain_us": round(mp, 1), "path_us": round(mq, 1), "plain_min_us": round(min(tp), 1), "plain_max_us": round(max(tp), 1),
            "plain_spread_us": round(full, 1), "plain_p10_p90_us": round(mid, 1), "path_min_us": round(min(tq), 1),
            "path_max_us": round(max(tq), 1), "path_minus_plain_us": round(mq - mp, 1), "within_plain_spread": bool(mq <= mp + mid)}


def kernels(runs, warmup):
    import torch
    import vit_amd.functional as vf

    dev = torch.device("cuda", 0)
    rows_out = []
    for name, (B, T, D) in SHAPES.items():
        M = B * T
        x, delta = torch.randn(M, D, device=dev), torch.randn(M, D, device=dev).to(torch.bfloat16)
        g, b = torch.randn(D, device=dev) * 0.1 + 1, torch.randn(D, device=dev) * 0.1
        xsum, y = torch.empty(M, D, device=dev), torch.empty(M, D, device=dev, dtype=torch.bfloat16)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        path = (RATE, SITE, T, 0)
        rows_out.append({"shape": name, "rows": M, "D": D, "pass": "forward_residual", "rate": RATE, **time_pair(
            torch,
            lambda: vf.layernorm_fwd_residual(x, delta, xsum, g, b, 1e-12, out=y, mean=mean, rstd=rstd),
            lambda: vf.layernorm_fwd_residual_path(x, delta, xsum, g, b, 1e-12, path, SEED, out=y, mean=mean, rstd=rstd),
            runs, warmup)})
        dy, dres = torch.randn(M, D, device=dev).to(torch.bfloat16), torch.randn(M, D, device=dev)
        dx, dyn = torch.empty(M, D, device=dev), torch.empty(M, D, device=dev, dtype=torch.bfloat16)
        dg, db, dbias = (torch.empty(D, device=dev) for _ in range(3))
        drop = (0.1, SEED, DSITE)
        rows_out.append({"shape": name, "rows": M, "D": D, "pass": "backward_fused", "rate": RATE, **time_pair(
            torch,
            lambda: vf.layernorm_bwd_rows(dy, xsum, g, mean, rstd, dres, dx, dg, db, dyn=dyn, dbias=dbias, dropout=drop),
            lambda: vf.layernorm_bwd_path(dy, xsum, g, mean, rstd, dres, dx, dg, db, dyn, dbias, path, dropout=drop),
            runs, warmup)})
    return rows_out


def train_steps(steps, warmup):
    import torch
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    dev = torch.device("cuda", 0)
    L, P, D, layers, heads, B = 50176, 256, 768, 12, 12, 256
    config = {"model": dict(name="vit", task_type="reg", image_size=L, patch_size=P, hidden_size=D, num_hidden_layers=layers,
                            num_attention_heads=heads, stride_size=P, proj_fn="SW"),
              "train": dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=False), "loss": {"name": "mae"},
              "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0}}
    seed_everything(42)
    module = ViTLModule(config=config)
    trainer = Trainer(config["train"], device=dev, verbose=False)
    trainer._setup(module)
    module.train()
    g = torch.Generator(device="cpu").manual_seed(1234)
    batch = tuple(t.to(dev) for t in (torch.randn((B, L), generator=g), 0.1 * torch.randn((B, L), generator=g).abs(),
                                      torch.rand((B,), generator=g)))
    cfg = module.model.engine.cfg
    times = {0.0: [], RATE: []}
    for i in range(max(2, warmup)):
        for rate in times:
            cfg.drop_path_rate = rate
            trainer.training_step(module, batch, i)
    torch.cuda.synchronize()
    block = 4
    for start in range(0, steps, block):
        for rate, acc in times.items():
            cfg.drop_path_rate = rate
            n = min(block, steps - start)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            ev[0].record()
            for i in range(n):
                trainer.training_step(module, batch, start + i)
                ev[i + 1].record()
            torch.cuda.synchronize()
            acc += [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]
    cfg.drop_path_rate = 0.0
    m0, m1 = statistics.median(times[0.0]), statistics.median(times[RATE])
    full, mid = spread(times[0.0])
    return {"workload": "vit_b16_224", "batch": B, "precision": "bf16-mixed", "mode": "eager", "steps_per_rate": steps,
            "rate0_ms": round(m0, 3), "rate0_min_ms": round(min(times[0.0]), 3), "rate0_max_ms": round(max(times[0.0]), 3),
            "rate0_p10_p90_ms": round(mid, 3), "rate": RATE, "rate_ms": round(m1, 3), "rate_min_ms": round(min(times[RATE]), 3),
            "rate_max_ms": round(max(times[RATE]), 3), "rate_minus_rate0_ms": round(m1 - m0, 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "droppath_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, HERE)
    import torch
    from vit_amd import build as vb

    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup, "source_stamp": vb.source_stamp()[:16],
           "kernels": kernels(a.runs, a.warmup)}
    if a.steps > 0:
        doc["train_step"] = train_steps(a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc["kernels"]:
        print(f"{r['shape']:12s} {r['pass']:17s} plain {r['plain_us']:7.1f} us [{r['plain_min_us']:.1f} .. {r['plain_max_us']:.1f}]  "
              f"path {r['path_us']:7.1f} us  diff {r['path_minus_plain_us']:+.1f} us  p10-p90 {r['plain_p10_p90_us']:.1f} us  "
              f"within: {r['within_plain_spread']}")
    if "train_step" in doc:
        print(json.dumps(doc["train_step"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
