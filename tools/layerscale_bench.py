"""What LayerScale costs: its two streaming kernels beside vit_ema_update, and one training step with the feature off and on.

    python tools/layerscale_bench.py [--runs 30] [--warmup 5] [--pairs 3] [--steps 6] [--out profiles/layerscale_bench.json]

One process, hipEvents, every launch warmed up first.  Per table (ViT-B: 12 x {768 x 768, 768 x 3072}; ViT-L: 24 x {1024 x 1024,
1024 x 4096}): the median time and bytes/s of `vit_layer_scale_fold` (one launch over the 2L entries, bf16 out), of
`vit_layer_scale_grad` as the engine issues it (L launches of one layer's two entries, timed together: the step's whole
unfold), and of `vit_ema_update` over the same number of parameters, the yardstick for bytes/s.  A round runs the three one
after the other, so they see the same minutes of a shared box.  Bytes are what the kernels must move: 4 + 2 per weight for the
fold, 12 for the overwriting unfold, 12 for the average's update.

`--pairs N` (0 = skip): the trainer's eager step at ViT-B, B = 256, bf16-mixed (forward + backward + AdamW), `--steps` steps
with the feature off and as many with it on (`layer_scale_init: 1e-5`), alternating, N pairs of blocks, in this process: two
models, since the feature changes the parameter layout.  Reported: the medians, the spread of the steps with the feature off,
the difference, and the difference as a share of the step with the feature off."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = {"vit_b": (12, 768), "vit_l": (24, 1024)}


def spread(ts):
    s = sorted(ts)
    return s[-1] - s[0], s[int(0.9 * (len(s) - 1))] - s[int(0.1 * (len(s) - 1))]


def timed(torch, f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); f(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def kernels(runs, warmup):
    import torch
    import vit_amd.functional as vf

    dev = torch.device("cuda", 0)
    out = []
    for name, (L, D) in TABLES.items():
        nw = 5 * D * D  # weights per layer: D x D and D x 4D
        entries = []
        for _ in range(L):
            for K in (D, 4 * D):
                entries.append(dict(W=torch.randn(D, K, device=dev), b=torch.randn(D, device=dev), lam=torch.rand(D, device=dev) + 0.5,
                                    Wf=torch.empty(D, K, device=dev, dtype=torch.bfloat16), bf=torch.empty(D, device=dev),
                                    dW_raw=torch.randn(D, K, device=dev), db_raw=torch.randn(D, device=dev),
                                    dW=torch.empty(D, K, device=dev), db=torch.empty(D, device=dev), dlam=torch.empty(D, device=dev)))
        tab = vf.layer_scale_table(entries, dev)
        n = L * nw
        ema, p = torch.zeros(n, device=dev), torch.randn(n, device=dev)
        passes = {
            "fold": (lambda: vf.layer_scale_fold(tab, torch.bfloat16), L * (6 * nw + 2 * 12 * D), 1),
            "grad": (lambda: [vf.layer_scale_grad(tab, False, first=2 * i, count=2) for i in range(L)], L * (12 * nw + 2 * 24 * D), L),
            "ema_update": (lambda: vf.ema_update(ema, p, 0.001), 12 * n, 1),
        }
        for _ in range(max(1, warmup)):
            for f, _, _ in passes.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in passes}
        for _ in range(runs):
            for k, (f, _, _) in passes.items():
                times[k].append(timed(torch, f))
        for k, (_, nbytes, launches) in passes.items():
            med = statistics.median(times[k])
            full, mid = spread(times[k])
            out.append({"table": name, "layers": L, "D": D, "parameters": n, "pass": k, "launches": launches, "bytes": nbytes,
                        "median_us": round(med, 1), "min_us": round(min(times[k]), 1), "max_us": round(max(times[k]), 1),
                        "p10_p90_us": round(mid, 1), "tb_per_s": round(nbytes / med * 1e-6, 3)})
    return out


def train_steps(pairs, steps, warmup):
    import torch
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    dev = torch.device("cuda", 0)
    Lsig, P, D, layers, heads, B = 50176, 256, 768, 12, 12, 256
    g = torch.Generator(device="cpu").manual_seed(1234)
    batch = tuple(t.to(dev) for t in (torch.randn((B, Lsig), generator=g), 0.1 * torch.randn((B, Lsig), generator=g).abs(),
                                      torch.rand((B,), generator=g)))
    runs = {}
    for key, init in (("off", None), ("on", 1e-5)):
        model = dict(name="vit", task_type="reg", image_size=Lsig, patch_size=P, hidden_size=D, num_hidden_layers=layers,
                     num_attention_heads=heads, stride_size=P, proj_fn="SW")
        if init is not None:
            model["layer_scale_init"] = init
        config = {"model": model, "train": dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=False), "loss": {"name": "mae"},
                  "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0}}
        seed_everything(42)
        module = ViTLModule(config=config)
        trainer = Trainer(config["train"], device=dev, verbose=False)
        trainer._setup(module)
        module.train()
        for i in range(max(2, warmup)):
            trainer.training_step(module, batch, i)
        runs[key] = (module, trainer, [])
    torch.cuda.synchronize()
    for _ in range(pairs):
        for module, trainer, acc in runs.values():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            ev[0].record()
            for i in range(steps):
                trainer.training_step(module, batch, i)
                ev[i + 1].record()
            torch.cuda.synchronize()
            acc += [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    off, on = runs["off"][2], runs["on"][2]
    m0, m1 = statistics.median(off), statistics.median(on)
    full, mid = spread(off)
    return {"workload": "vit_b16_224", "batch": B, "precision": "bf16-mixed", "mode": "eager", "pairs": pairs, "steps_per_block": steps,
            "off_ms": round(m0, 3), "off_min_ms": round(min(off), 3), "off_max_ms": round(max(off), 3), "off_p10_p90_ms": round(mid, 3),
            "on_ms": round(m1, 3), "on_min_ms": round(min(on), 3), "on_max_ms": round(max(on), 3),
            "on_minus_off_ms": round(m1 - m0, 3), "on_minus_off_percent_of_off": round(100 * (m1 - m0) / m0, 2)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "layerscale_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    if 0 < a.pairs < 3:
        ap.error("--pairs must be 0 or at least 3")
    sys.path.insert(0, HERE)
    import torch
    from vit_amd import build as vb

    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup, "source_stamp": vb.source_stamp()[:16],
           "kernels": kernels(a.runs, a.warmup)}
    if a.pairs > 0:
        doc["train_step"] = train_steps(a.pairs, a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc["kernels"]:
        print(f"{r['table']:6s} {r['pass']:11s} {r['median_us']:8.1f} us [{r['min_us']:.1f} .. {r['max_us']:.1f}]  "
              f"{r['bytes'] / 1e6:7.1f} MB  {r['tb_per_s']:.2f} TB/s  ({r['launches']} launch(es))")
    if "train_step" in doc:
        print(json.dumps(doc["train_step"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
