"""What the weight-averaging kernels reach, beside the AdamW step they run behind.

    python tools/ema_bench.py [--runs 30] [--warmup 5] [--out profiles/ema_bench.json]

One process times, interleaved on the same buffers at ViT-B's parameter count (n = 85 254 912, f32 master weights with the
bf16 shadow), with hipEvents around single launches:

    vit_adamw_step            30 B per parameter (p, g, m, v read; p, m, v, shadow written) -- untouched by the averaging, the yardstick
    vit_ema_update            12 B per parameter (p, ema read; ema written), w = 1 - 0.999
    vit_ema_update, w = 1      8 B per parameter (the first update: a copy; ema is not read)
    vit_ema_update from cell  12 B per parameter, the weight read from device memory (the captured step's form)
    vit_ema_swap              18 B per parameter (p, ema read and written; shadow written)

The figure per kernel is the median over `--runs` rounds (each round launches every kernel once, in turn, so all of them see
the same minutes of a shared box); min / max is the spread to read it against.  `ratio_to_adamw` is achieved bytes/s over
vit_adamw_step's in the same run: the averaging kernels are the same kind of stream and are expected at >= 0.9 of it."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_N = 85_254_912


def measure(runs: int, warmup: int):
    import torch
    import vit_amd.functional as vf
    from vit_amd import build as vb

    dev = torch.device("cuda", 0)
    n = KERNEL_N
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ema = torch.randn(n, device=dev)
    pb = torch.empty(n, device=dev, dtype=torch.bfloat16)
    sq = torch.ones(1, device=dev)
    cell = torch.zeros(1, 4, device=dev)
    w = 1.0 - 0.999
    vf.ema_weight_write(cell, w)
    calls = {
        "vit_adamw_step": (30, lambda: vf.adamw_step(p, g, m, v, pb, lr=1e-3, weight_decay=0.01, step=3, sqnorm=sq, max_norm=0.5)),
        "vit_ema_update": (12, lambda: vf.ema_update(ema, p, w)),
        "vit_ema_update (w = 1: copy)": (8, lambda: vf.ema_update(ema, p, 1.0)),
        "vit_ema_update (weight_dev)": (12, lambda: vf.ema_update(ema, p, weight_dev=cell)),
        "vit_ema_swap": (18, lambda: vf.ema_swap(p, ema, pb)),
    }
    for _ in range(max(1, warmup)):
        for _, f in calls.values():
            f()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(runs):
        for name, (_, f) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    rows = []
    for name, (nbytes, _) in calls.items():
        t = statistics.median(times[name])
        rows.append({"kernel": name, "n": n, "bytes_per_param": nbytes, "us": round(t, 1), "us_min": round(min(times[name]), 1),
                     "us_max": round(max(times[name]), 1), "bytes_per_s": round(n * nbytes / (t * 1e-6)),
                     "gb_per_s": round(n * nbytes / t / 1e3, 1)})
    base = rows[0]["bytes_per_s"]
    for r in rows:
        r["ratio_to_adamw"] = round(r["bytes_per_s"] / base, 3)
    return {"device": torch.cuda.get_device_name(0), "runs": runs, "warmup": warmup, "source_stamp": vb.source_stamp()[:16],
            "kernels": rows}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ema_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, HERE)
    doc = measure(a.runs, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc["kernels"]:
        print(f"{r['kernel']:32s} {r['us']:8.1f} us  [{r['us_min']:.1f} .. {r['us_max']:.1f}]  {r['gb_per_s']:8.1f} GB/s  "
              f"x{r['ratio_to_adamw']:.3f} of adamw")
    return 0


if __name__ == "__main__":
    sys.exit(main())
