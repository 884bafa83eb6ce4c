"""What the Mixup / CutMix kernels reach, beside the plain copy they replace, and the soft-target head losses beside hard CE.

    python tools/mix_bench.py [--runs 30] [--warmup 5] [--out profiles/mix_bench.json]

One process times, interleaved on the same buffers at ViT-B's input (B = 256 spectra of L = 50176 f32), with hipEvents around
single calls:

    Tensor.copy_                       2 x B x L x 4 bytes: the launch the copy form replaces (the captured step's input copy)
    vit_mix_signal, copy form          2 x B x L x 4 bytes whatever the plan holds: Mixup with a one-row plan and with a
                                       per-sample plan, CutMix with a span of L / 2
    vit_mix_signal, in place, Mixup    4 x L x 4 bytes per pair = 2 x B x L x 4
    vit_mix_plan_write                 1 and 256 rows (32 bytes a row, in kernel arguments)
    head loss forward + backward       B = 256, C = 1000, D = 768: VIT_LOSS_CE, VIT_LOSS_SOFT_CE, VIT_LOSS_BCE

The figure per call is the median over `--runs` rounds (each round makes every call once, in turn, so all of them see the same
minutes of a shared box); min / max is the spread to read it against.  `ratio_to_copy` is achieved bytes/s over Tensor.copy_'s
in the same run: the copy form moves exactly the copy's bytes, so the target is parity, with 10 % allowed for the plan lookup
and the two-row access pattern.  The losses are reported beside each other without a threshold."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L = 256, 50176
HEAD = dict(B=256, T=197, D=768, C=1000)


def measure(runs: int, warmup: int):
    import torch
    import vit_amd.functional as vf
    from vit_amd import _cabi
    from vit_amd import build as vb

    dev = torch.device("cuda", 0)
    x = torch.randn(B, L, device=dev)
    xin = torch.randn(B, L, device=dev)  # the in-place form's own buffer
    out = torch.empty_like(x)
    mix_row = (0.37, 0.63, 0, 0, 0.37, 0.63)
    cut_row = (1.0, 0.0, L // 4, L // 4 + L // 2, 0.5, 0.5)

    def plan_of(rows):
        plan = torch.zeros(len(rows) * vf.MIX_ROW_BYTES, dtype=torch.uint8, device=dev)
        vf.mix_plan_write(plan, rows)
        return plan

    p_mix1, p_mixB, p_cut1 = plan_of([mix_row]), plan_of([mix_row] * B), plan_of([cut_row])
    scratch = torch.zeros(B * vf.MIX_ROW_BYTES, dtype=torch.uint8, device=dev)
    nbytes = 2 * B * L * 4
    hb = HEAD
    last = torch.randn(hb["B"], hb["T"], hb["D"], device=dev)
    W, b = torch.randn(hb["C"], hb["D"], device=dev) * 0.02, torch.zeros(hb["C"], device=dev)
    y = torch.randint(0, hb["C"], (hb["B"],), device=dev)
    t = torch.softmax(torch.randn(hb["B"], hb["C"], device=dev), 1)
    dloss = torch.ones(1, device=dev)
    dlast, dW, db = torch.empty_like(last), torch.empty_like(W), torch.empty_like(b)

    def head(labels, kind):
        logits, _ = vf.head_loss_fwd(last, W, b, labels, kind)
        vf.head_loss_bwd(last, W, logits, labels, dloss, kind, dlast=dlast, dW=dW, db=db)

    calls = {
        "Tensor.copy_": (nbytes, lambda: out.copy_(x)),
        "vit_mix_signal copy, Mixup, one-row plan": (nbytes, lambda: vf.mix_signal(x, p_mix1, 1, out=out)),
        "vit_mix_signal copy, Mixup, per-sample plan": (nbytes, lambda: vf.mix_signal(x, p_mixB, B, out=out)),
        "vit_mix_signal copy, CutMix span L/2": (nbytes, lambda: vf.mix_signal(x, p_cut1, 1, out=out)),
        "vit_mix_signal in place, Mixup": (nbytes, lambda: vf.mix_signal(xin, p_mix1, 1, out=xin)),
        "vit_mix_plan_write, 1 row": (32, lambda: vf.mix_plan_write(scratch, [mix_row])),
        "vit_mix_plan_write, 256 rows": (32 * B, lambda: vf.mix_plan_write(scratch, [mix_row] * B)),
        "head loss fwd + bwd, VIT_LOSS_CE": (0, lambda: head(y, _cabi.LOSS_CE)),
        "head loss fwd + bwd, VIT_LOSS_SOFT_CE": (0, lambda: head(t, _cabi.LOSS_SOFT_CE)),
        "head loss fwd + bwd, VIT_LOSS_BCE": (0, lambda: head(t, _cabi.LOSS_BCE)),
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
    for name, (nb, _) in calls.items():
        us = statistics.median(times[name])
        row = {"call": name, "us": round(us, 1), "us_min": round(min(times[name]), 1), "us_max": round(max(times[name]), 1)}
        if nb >= nbytes:
            row.update(bytes=nb, gb_per_s=round(nb / us / 1e3, 1))
        rows.append(row)
    base = rows[0]["gb_per_s"]
    for r in rows:
        if "gb_per_s" in r:
            r["ratio_to_copy"] = round(r["gb_per_s"] / base, 3)
    return {"device": torch.cuda.get_device_name(0), "runs": runs, "warmup": warmup, "source_stamp": vb.source_stamp()[:16],
            "signal": {"B": B, "L": L}, "head": HEAD, "calls": rows}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mix_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, HERE)
    doc = measure(a.runs, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc["calls"]:
        rate = f"{r['gb_per_s']:8.1f} GB/s  x{r['ratio_to_copy']:.3f} of copy_" if "gb_per_s" in r else ""
        print(f"{r['call']:46s} {r['us']:9.1f} us  [{r['us_min']:.1f} .. {r['us_max']:.1f}]  {rate}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
