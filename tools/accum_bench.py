"""What in-place gradient accumulation costs: one forward + backward in overwrite mode (every parameter's .grad is None, the
kernels store their gradients) against one in accumulate mode (the .grad views are kept, the kernels store old + new:
vit_handle_set_option "grad_accumulate"), in ONE process on the same model, batch and dropout stream.

    python tools/accum_bench.py [--steps 20] [--rounds 5] [--warmup 5] [--out FILE.json]

Shapes: C3 (ViT-B/16 geometry) at B = 256 and C1 at B = 64, bf16-mixed.  Timing: hipEvents around each forward + backward on
the compute stream; the two modes alternate in blocks of `--steps` (`--rounds` blocks each, after `--warmup` steps of each
mode), and the figure is the median over all steps of a mode; the per-block medians show the spread the difference has to be
read against.  The only traffic accumulate mode adds is the old value read in each final write (DESIGN.md section 2b sets the
measured difference beside that estimate and beside the three passes of a second buffer + add kernel)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(name: str, batch: int, dev):
    from oracle import refvit  # seeded weights / inputs only
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    rc = refvit.named_config(name)
    cfg = ViTConfig(task_type="reg", image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                    num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, stride_size=rc.stride_size)
    model = MyViT(cfg, loss_name="mae")
    model.set_precision("bf16-mixed")
    model.load_state_dict(refvit.make_state_dict(rc, 1))
    model.to(dev).train()
    flux, _, labels = refvit.make_inputs(rc, batch, 2)
    return model, flux.to(dev), labels.to(dev)


def timed_steps(model, x, y, n: int, accumulate: bool):
    """ms of each of n forward + backward passes (device events); overwrite mode drops the .grad views first, as
    zero_grad(set_to_none=True) does at the start of a step."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        if not accumulate:
            for p in model._param_list:
                p.grad = None
        a.record()
        model(x, labels=y).loss.backward()
        b.record()
    torch.cuda.synchronize()
    assert model.engine._accum is False
    return [a.elapsed_time(b) for a, b in ev]


def measure(name: str, batch: int, steps: int, rounds: int, warmup: int, dev):
    model, x, y = build(name, batch, dev)
    timed_steps(model, x, y, warmup, False)
    timed_steps(model, x, y, warmup, True)  # the first of these is an overwrite (no views yet); warm-up either way
    ms = {"overwrite": [], "accumulate": []}
    blocks = {"overwrite": [], "accumulate": []}
    for _ in range(rounds):
        for mode in ("overwrite", "accumulate"):
            if mode == "accumulate":  # make sure the views are held, outside the timed window
                model(x, labels=y).loss.backward()
            t = timed_steps(model, x, y, steps, mode == "accumulate")
            ms[mode] += t
            blocks[mode].append(round(statistics.median(t), 4))
    ow, acc = statistics.median(ms["overwrite"]), statistics.median(ms["accumulate"])
    n = model.engine.layout.n_trainable
    return {"config": name, "batch": batch, "precision": "bf16-mixed", "gradient_mbytes": round(4 * n / 1e6, 1),
            "overwrite_ms": round(ow, 4), "accumulate_ms": round(acc, 4), "difference_ms": round(acc - ow, 4),
            "block_medians_ms": blocks, "steps_per_mode": len(ms["overwrite"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench.py times kernels on an MI355X; there is no GPU here and no fallback")
    dev = torch.device("cuda", 0)
    results = []
    for name, batch in (("C3", 256), ("C1", 64)):
        r = measure(name, batch, args.steps, args.rounds, args.warmup, dev)
        results.append(r)
        print(f"{name} B={batch} bf16-mixed: forward + backward overwrite {r['overwrite_ms']:.3f} ms, accumulate "
              f"{r['accumulate_ms']:.3f} ms, difference {r['difference_ms']:+.3f} ms (gradient buffer {r['gradient_mbytes']} MB; "
              f"block medians overwrite {r['block_medians_ms']['overwrite']} accumulate {r['block_medians_ms']['accumulate']})",
              flush=True)
    line = json.dumps({"accum_bench": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
