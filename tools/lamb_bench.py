"""What the fused LAMB step costs beside the fused AdamW step, and what each of its three passes reaches.

    python tools/lamb_bench.py [--rounds 9] [--reps 3] [--out profiles/lamb_bench.json]

One process, one GPU, the manner of tools/optim_bench.py's kernel rows: flat f32 buffers of ViT-B's trainable length (85.8 M
elements, its parameter layout with every tensor padded to 8), ViT-B's `no_decay: true` groups, the clip coefficient read
from a device cell, the bf16 shadow written.  Timed with hipEvents around `reps` back-to-back calls, all rows interleaved in
every round so that each sees the same minutes; the figure is the median over the rounds, min / max the spread.

    adamw table          vit_adamw_step_groups over the merged no-decay table (the kernel FusedAdamW launches; this change
                         does not touch it)                                                                        30 B / parameter
    lamb                 vit_lamb_step_groups over the per-parameter table: the three launches                     42 B
    lamb pass 1 / 2 / 3  one launch alone (the handle's measurement option "lamb_passes"): moments + partial norms 24 B,
                         ratios (reads the tile partials: 16 B per 4096 elements), apply 18 B

Bytes are what the algorithm must move per parameter (shadow included), so GB/s is comparable with the 5.8 - 6.0 TB/s the
project's streaming kernels reach.  The target this change set itself: lamb <= 1.4 x 1.10 x the same-run adamw time; the JSON
records the ratio and whether it is met.  Timing leaves the buffers changed; nothing here checks values (tests/test_lamb_gpu.py does)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

TARGET = 1.4 * 1.10


def _vitb_triples():
    """(offset, padded numel, group) of every trainable tensor of ViT-B under `no_decay: true` (group 0 decays), from the parameter
    layout alone -- no model is allocated."""
    from vit_amd.config import ViTConfig
    from vit_amd.engine import ParamLayout

    lay = ParamLayout(ViTConfig(task_type="reg", image_size=50176, patch_size=256, hidden_size=768, num_hidden_layers=12,
                                num_attention_heads=12, stride_size=256, num_labels=1))
    triples = []
    for name, (off, shape) in sorted(lay.entries.items(), key=lambda kv: kv[1][0]):
        if off < lay.n_trainable:
            skip = len(shape) <= 1 or name.endswith(("cls_token", "position_embeddings"))
            triples.append((off, (lay.numel(name) + 7) // 8 * 8, int(skip)))
    return triples


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lamb_bench.py times an MI355X; there is no GPU here and no fallback")
    import vit_amd.functional as vf

    dev = torch.device("cuda", 0)
    triples = _vitb_triples()
    n = triples[-1][0] + triples[-1][1]
    merged = vf.optim_group_tables(triples, 2, dev)
    per_param = vf.optim_param_tables(triples, 2, dev)
    for t in (merged, per_param):
        vf.optim_groups_write(t, [(1e-3, 0.05, 0.0), (1e-3, 0.0, 0.0)])
    p = torch.randn(n, device=dev) * 0.02
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = torch.empty(n, device=dev, dtype=torch.bfloat16)
    sq = torch.ones(1, device=dev)
    trust = torch.ones(per_param.n_segments, device=dev)
    handle = vf._h(p)
    tiles = sum((k + vf.LAMB_TILE - 1) // vf.LAMB_TILE for _, k, _ in triples)

    def adamw():
        vf.adamw_step_groups(p, g, m, v, pb, merged, step=3, sqnorm=sq, max_norm=0.5)

    def lamb(passes=7):
        def call():
            handle.set_option("lamb_passes", passes)
            try:
                vf.lamb_step_groups(p, g, m, v, pb, per_param, trust, step=3, sqnorm=sq, max_norm=0.5)
            finally:
                handle.set_option("lamb_passes", 7)
        return call

    # name -> (bytes moved per call, call)
    calls = {"adamw table (30 B)": (30 * n, adamw), "lamb (42 B)": (42 * n, lamb()),
             "lamb pass 1: moments + partial norms (24 B)": (24 * n, lamb(1)),
             "lamb pass 2: ratios": (16 * tiles + 4 * per_param.n_segments, lamb(2)),
             "lamb pass 3: apply (18 B)": (18 * n, lamb(4))}
    for _, f in calls.values():
        f(); f()
    torch.cuda.synchronize()
    ts = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, (_, f) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
    rows = []
    for name, (nbytes, _) in calls.items():
        us = statistics.median(ts[name])
        rows.append({"kernel": name, "n": n, "bytes": nbytes, "us": round(us, 1), "us_min": round(min(ts[name]), 1),
                     "us_max": round(max(ts[name]), 1), "gb_per_s": round(nbytes / us / 1e3, 1)})
        print(f"{name:46s} {us:8.1f} us [{min(ts[name]):.1f} .. {max(ts[name]):.1f}] = {rows[-1]['gb_per_s']:.0f} GB/s", flush=True)
    by = {r["kernel"]: r for r in rows}
    ratio = by["lamb (42 B)"]["us"] / by["adamw table (30 B)"]["us"]
    result = {"lamb_bench": {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "n": n,
                             "n_segments": per_param.n_segments, "n_segments_adamw": merged.n_segments, "tile": vf.LAMB_TILE,
                             "tiles": tiles, "kernels": rows, "lamb_over_adamw": round(ratio, 4), "target": round(TARGET, 4),
                             "target_met": bool(ratio <= TARGET)}}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
