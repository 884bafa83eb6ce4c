"""What register tokens cost: the register embedding kernels beside the existing entry points at the same sequence length, the
ViT-B training step with 4 registers beside the step without, and (optionally) bench.py of this tree beside a parent tree's.

    python tools/registers_bench.py [--runs 30] [--warmup 3] [--steps 40] [--parent DIR] [--bench-rounds 3]
                                    [--out profiles/registers_bench.json]

One process, hipEvents, every shape warmed up first, medians with min / max and the 10 % .. 90 % width; the variants of a
comparison alternate within the process, so both see the same minutes of a shared box.  Each expectation is stated here, before
the run, and the output records whether it `holds`:
 1. Kernels (B = 256, D = 768, T = 201, dropout 0.1, learned positions; dpatch bf16): vit_embed_finish_reg / _bwd at R = 4
    (N = 196) beside vit_embed_finish / _bwd at the same T (N = 200) -- the existing entry points, not the code under test --
    and, with a mask of ratio 0.6 in blocks of 4, beside vit_embed_finish_masked / _bwd.  Expectation: no slower beyond the
    run-to-run spread (median <= the twin's median + the wider p10-p90 of the two): they move the same bytes.
 2. Eager step (ViT-B/16 geometry, B = 256, bf16-mixed, forward + backward + AdamW) with R = 4 beside R = 0, in alternating
    blocks of 4 steps.  Expectation: the ratio of the medians is about 201 / 197 = 1.0203 -- every B * T-scaled kernel grows by
    that much and no tile count changes (B * T = 51456 = 201 tiles of 256 rows against 197).  `holds` = the measured ratio lies
    within 201 / 197 +- the relative spread (the wider p10-p90 over its median).  With RoPE the R = 4 step would also trade the
    QKV projection's rotating epilogue for a vit_rope_qk pass; this step has no position encoding, like bench.py's.
 3. `--parent DIR` (a built checkout of the parent commit): `bench.py --gpus 1` of this tree and of DIR, each run a fresh child
    process, alternating, `--bench-rounds` times each.  Expectation: equal within the spread (|difference of the medians of
    ms_per_step| <= the wider min-max range of the two): 0 registers cost nothing.  Without --parent it is recorded as not
    measured.
Not measured by this tool: a captured step's time, multi-GPU runs, any accuracy effect on real spectra."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, P, D, LAYERS, HEADS, N, R = 256, 50176, 256, 768, 12, 12, 196, 4
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
    from vit_amd.config import mim_blocks

    dev = torch.device("cuda", 0)
    T = 1 + R + N  # 201; the twins run the same T with N + R patches
    i32, bf = torch.int32, torch.bfloat16

    def block_mask(n):
        nb, kb = mim_blocks(n, SPAN, RATIO)
        keep, slot = torch.empty(B, kb, dtype=i32, device=dev), torch.empty(B, nb, dtype=i32, device=dev)
        mask = torch.empty(B, n, dtype=i32, device=dev)
        vf.patch_select(B, nb, kb, SEED, 49, keep, slot)
        return vf.mim_mask(slot, SPAN, mask)

    mask_r, mask_t = block_mask(N), block_mask(N + R)
    tok, cls, reg, mtok = torch.randn(B, T, D, device=dev), torch.randn(D, device=dev), torch.randn(R, D, device=dev), torch.randn(D, device=dev)
    pos_r, pos_t = torch.randn(1 + N, D, device=dev), torch.randn(T, D, device=dev)
    dcls, dreg, dmt = torch.empty(D, device=dev), torch.empty(R, D, device=dev), torch.empty(D, device=dev)
    dpos_r, dpos_t = torch.empty(1 + N, D, device=dev), torch.empty(T, D, device=dev)
    dpa_r, dpa_t = torch.empty(B * N, D, dtype=bf, device=dev), torch.empty(B * (N + R), D, dtype=bf, device=dev)
    drop = (0.1, SEED, 0)
    rows = []
    for name, twin, ours in (
            ("embed_finish", lambda: vf.embed_finish(tok, cls, pos_t, dropout=drop),
             lambda: vf.embed_finish_reg(tok, R, cls, reg, pos_r, dropout=drop)),
            ("embed_finish_bwd", lambda: vf.embed_finish_bwd(tok, dcls, dpos_t, dropout=drop, dpatch=dpa_t),
             lambda: vf.embed_finish_reg_bwd(tok, R, dcls, dreg, dpos_r, dropout=drop, dpatch=dpa_r)),
            ("embed_finish_masked", lambda: vf.embed_finish_masked(tok, cls, mask_t, mtok, pos_t, dropout=drop),
             lambda: vf.embed_finish_reg(tok, R, cls, reg, pos_r, mask_r, mtok, dropout=drop)),
            ("embed_finish_masked_bwd", lambda: vf.embed_finish_masked_bwd(tok, mask_t, dcls, dmt, dpos_t, dropout=drop, dpatch=dpa_t),
             lambda: vf.embed_finish_reg_bwd(tok, R, dcls, dreg, dpos_r, mask_r, dmt, dropout=drop, dpatch=dpa_r))):
        tt, to = time_calls(torch, (twin, ours), runs, warmup)
        st, so = stats(tt, "us", 1), stats(to, "us", 1)
        rows.append({"kernel": name, "rows": B * T, **{"twin_" + k: v for k, v in st.items()}, **{"reg_" + k: v for k, v in so.items()},
                     "expectation": "reg median <= twin median + the wider p10-p90",
                     "holds": bool(so["median_us"] <= st["median_us"] + max(st["p10_p90_us"], so["p10_p90_us"]))})
    return rows


def make_module(torch, registers):
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    model = dict(name="vit", task_type="reg", image_size=L, patch_size=P, hidden_size=D, num_hidden_layers=LAYERS,
                 num_attention_heads=HEADS, stride_size=P, proj_fn="SW", num_register_tokens=registers)
    config = {"model": model, "train": dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=False), "loss": {"name": "mae"},
              "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0}}
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
    for label, registers in (("registers_0", 0), ("registers_4", R)):
        module, trainer = make_module(torch, registers)
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
    a, b = doc["registers_0"], doc["registers_4"]
    ratio, expected = b["median_ms"] / a["median_ms"], (1 + R + N) / (1 + N)
    spread = max(a["p10_p90_ms"] / a["median_ms"], b["p10_p90_ms"] / b["median_ms"])
    doc.update(ratio=round(ratio, 4), expected_ratio=round(expected, 4), relative_spread=round(spread, 4),
               expectation="ratio within 201 / 197 +- the wider relative p10-p90", holds=bool(abs(ratio - expected) <= spread))
    return doc


def bench_against(parent, rounds, bench_steps, bench_warmup):
    """bench.py of this tree and of `parent`, alternating, each run a fresh child process; its one JSON line per run."""
    args = ["--gpus", "1", "--steps", str(bench_steps), "--warmup", str(bench_warmup), "--no-cpu-baseline", "--no-secondary",
            "--no-input-probe", "--no-kernel-timing"]
    runs = {"this": [], "parent": []}
    for _ in range(rounds):
        for label, root in (("parent", parent), ("this", HERE)):
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *args], cwd=root, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"bench.py failed in {root} (exit {r.returncode}):\n{r.stderr[-2000:]}")
            line = next(ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{"))
            runs[label].append(json.loads(line)["ms_per_step"])
    doc = {k: {"ms_per_step": v, "median_ms": round(statistics.median(v), 3), "range_ms": round(max(v) - min(v), 3)}
           for k, v in runs.items()}
    diff = doc["this"]["median_ms"] - doc["parent"]["median_ms"]
    doc.update(command="bench.py " + " ".join(args), this_minus_parent_ms=round(diff, 3),
               expectation="|difference of the medians| <= the wider min-max range",
               holds=bool(abs(diff) <= max(doc["this"]["range_ms"], doc["parent"]["range_ms"])))
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py of both trees, alternating")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "registers_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, HERE)
    import torch
    from vit_amd import build as vb

    if not torch.cuda.is_available():
        raise SystemExit("registers_bench needs an MI355X: there is nothing to time without one")
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup, "steps_per_variant": a.steps,
           "source_stamp": vb.source_stamp()[:16], "workload": "vit_b16_224", "batch": B, "precision": "bf16-mixed", "registers": R,
           "not_measured": ["a captured step's time", "multi-GPU runs", "any accuracy effect on real spectra"]}
    # the child processes of (3) run first, while this process holds no GPU memory
    if a.parent:
        doc["bench_against_parent"] = bench_against(os.path.abspath(a.parent), a.bench_rounds, a.bench_steps, a.bench_warmup)
    else:
        doc["bench_against_parent"] = "not measured (no --parent)"
        doc["not_measured"].append("bench.py against the parent commit")
    doc["kernels"] = kernels(a.runs, a.warmup)
    doc["steps"] = steps(torch, a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in doc["kernels"]:
        print(json.dumps(r))
    print(json.dumps(doc["steps"]))
    print(json.dumps(doc["bench_against_parent"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
