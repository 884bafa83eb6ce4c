"""What patch dropout costs and buys: the gather kernels beside their plain twins, the RoPE pass beside the rotating epilogue,
and ViT-B training steps at patch_drop_rate 0, 0.25 and 0.5, eager and captured.

    python tools/patchdrop_bench.py [--runs 30] [--warmup 3] [--steps 40] [--parent-root DIR] [--out profiles/patchdrop_bench.json]

One process, hipEvents, every shape warmed up first.
Kernels (B = 256, N = 196, K = 98, D = 768, P = 256): a round launches the plain form over all 196 patches and then the gather form
over the kept 98, so both see the same minutes of a shared box; the selection and the table gather have no twin and are timed
alone.  The gather forms move half the rows: their times are NOT expected to equal the plain forms'.
Steps: ViT-B/16 geometry, B = 256, bf16-mixed, forward + backward + AdamW.  One model per rate (the training arena is sized by the
token count, so one model switched between rates would time the allocator; a capture freezes K), eager and as one hipGraph each,
run in blocks of 4 steps with the three rates alternating.  Reported per rate: the median, min, max and the 10 % .. 90 % width.
RoPE: the same geometry with pos_encoding_type 'rope', eager: rate 0 rotates in the QKV projection's epilogue, a dropping step
by a vit_rope_qk pass behind it (and its inverse in the backward) over per-step gathered tables; that pass alone is timed at
the rate-0.5 shape, forward + inverse, per layer.
`--parent-root DIR`: a built checkout of the parent commit.  Its eager rate-0 step is timed by this script in a child process
before and after this tree's steps (`--root DIR --child`), and `rate0_within_parent` records whether this tree's rate-0 median
lies within the parent's median + this tree's rate-0 10 % .. 90 % width."""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, P, D, LAYERS, HEADS, N = 256, 50176, 256, 768, 12, 12, 196
RATES = (0.0, 0.25, 0.5)
SEED = 0x1234567


def spread(ts):
    s = sorted(ts)
    return s[-1] - s[0], s[int(0.9 * (len(s) - 1))] - s[int(0.1 * (len(s) - 1))]


def stats(ts, unit, nd):
    full, mid = spread(ts)
    return {f"median_{unit}": round(statistics.median(ts), nd), f"min_{unit}": round(min(ts), nd), f"max_{unit}": round(max(ts), nd),
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
    K, T, Tc, dh = N // 2, N + 1, N // 2 + 1, D // HEADS
    i32, bf = torch.int32, torch.bfloat16
    idx, slot = torch.empty(B, K, dtype=i32, device=dev), torch.empty(B, N, dtype=i32, device=dev)
    vf.patch_select(B, N, K, SEED, 49, idx, slot)
    x = torch.randn(B, L, device=dev)
    pat, patg = torch.empty(B * N, P, dtype=bf, device=dev), torch.empty(B * K, P, dtype=bf, device=dev)
    tok, tokg = torch.randn(B, T, D, device=dev), torch.randn(B, Tc, D, device=dev)
    cls, pos = torch.randn(D, device=dev), torch.randn(T, D, device=dev)
    dcls, dpos = torch.empty(D, device=dev), torch.empty(T, D, device=dev)
    dpa, dpag = torch.empty(B * N, D, dtype=bf, device=dev), torch.empty(B * K, D, dtype=bf, device=dev)
    drop = (0.1, SEED, 0)
    dp, dpg, dx = torch.randn(B * N, P, device=dev), torch.randn(B * K, P, device=dev), torch.empty(B, L, device=dev)
    table, tout = torch.randn(T, dh // 2, device=dev), torch.empty(B * Tc, dh // 2, device=dev)
    qkv = torch.randn(B * Tc, 3 * D, device=dev).to(bf)
    cg, sg = torch.randn(B * Tc, dh // 2, device=dev), torch.randn(B * Tc, dh // 2, device=dev)
    pairs = [
        ("unfold_cast", lambda: vf.unfold_cast(x, P, P, N, out=pat), lambda: vf.unfold_gather_cast(x, idx, P, P, N, out=patg)),
        ("embed_finish", lambda: vf.embed_finish(tok, cls, pos, dropout=drop),
         lambda: vf.embed_finish_gather(tokg, cls, idx, T, pos, dropout=drop)),
        ("embed_finish_bwd", lambda: vf.embed_finish_bwd(tok, dcls, dpos, dropout=drop, dpatch=dpa),
         lambda: vf.embed_finish_gather_bwd(tokg, slot, dcls, dpos, dropout=drop, dpatch=dpag)),
        ("fold_add", lambda: vf.fold_add(dp, B, L, P, P, N, out=dx), lambda: vf.fold_add_gather(dpg, slot, L, P, P, out=dx)),
    ]
    rows = []
    for name, plain, gather in pairs:
        tp, tg = time_calls(torch, (plain, gather), runs, warmup)
        rows.append({"kernel": name, "plain_rows": B * N, "gather_rows": B * K,
                     **{"plain_" + k: v for k, v in stats(tp, "us", 1).items()},
                     **{"gather_" + k: v for k, v in stats(tg, "us", 1).items()}})
    alone = [("patch_select", lambda: vf.patch_select(B, N, K, SEED, 49, idx, slot)),
             ("rows_gather", lambda: vf.rows_gather(table, idx, out=tout)),
             ("rope_qk_pass_fwd_plus_inverse", lambda: (vf.rope_qk(qkv, cg, sg, B * Tc, HEADS, dh),
                                                        vf.rope_qk(qkv, cg, sg, B * Tc, HEADS, dh, inverse=True)))]
    for (name, _), ts in zip(alone, time_calls(torch, [f for _, f in alone], runs, warmup)):
        rows.append({"kernel": name, "rows": B * Tc if name != "patch_select" else B * N, **stats(ts, "us", 1)})
    return rows


def make_module(torch, rate, rope=False, layers=LAYERS):
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    model = dict(name="vit", task_type="reg", image_size=L, patch_size=P, hidden_size=D, num_hidden_layers=layers,
                 num_attention_heads=HEADS, stride_size=P, proj_fn="SW")
    if rope:
        model["pos_encoding_type"] = "rope"
    config = {"model": model, "train": dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=False), "loss": {"name": "mae"},
              "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0}}
    seed_everything(42)
    module = ViTLModule(config=config)
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.train()
    module.model.engine.cfg.patch_drop_rate = rate  # an attribute nobody reads on a tree without the feature
    return module, trainer


def make_batch(torch):
    g = torch.Generator(device="cpu").manual_seed(1234)
    return tuple(t.to("cuda:0") for t in (torch.randn((B, L), generator=g), 0.1 * torch.randn((B, L), generator=g).abs(),
                                          torch.rand((B,), generator=g)))


def blocks(torch, steppers, steps, warmup, block=4):
    """`steppers`: {label: callable running ONE step}.  Alternating blocks of `block` steps per label; per-step milliseconds."""
    for _ in range(max(2, warmup)):
        for f in steppers.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in steppers}
    for start in range(0, steps, block):
        for label, f in steppers.items():
            n = min(block, steps - start)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            ev[0].record()
            for i in range(n):
                f()
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[label] += [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]
    return times


def eager_steps(torch, rates, steps, warmup, rope=False):
    """One model per rate: the training arena is sized by the forward's token count, so ONE model switched between rates would
    re-allocate it (17 GB at rate 0) at every switch and time the allocator."""
    batch, steppers, keep = make_batch(torch), {}, []
    for rate in rates:
        module, trainer = make_module(torch, rate, rope=rope)
        keep.append((module, trainer))
        steppers[rate] = (lambda m, t: (lambda: t.training_step(m, batch, 0)))(module, trainer)
    times = blocks(torch, steppers, steps, warmup)
    return {f"rate_{rate}": dict(tokens=None, **stats(ts, "ms", 3)) for rate, ts in times.items()}


def captured_steps(torch, rates, steps, warmup):
    from vit_amd.graph import GraphedTrainStep

    batch = make_batch(torch)
    steppers, keep = {}, []
    for rate in rates:
        module, trainer = make_module(torch, rate)
        gs = GraphedTrainStep(module, trainer.optimizer, batch)
        keep.append((module, trainer, gs))
        steppers[rate] = (lambda g: (lambda: g.step(batch)))(gs)
    times = blocks(torch, steppers, steps, warmup)
    return {f"rate_{rate}": dict(tokens=None, **stats(ts, "ms", 3)) for rate, ts in times.items()}


def with_tokens(doc):
    for key, row in doc.items():
        rate = float(key.split("_")[1])
        K = max(1, int(N * (1.0 - rate)))
        row["tokens"] = 1 + (K if rate > 0 and K < N else N)
    return doc


def parent_rate0(root, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--child", "--steps", str(steps), "--warmup", str(warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"the parent tree's run failed:\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--root", default=HERE, help="the tree vit_amd is imported from")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (its rate-0 step is timed too)")
    ap.add_argument("--child", action="store_true", help="time the eager rate-0 step of --root and print one JSON line")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "patchdrop_bench.json"))
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20 (the figures are medians)")
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from vit_amd import build as vb

    if not torch.cuda.is_available():
        raise SystemExit("patchdrop_bench needs an MI355X: there is nothing to time without one")
    if a.child:
        print(json.dumps(dict(source_stamp=vb.source_stamp()[:16], **eager_steps(torch, (0.0,), a.steps, a.warmup)["rate_0.0"])))
        return 0
    doc = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "warmup": a.warmup, "steps_per_rate": a.steps,
           "source_stamp": vb.source_stamp()[:16], "workload": "vit_b16_224", "batch": B, "precision": "bf16-mixed"}
    parent = [parent_rate0(a.parent_root, a.steps, a.warmup)] if a.parent_root else []
    doc["eager"] = with_tokens(eager_steps(torch, RATES, a.steps, a.warmup))
    if a.parent_root:
        parent.append(parent_rate0(a.parent_root, a.steps, a.warmup))
        ours, width = doc["eager"]["rate_0.0"]["median_ms"], doc["eager"]["rate_0.0"]["p10_p90_ms"]
        pm = statistics.median(p["median_ms"] for p in parent)
        doc["parent"] = {"eager_rate0_runs": parent, "eager_rate0_median_ms": round(pm, 3), "rate0_median_ms": ours,
                         "rate0_p10_p90_ms": width, "rate0_within_parent": bool(ours <= pm + width)}
    gc.collect(); torch.cuda.empty_cache()
    doc["captured"] = with_tokens(captured_steps(torch, RATES, a.steps, a.warmup))
    gc.collect(); torch.cuda.empty_cache()
    doc["rope_eager"] = with_tokens(eager_steps(torch, (0.0, 0.5), a.steps, a.warmup, rope=True))
    doc["rope_eager"]["note"] = "rate 0: rotating QKV epilogue; rate 0.5: vit_rope_qk pass over gathered tables, forward and inverse"
    doc["kernels"] = kernels(a.runs, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for mode in ("eager", "captured", "rope_eager"):
        for key, row in doc[mode].items():
            if key.startswith("rate_"):
                print(f"{mode:10s} {key:9s} T = {row['tokens']:3d}  {row['median_ms']:8.3f} ms [{row['min_ms']:.3f} .. {row['max_ms']:.3f}]"
                      f"  p10-p90 {row['p10_p90_ms']:.3f} ms")
    if "parent" in doc:
        print(json.dumps(doc["parent"]))
    for r in doc["kernels"]:
        print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
