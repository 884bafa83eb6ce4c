"""What the fused Muon step costs: its grouped Newton-Schulz products, its streaming passes, and the step around them.

    python tools/muon_bench.py [--rounds 7] [--reps 2] [--steps 12] [--skip-steps] [--out profiles/muon_bench.json]

One process, one MI355X, ViT-B/16 geometry (12 layers, D = 768, F = 3072: 72 encoder matrices, 84.9 M elements), variants
alternating within every round, medians with p10-p90 over the rounds, hipEvents around `reps` back-to-back calls.  Inputs are
N(0, 1) draws, not zeros.  Nothing here checks values (tests/test_muon_gpu.py does).

Expectations, written before the first run and not edited afterwards; a miss is printed as FAILS:
  (1) the 15 grouped launches of ns_steps = 5 (1,080 products, 1.63 TFLOP) against the same 1,080 products issued one by one
      through vit_gemm: FASTER.  The achieved TFLOP/s of the 1.63 TFLOP is reported.
  (2) the four streaming passes (momentum + partials, norms, normalise, apply: 4 + 2 + 2 | 2 + 2 | 4 + 2 + 4 + 2 = 24 B per matrix
      element with the shadow) against vit_lamb_step_groups over the same 84.9 M elements (42 B): NO SLOWER beyond the wider
      p10-p90 of the two.
  (3) the eager and the captured training step (B = 256, bf16-mixed) with opt.type muon against the same step with AdamW:
      reported beside the FLOP floor of 6 % (1.63 / 26.9 TFLOP); no expectation is set on it.
  (4) bench.py on this tree and on the parent's is a separate run of bench.py itself.
Not measured: multi-GPU runs, accuracy on real spectra."""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

D, F, LAYERS = 768, 3072, 12
NS_STEPS = 5


def _shapes():
    return [s for _ in range(LAYERS) for s in ((D, D), (D, D), (D, D), (D, D), (F, D), (D, F))]


def _flop(shapes, ns_steps):
    total = 0
    for r, c in shapes:
        m, n = min(r, c), max(r, c)
        total += ns_steps * (2 * m * m * n + 2 * m * m * m + 2 * m * m * n)
    return total


def _spread(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=10) if len(xs) >= 3 else [xs[0], xs[-1]]
    return statistics.median(xs), q[0], q[-1]


def _timed(calls, rounds, reps, torch):
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(rounds):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) / reps * 1e3)
    return {k: _spread(v) for k, v in ts.items()}


def _step_run(opt_cfg, use_graph, torch, dev):
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    L, P, B = 50176, 256, 256
    config = {"model": dict(name="vit", task_type="reg", image_size=L, patch_size=P, hidden_size=D, num_hidden_layers=LAYERS,
                            num_attention_heads=12, stride_size=P, proj_fn="SW"),
              "train": dict(batch_size=B, ep=1, precision="bf16-mixed", hip_graph=use_graph), "loss": {"name": "mae"},
              "opt": dict(opt_cfg), "data": {"param": "log_g"}, "noise": {"noise_level": 0}}
    seed_everything(42)
    with contextlib.redirect_stdout(sys.stderr):
        module = ViTLModule(config=config)
    trainer = Trainer(config["train"], device=dev, verbose=False)
    trainer._setup(module)
    module.train()
    g = torch.Generator(device="cpu").manual_seed(1234)
    batch = (torch.randn((B, L), generator=g).to(dev), (0.1 * torch.randn((B, L), generator=g).abs()).to(dev),
             torch.rand((B,), generator=g).to(dev))
    count = [0]

    def step():
        trainer.training_step(module, batch, count[0])
        count[0] += 1
    return step


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--skip-steps", action="store_true", help="leave out (3), the full training steps")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("muon_bench.py times an MI355X; there is no GPU here and no fallback")
    import vit_amd.functional as vf

    dev = torch.device("cuda", 0)
    shapes = _shapes()
    ents, off = [], 0
    for r, c in shapes:
        ents.append((off, off, r, c, 0, vf.muon_adjust_ratio("match_rms_adamw", r, c)))
        off += r * c
    n = off
    tables = vf.muon_mat_table(ents, dev)
    plan = vf.MuonPlan(tables, (3.4445, -4.775, 2.0315), dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    p = torch.randn(n, device=dev, generator=gen) * 0.02
    buf, m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = torch.empty(n, device=dev, dtype=torch.bfloat16)
    part = torch.zeros(tables.n_tiles, dtype=torch.float64, device=dev)
    inv, norms = torch.zeros(tables.n_mats, device=dev), torch.zeros(tables.n_mats, device=dev)
    sq = torch.ones(1, device=dev)
    groups = torch.tensor([[1e-3, 0.05, 0.0, 0.0]], device=dev)
    lamb_tab = vf.optim_param_tables([(o, r * c, 0) for o, _, r, c, _, _ in ents], 1, dev)
    vf.optim_groups_write(lamb_tab, [(1e-3, 0.05, 0.0)])
    trust = torch.ones(lamb_tab.n_segments, device=dev)

    def streaming():
        vf.muon_momentum(g, buf, plan.x[1], tables, part, sqnorm=sq, max_norm=0.5)
        vf.muon_norms(tables, part, inv, norms)
        vf.muon_normalize(plan.x[1], plan.x[0], tables, inv)
        vf.muon_apply(p, pb, plan.x[1], tables, groups)

    def grouped():
        plan.iterate(NS_STEPS)

    def one_by_one():  # the same products, one vit_gemm each; the epilogue's beta * R term is left out (it only helps this side)
        # (vit_gemm's b_trans = False reads B as [N, K], K-contiguous; True as [K, N])
        for _ in range(NS_STEPS):
            for k in range(0, len(plan.gram[0].held), 4):
                X, _, _, Am = plan.gram[0].held[k:k + 4]
                vf.gemm(X, X, M=X.shape[0], N=X.shape[0], K=X.shape[1], out=Am)
            for k in range(0, len(plan.poly.held), 4):
                Am, _, _, Bm = plan.poly.held[k:k + 4]
                vf.gemm(Am, Am, M=Am.shape[0], N=Am.shape[0], K=Am.shape[0], out=Bm)
            for k in range(0, len(plan.upd[0].held), 4):
                Bm, X, _, Xn = plan.upd[0].held[k:k + 4]
                vf.gemm(Bm, X, M=Bm.shape[0], N=X.shape[1], K=Bm.shape[1], b_trans=True, out=Xn)

    def lamb():
        vf.lamb_step_groups(p, g, m, v, pb, lamb_tab, trust, step=3, sqnorm=sq, max_norm=0.5)

    vf.muon_momentum(g, buf, plan.x[1], tables, part)
    vf.muon_norms(tables, part, inv, norms)
    vf.muon_normalize(plan.x[1], plan.x[0], tables, inv)
    res = _timed({"grouped": grouped, "one_by_one": one_by_one, "streaming": streaming, "lamb": lamb}, args.rounds, args.reps, torch)
    flop = _flop(shapes, NS_STEPS)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "matrices": len(shapes), "elements": n,
           "ns_flop": flop, "us": {k: {"median": round(a, 1), "p10": round(b, 1), "p90": round(c, 1)} for k, (a, b, c) in res.items()}}
    gm, om = res["grouped"][0], res["one_by_one"][0]
    out["grouped_tflops"] = round(flop / gm / 1e6, 1)
    out["expect_1_grouped_faster"] = "holds" if gm < om else "FAILS"
    sm, lm = res["streaming"][0], res["lamb"][0]
    room = max(res["streaming"][2] - res["streaming"][1], res["lamb"][2] - res["lamb"][1])
    out["expect_2_streaming_no_slower_than_lamb"] = "holds" if sm <= lm + room else "FAILS"
    print(f"(1) grouped {gm:.0f} us = {out['grouped_tflops']} TFLOP/s, one by one {om:.0f} us: {out['expect_1_grouped_faster']}")
    print(f"(2) streaming {sm:.0f} us, lamb {lm:.0f} us (room {room:.0f}): {out['expect_2_streaming_no_slower_than_lamb']}")
    if not args.skip_steps:
        muon_cfg, adamw_cfg = {"type": "muon", "lr": 1e-3, "weight_decay": 0.05}, {"type": "AdamW", "lr": 1e-3, "weight_decay": 0.05}
        steps = {}
        for graph in (False, True):
            calls = {f"{name}_{'captured' if graph else 'eager'}": _step_run(cfg, graph, torch, dev)
                     for name, cfg in (("adamw", adamw_cfg), ("muon", muon_cfg))}
            for f in calls.values():
                for _ in range(3):
                    f()
            r = _timed(calls, args.steps, 1, torch)
            steps.update({k: {"median_ms": round(a / 1e3, 3), "p10_ms": round(b / 1e3, 3), "p90_ms": round(c / 1e3, 3)}
                          for k, (a, b, c) in r.items()})
            del calls
            torch.cuda.empty_cache()
        out["steps"] = steps
        for mode in ("eager", "captured"):
            a, b = steps[f"adamw_{mode}"]["median_ms"], steps[f"muon_{mode}"]["median_ms"]
            out[f"muon_over_adamw_{mode}"] = round(b / a, 4)
            print(f"(3) {mode}: adamw {a:.2f} ms, muon {b:.2f} ms, ratio {b / a:.4f} (FLOP floor 1.06)")
    line = json.dumps({"muon_bench": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
