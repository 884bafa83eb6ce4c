"""What the fused SGD / Adam-L2 steps buy over the torch.optim fall-through they replace, and what the bare kernels reach.

    python tools/optim_bench.py --parent DIR [--rounds 3] [--steps 30] [--warmup 10] [--out FILE.json]

`DIR` is a built checkout of the parent commit (its own vit_amd/lib/libvit_amd.so).  This process never touches the GPU: it
starts one fresh worker process per (tree, round), alternating parent / this tree, so both see the same box in the same
minutes.  A worker imports `vit_amd` from ITS tree and times, with hipEvents around blocks of eager `Trainer.training_step`
calls (ms per step, host launches included), bf16-mixed:

    C1 at B = 64 and C3 at B = 256, for  opt: {type: SGD} | {type: SGD, lr_sch: onecycle} | {type: Adam, weight_decay: 0.01}
    C1 at B = 64 with train.hip_graph: true for the same three (the parent warns and falls back to eager launches there)

Per configuration the figure is the median over the rounds; min / max over the rounds is the spread to read it against.
The last worker (this tree only) times the bare kernels at n = 85.8 M against the bytes the algorithm moves per parameter
(shadow included): SGD 14 B, SGD with momentum 22 B, Adam-L2 30 B -- beside vit_adamw_step (30 B) in the same process.

    python tools/optim_bench.py --groups [--parent DIR] [--rounds 3] [--out profiles/optim_groups_bench.json]

The parameter-group study instead (vit_*_step_groups).  Kernel rows at n = 85.8 M, one fresh worker per round, all of them
interleaved in the same process: vit_adamw_step (by value) | the table kernel with one segment | with ViT-B's no-decay table |
with ViT-L's layer-decay + no-decay table (its segments below n) | vit_sgd_step with momentum by value | with one segment.
With `--parent` the same process also loads the parent's library and times its entry points of the same names on the same
buffers (rows "parent: ..."): the yardstick is the parent's by-value kernel, the allowance is the spread that row shows
across the session's rounds.  Step rows: C1 (eager and hip_graph) and C3 with AdamW, weight_decay 0.05, with and without
`no_decay: true` + `layer_decay: 0.75` (`--parent`: its steps beside them)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = {"sgd": {"type": "SGD", "lr": 1e-2}, "sgd_onecycle": {"type": "SGD", "lr": 1e-2, "lr_sch": "onecycle"},
        "adam_l2": {"type": "Adam", "lr": 1e-3, "weight_decay": 0.01}}
CASES = [("C1", 64, False), ("C3", 256, False), ("C1", 64, True)]
GROUP_OPTS = {"adamw": {"type": "AdamW", "lr": 1e-3, "weight_decay": 0.05},
              "adamw_groups": {"type": "AdamW", "lr": 1e-3, "weight_decay": 0.05, "no_decay": True, "layer_decay": 0.75}}
KERNEL_N = 85_800_000


def _train_case(name, batch, graph, opt_name, steps, warmup, dev, opts=OPTS):
    import warnings

    import torch
    from oracle import refvit  # seeded inputs only
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    seed_everything(42)
    rc = refvit.named_config(name)
    cfg = {"model": dict(name="vit", task_type="reg", image_size=rc.image_size, patch_size=rc.patch_size,
                         hidden_size=rc.hidden_size, num_hidden_layers=rc.num_hidden_layers,
                         num_attention_heads=rc.num_attention_heads, stride_size=rc.stride_size, proj_fn="SW"),
           "train": dict(batch_size=batch, ep=1, precision="bf16-mixed", hip_graph=graph),
           "loss": {"name": "mae"}, "opt": dict(opts[opt_name]), "data": {"param": "log_g", "num_samples": batch * 1000},
           "noise": {"noise_level": 0}}
    module = ViTLModule(config=cfg)
    trainer = Trainer(cfg["train"], device=dev, verbose=False)
    trainer._setup(module)
    module.train()
    b = tuple(t.to(dev) for t in refvit.make_inputs(rc, batch, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the parent's "continuing with eager launches"
        for i in range(warmup):
            trainer.training_step(module, b, i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(steps):
            trainer.training_step(module, b, i)
        e1.record()
        torch.cuda.synchronize()
    return {"config": name, "batch": batch, "hip_graph": graph, "opt": opt_name, "optimizer": type(trainer.optimizer).__name__,
            "param_groups": len(trainer.optimizer.param_groups),
            "graph_in_use": bool(trainer.use_graph), "ms_per_step": round(e0.elapsed_time(e1) / steps, 4)}


def _kernels(dev):
    import torch
    import vit_amd.functional as vf

    n = KERNEL_N
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-3
    a, b = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = torch.empty(n, device=dev, dtype=torch.bfloat16)
    sq = torch.ones(1, device=dev)
    clip = dict(sqnorm=sq, max_norm=0.5)
    calls = {
        "sgd (14 B)": (14, lambda: vf.sgd_step(p, g, None, pb, lr=1e-2, **clip)),
        "sgd momentum (22 B)": (22, lambda: vf.sgd_step(p, g, a, pb, lr=1e-2, momentum=0.9, weight_decay=0.01, **clip)),
        "sgd nesterov (22 B)": (22, lambda: vf.sgd_step(p, g, a, pb, lr=1e-2, momentum=0.9, weight_decay=0.01, nesterov=True, **clip)),
        "adam_l2 (30 B)": (30, lambda: vf.adam_l2_step(p, g, a, b, pb, lr=1e-3, weight_decay=0.01, step=3, **clip)),
        "adamw (30 B)": (30, lambda: vf.adamw_step(p, g, a, b, pb, lr=1e-3, weight_decay=0.01, step=3, **clip)),
    }
    out = []
    for name, (nbytes, f) in calls.items():
        f(); f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); f(); f(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 3 * 1e3)
        t = statistics.median(ts)
        out.append({"kernel": name, "n": n, "us": round(t, 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                    "gb_per_s": round(n * nbytes / t / 1e3, 1)})
    return out


def _model_table(hidden, layers, heads, dev, layer_decay):
    """The segment / group tables the fused optimizer would build for a ViT of this shape (no_decay: true, and layer_decay when
    asked), from the parameter layout alone -- no model is allocated."""
    import vit_amd.functional as vf
    from vit_amd.config import ViTConfig
    from vit_amd.engine import ParamLayout
    from vit_amd.optimizer import _layer_id

    lay = ParamLayout(ViTConfig(task_type="reg", image_size=50176, patch_size=256, hidden_size=hidden, num_hidden_layers=layers,
                                num_attention_heads=heads, stride_size=256, num_labels=1))
    keys, triples = {}, []
    for name, (off, shape) in sorted(lay.entries.items(), key=lambda kv: kv[1][0]):
        if off >= lay.n_trainable:
            continue
        skip = len(shape) <= 1 or name.endswith(("cls_token", "position_embeddings"))
        key = (_layer_id(name, layers) if layer_decay else 0, skip)
        triples.append((off, (lay.numel(name) + 7) // 8 * 8, keys.setdefault(key, len(keys))))
    t = vf.optim_group_tables(triples, len(keys), dev)
    vf.optim_groups_write(t, [(1e-3 * 0.75 ** (layers + 1 - d), 0.0 if skip else 0.05, 0.0) for d, skip in keys])
    return t


def _parent_calls(lib_path):
    """The parent library's optimizer entry points under this tree's prototypes (their signatures are the ABI both share),
    called without a handle: they need neither a workspace nor a bound record."""
    import ctypes as C

    from vit_amd import _cabi

    lib = C.CDLL(lib_path)
    for name in ("vit_adamw_step", "vit_adamw_step_groups", "vit_sgd_step", "vit_sgd_step_groups"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _cabi._PROTOS[name], C.c_int

    def call(name, *args):
        if getattr(lib, name)(None, *args) != 0:
            raise SystemExit(f"parent {name} failed")
    return call


def _group_kernels(dev, parent_lib=""):
    import torch
    import vit_amd.functional as vf

    n = KERNEL_N
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-3
    a, b = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = torch.empty(n, device=dev, dtype=torch.bfloat16)
    sq = torch.ones(1, device=dev)
    clip = dict(sqnorm=sq, max_norm=0.5)
    one = vf.optim_group_tables([(0, n, 0)], 1, dev, total=n)
    vf.optim_groups_write(one, [(1e-3, 0.01, 0.0)])
    one_sgd = vf.optim_group_tables([(0, n, 0)], 1, dev, total=n)
    vf.optim_groups_write(one_sgd, [(1e-2, 0.01, 0.9)])
    tables = {"1 segment": one, "ViT-B no_decay": _model_table(768, 12, 12, dev, False),
              "ViT-L layer_decay + no_decay": _model_table(1024, 24, 16, dev, True)}
    # name -> (bytes per parameter, table or None, call)
    calls = {"adamw (by value)": (30, None, lambda: vf.adamw_step(p, g, a, b, pb, lr=1e-3, weight_decay=0.01, step=3, **clip))}
    for name, t in tables.items():
        calls["adamw table, " + name] = (30, t, lambda t=t: vf.adamw_step_groups(p, g, a, b, pb, t, step=3, **clip))
    calls["sgd momentum (by value)"] = (22, None, lambda: vf.sgd_step(p, g, a, pb, lr=1e-2, momentum=0.9, weight_decay=0.01, **clip))
    calls["sgd momentum table, 1 segment"] = (22, one_sgd, lambda: vf.sgd_step_groups(p, g, a, pb, one_sgd, **clip))
    if parent_lib:
        call = _parent_calls(parent_lib)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptrs = (p.data_ptr(), g.data_ptr(), a.data_ptr(), b.data_ptr(), pb.data_ptr(), n)
        sgd_ptrs = (p.data_ptr(), g.data_ptr(), a.data_ptr(), pb.data_ptr(), n)
        tail = (sq.data_ptr(), 0.5, stream)
        calls["parent: adamw (by value)"] = (30, None, lambda: call("vit_adamw_step", *ptrs, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, *tail))
        for name, t in tables.items():
            calls["parent: adamw table, " + name] = (30, t, lambda t=t: call(
                "vit_adamw_step_groups", *ptrs, *vf._groups_args(t, 0), 0.9, 0.999, 1e-8, 3, *tail))
        calls["parent: sgd momentum (by value)"] = (22, None, lambda: call("vit_sgd_step", *sgd_ptrs, 1e-2, 0.9, 0.01, 0, *tail))
        calls["parent: sgd momentum table, 1 segment"] = (22, one_sgd, lambda: call(
            "vit_sgd_step_groups", *sgd_ptrs, *vf._groups_args(one_sgd, 0), 0, *tail))
    out, ts = [], {name: [] for name in calls}
    for _, _, f in calls.values():
        f(); f()
    torch.cuda.synchronize()
    for _ in range(7):  # interleaved: every kernel sees the same minutes
        for name, (_, _, f) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); f(); f(); e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) / 3 * 1e3)
    for name, (nbytes, t, _) in calls.items():
        us = statistics.median(ts[name])
        row = {"kernel": name, "n": n, "bytes_per_param": nbytes, "us": round(us, 1), "us_min": round(min(ts[name]), 1),
               "us_max": round(max(ts[name]), 1), "gb_per_s": round(n * nbytes / us / 1e3, 1)}
        if t is not None:
            row.update(n_groups=t.n_groups, n_segments=t.n_segments, segments_below_n=int((t.seg_end <= n).sum()) + 1)
        out.append(row)
    return out


def worker(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    os.chdir(root)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py times an MI355X; there is no GPU here and no fallback")
    dev = torch.device("cuda", 0)
    if args.worker == "kernels":
        res = _kernels(dev)
    elif args.worker == "group_kernels":
        res = _group_kernels(dev, args.parent_lib)
    elif args.worker == "group_train":
        res = [_train_case(name, batch, graph, opt, args.steps, args.warmup, dev, GROUP_OPTS)
               for name, batch, graph in CASES for opt in GROUP_OPTS]
    else:
        res = [_train_case(name, batch, graph, opt, args.steps, args.warmup, dev)
               for name, batch, graph in CASES for opt in OPTS]
    print("RESULT " + json.dumps(res), flush=True)


def _spawn(root, what, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--root", root, "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    if what == "group_kernels" and args.parent:
        cmd += ["--parent-lib", os.path.join(os.path.abspath(args.parent), "vit_amd", "lib", "libvit_amd.so")]
    env = {k: v for k, v in os.environ.items() if k != "VIT_AMD_LIB"}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
    if r.returncode != 0:
        raise SystemExit(f"worker {what} in {root} failed ({r.returncode}); nothing further is started:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def groups_main(args):
    """The parameter-group study (see the module docstring): kernel rows and step rows, `rounds` fresh workers each."""
    kernel_rounds, train = [], {"this": []}
    if args.parent:
        train["parent"] = []
    for rnd in range(args.rounds):
        kernel_rounds.append(_spawn(HERE, "group_kernels", args))
        print(f"[round {rnd}] kernels: " + " ".join(f"{k['us']:.1f}" for k in kernel_rounds[-1]), flush=True)
        if args.parent:
            train["parent"].append(_spawn(os.path.abspath(args.parent), "group_train", args))
        train["this"].append(_spawn(HERE, "group_train", args))
    kernels = []
    for i, first in enumerate(kernel_rounds[0]):
        us = [r[i]["us"] for r in kernel_rounds]
        row = dict(first, us=round(statistics.median(us), 1), us_rounds=us, us_min=min(r[i]["us_min"] for r in kernel_rounds),
                   us_max=max(r[i]["us_max"] for r in kernel_rounds))
        row["gb_per_s"] = round(row["n"] * row["bytes_per_param"] / row["us"] / 1e3, 1)
        kernels.append(row)
        print(f"{row['kernel']:40s} {row['us']:8.1f} us, rounds {us}, samples [{row['us_min']:.1f} .. {row['us_max']:.1f}] = "
              f"{row['gb_per_s']:.0f} GB/s", flush=True)
    table = []
    for tree, rounds in train.items():
        for i, first in enumerate(rounds[0]):
            ms = [r[i]["ms_per_step"] for r in rounds]
            row = {k: first[k] for k in ("config", "batch", "hip_graph", "opt", "optimizer", "graph_in_use")}
            row.update(tree=tree, param_groups=first.get("param_groups", 1), ms_median=round(statistics.median(ms), 4),
                       ms_min=min(ms), ms_max=max(ms), ms_rounds=ms)
            table.append(row)
            print(f"{tree:6s} {row['config']} B={row['batch']} graph={int(row['graph_in_use'])} {row['opt']:13s} groups="
                  f"{row['param_groups']:2d}: {row['ms_median']:.3f} ms [{row['ms_min']:.3f} .. {row['ms_max']:.3f}]", flush=True)
    line = json.dumps({"optim_groups_bench": {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                                              "kernels": kernels, "train": table}})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--groups", action="store_true", help="the parameter-group study instead")
    ap.add_argument("--worker", default="", choices=["", "train", "kernels", "group_kernels", "group_train"])
    ap.add_argument("--parent-lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.groups:
        return groups_main(args)
    trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this", HERE)]
    runs = {t: [] for t, _ in trees}
    for rnd in range(args.rounds):
        for tree, root in trees:
            runs[tree].append(_spawn(root, "train", args))
            print(f"[round {rnd}] {tree}: " + " ".join(f"{r['ms_per_step']:.2f}" for r in runs[tree][-1]), flush=True)
    table = []
    for i, (name, batch, graph) in enumerate((c, b, g) for c, b, g in CASES for _ in OPTS):
        opt = list(OPTS)[i % len(OPTS)]
        row = {"config": name, "batch": batch, "hip_graph": graph, "opt": opt}
        for tree in runs:
            ms = [r[i]["ms_per_step"] for r in runs[tree]]
            row[tree] = {"optimizer": runs[tree][0][i]["optimizer"], "graph_in_use": runs[tree][0][i]["graph_in_use"],
                         "ms_median": round(statistics.median(ms), 4), "ms_min": min(ms), "ms_max": max(ms), "ms_rounds": ms}
        table.append(row)
        print(f"{name} B={batch} graph={int(graph)} {opt:13s} " + "  ".join(
            f"{t}: {row[t]['ms_median']:.3f} ms [{row[t]['ms_min']:.3f} .. {row[t]['ms_max']:.3f}] ({row[t]['optimizer']}"
            f"{', graph' if row[t]['graph_in_use'] else ''})" for t in runs), flush=True)
    kernels = _spawn(HERE, "kernels", args)
    for k in kernels:
        print(f"{k['kernel']:22s} n = {k['n'] / 1e6:.1f} M: {k['us']:8.1f} us [{k['us_min']:.1f} .. {k['us_max']:.1f}] = "
              f"{k['gb_per_s']:.0f} GB/s", flush=True)
    line = json.dumps({"optim_bench": {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "train": table,
                                       "kernels": kernels}})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
