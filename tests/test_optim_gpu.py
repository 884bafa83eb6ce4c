"""The fused SGD and Adam-with-L2-decay steps on the MI355X, from the kernels (vit_amd/csrc/optim.hip) up to the trainer:
each layer against torch.optim.SGD / torch.optim.Adam on identical gradients (the reference builds exactly those:
src/opt/optimizer.py:14-26,108), the captured step against the eager one bit for bit, `zero1` against `allreduce`.

Gates.  Kernel level: rel(p, p_torch) < 1e-6 after every step -- the project's gate for the AdamW kernel
(test_kernels_gpu.py::test_sqnorm_adamw); it leaves room for f32 reordering only.  The same gate for the momentum buffer and
the Adam moments (for the second moment see test_adam_l2_kernel_second_moment_equals_torch_adam); the bf16 shadow is
bf16(p) exactly.  Model level: rel < 2e-6 per parameter on identical gradients (the step-0 gate of
test_parity_gpu.py::test_fused_adamw_equals_torch_adamw), the clipping norm at 1e-6."""
import copy
import os
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tail only | exactly one 16-byte vector | vector + tail | many blocks + tail | one element past ... a full pass of the
# launch's grid (grid_for caps it at 4096 blocks x 256 lanes x 4 floats): the stride loop runs a second time
SIZES = [1, 3, 4, 7, 1027, 4096 * 256 * 4 + 1027]
SGD_CASES = [(0.0, 0.0, False), (0.9, 0.01, False), (0.9, 0.01, True)]  # (momentum, weight_decay, nesterov)
MAX_NORM = 0.5


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _clip_like_torch(pt, gd):
    """clip_grad_norm_(MAX_NORM) on the torch side; for the kernel, the squared norm the fused step would be handed.

    The kernel under test turns a squared norm into the coefficient min(1, max_norm / (sqrt(sq) + 1e-6)); it does not compute
    the norm.  torch's f32 reduction on the CPU is itself off by up to 8e-5 relative at the largest size here (measured
    against float64; it depends on the host's thread count), 80 times the gate -- so the kernel gets the very norm torch
    clipped with, and vit_grad_sqnorm is held against float64 instead: at most ~40 f32 roundings lie between an element and
    the total (4 serial adds per lane, 6 + 2 tree levels per block, 16 serial + 8 tree levels across blocks), 2.4e-6 on the
    sum of squares in the worst case, half of that on the norm, plus the square root's own rounding: 1.5e-6."""
    import vit_amd.functional as vf

    norm = torch.nn.utils.clip_grad_norm_([pt], MAX_NORM)
    assert float(norm) > MAX_NORM  # the coefficient is not 1
    exact = float(gd.double().norm())
    ours = float(vf.grad_sqnorm(gd).sqrt())
    assert abs(ours - exact) <= 1.5e-6 * exact, (ours, exact)
    return (norm.to(gd.device, torch.float32) ** 2).reshape(1)


def _inputs(n):
    gen = torch.Generator().manual_seed(1000 + n % 997)
    p0 = torch.randn(n, generator=gen)
    g0 = torch.randn(n, generator=gen)
    g0[0] = 1.0 + g0[0].abs()  # whatever n: the norm is above MAX_NORM, the clip coefficient is not 1
    return p0, g0


# ---------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("momentum,wd,nesterov", SGD_CASES)
@pytest.mark.parametrize("n", SIZES)
def test_sgd_kernel_equals_torch_sgd(dev, n, momentum, wd, nesterov, clip):
    import vit_amd.functional as vf

    p0, g0 = _inputs(n)
    pt = p0.clone().requires_grad_(True)
    ref = torch.optim.SGD([pt], lr=0.1, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    p = p0.to(dev)
    # without a momentum the kernel must neither read nor write a buffer: a poisoned one beside the call stays poisoned
    buf = torch.zeros(n, device=dev) if momentum else torch.full((n,), float("nan"), device=dev)
    pb = torch.empty(n, dtype=torch.bfloat16, device=dev)
    for step in range(1, 4):
        gs = g0 * step
        pt.grad = gs.clone()
        gd = gs.to(dev)
        sq = _clip_like_torch(pt, gd) if clip else None
        ref.step()
        vf.sgd_step(p, gd, buf, pb, lr=0.1, momentum=momentum, weight_decay=wd, nesterov=nesterov, sqnorm=sq, max_norm=MAX_NORM)
        e = rel(p, pt.detach())
        assert e < 1e-6, (step, e)
        if momentum:
            e = rel(buf, ref.state[pt]["momentum_buffer"])
            assert e < 1e-6, (step, e)
        assert torch.equal(pb, p.to(torch.bfloat16))
    if not momentum:
        assert torch.isnan(buf).all() and torch.isfinite(p).all()


def _adam_l2_three_steps(dev, n, clip):
    """(rel p, rel exp_avg, rel exp_avg_sq, shadow == bf16(p)) after each of three steps against torch.optim.Adam."""
    import vit_amd.functional as vf

    p0, g0 = _inputs(n)
    pt = p0.clone().requires_grad_(True)
    ref = torch.optim.Adam([pt], lr=1e-3, weight_decay=0.01)
    p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pb = torch.empty(n, dtype=torch.bfloat16, device=dev)
    out = []
    for step in range(1, 4):
        gs = g0 * step
        pt.grad = gs.clone()
        gd = gs.to(dev)
        sq = _clip_like_torch(pt, gd) if clip else None
        ref.step()
        vf.adam_l2_step(p, gd, m, v, pb, lr=1e-3, weight_decay=0.01, step=step, sqnorm=sq, max_norm=MAX_NORM)
        out.append((rel(p, pt.detach()), rel(m, ref.state[pt]["exp_avg"]), rel(v, ref.state[pt]["exp_avg_sq"]),
                    torch.equal(pb, p.to(torch.bfloat16))))
    return out


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_l2_kernel_equals_torch_adam(dev, n, clip):
    for step, (ep, em, ev, shadow_ok) in enumerate(_adam_l2_three_steps(dev, n, clip), 1):
        print(f"[adam_l2 n={n} clip={clip} step={step}] rel p {ep:.2e} exp_avg {em:.2e} exp_avg_sq {ev:.2e}")
        assert ep < 1e-6 and em < 1e-6, (step, ep, em)
        assert shadow_ok


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_l2_kernel_second_moment_equals_torch_adam(dev, n, clip):
    """The same 1e-6 gate on exp_avg_sq.  It holds only because the entry point forms the weight of g'^2 as torch does,
    float(1 - 0.999) = 0.001f: with AdamW's 1.f - 0.999f = 0.00099998713 exp_avg_sq sits 1.29e-5 off torch's in every case."""
    for step, (_, _, ev, _) in enumerate(_adam_l2_three_steps(dev, n, clip), 1):
        assert ev < 1e-6, (step, ev)


# ----------------------------------------------------------------------------------------------------------- model level
def _fused_and_torch(kind, model, twins):
    from vit_amd.optimizer import FusedAdamW, FusedSGD

    if kind == "sgd":
        kw = dict(lr=1e-2)
        return FusedSGD(model, **kw), torch.optim.SGD(twins, **kw)
    if kind == "sgd_momentum":
        kw = dict(lr=1e-2, momentum=0.9, weight_decay=0.01)
        return FusedSGD(model, **kw), torch.optim.SGD(twins, **kw)
    if kind == "sgd_nesterov":
        kw = dict(lr=1e-2, momentum=0.9, weight_decay=0.01, nesterov=True)
        return FusedSGD(model, **kw), torch.optim.SGD(twins, **kw)
    kw = dict(lr=1e-3, weight_decay=0.01)
    return FusedAdamW(model, adam_l2=True, **kw), torch.optim.Adam(twins, **kw)


def _hand_over_grads(model, twins):
    """The twin is never run: its gradients are clones of the model's (views of the flat gradient buffer), so both optimizers
    see identical gradients and only the update arithmetic differs."""
    for tw, p in zip(twins, model.parameters()):
        tw.grad = None if p.grad is None else p.grad.detach().clone()
    return [tw for tw in twins if tw.grad is not None]


def _assert_same(model, twins, start, step):
    for (name, p), tw, p0 in zip(model.named_parameters(), twins, start):
        if p.grad is None:  # the pooler: no gradient, untouched by both
            assert torch.equal(p.detach(), p0) and torch.equal(tw.detach(), p0), name
            continue
        e = rel(p.detach(), tw.detach())
        assert e < 2e-6, (step, name, e)


@pytest.mark.parametrize("kind", ["sgd", "sgd_momentum", "sgd_nesterov", "adam_l2"])
def test_fused_optimizer_equals_torch_on_the_model(dev, kind):
    from test_parity_gpu import setup

    rc, g, sd, model, x, labels = setup("c1", dev)
    model.eval()
    twins = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    start = [p.detach().clone() for p in model.parameters()]
    fused, ref = _fused_and_torch(kind, model, twins)
    fused.set_grad_clip(MAX_NORM)
    gradless = 0
    for s in range(3):
        fused.zero_grad()
        model(x, labels=labels).loss.backward()
        with_grad = _hand_over_grads(model, twins)
        gradless = len(twins) - len(with_grad)
        norm = torch.nn.utils.clip_grad_norm_(with_grad, MAX_NORM)
        fused.step()
        ref.step()
        got = float(fused.last_grad_norm.sqrt())
        assert abs(got - float(norm)) <= 1e-6 * float(norm), (s, got, float(norm))
        _assert_same(model, twins, start, s)
    assert gradless >= 1  # the case "a parameter without a gradient" was there
    assert any(not torch.equal(p.detach(), p0) for p, p0 in zip(model.parameters(), start))


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_one_group_follows_its_param_group_from_step_to_step(dev, kind):
    """One group is a one-segment, one-row table: `param_groups[0]["lr"]` (for SGD also the momentum, 0 -> 0.9 -> 0) changes
    between the steps and every step agrees with torch's class at the model-level gate.  While SGD's momentum is 0 the buffer
    is neither read nor written: there is none after step 1, and a NaN-poisoned slice of it stays poisoned in step 4."""
    from test_parity_gpu import setup
    from vit_amd.optimizer import FusedAdamW, FusedSGD

    rc, g, sd, model, x, labels = setup("c1", dev)
    model.eval()
    twins = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    start = [p.detach().clone() for p in model.parameters()]
    if kind == "sgd":
        kw = dict(lr=1e-2, weight_decay=0.01)
        fused, ref = FusedSGD(model, **kw), torch.optim.SGD(twins, **kw)
        lrs, mus = [1e-2, 5e-3, 2e-2, 1e-3], [0.0, 0.9, 0.9, 0.0]
    else:
        kw = dict(lr=1e-3, weight_decay=0.05)
        fused, ref = FusedAdamW(model, **kw), torch.optim.AdamW(twins, **kw)
        lrs, mus = [1e-3, 5e-4, 2e-3, 1e-4], [None] * 4
    assert len(fused.param_groups) == 1
    fused.set_grad_clip(MAX_NORM)
    poisoned = slice(1024, 1024 + 264)
    for s, (lr, mu) in enumerate(zip(lrs, mus)):
        for opt in (fused, ref):
            opt.param_groups[0]["lr"] = lr
            if mu is not None:
                opt.param_groups[0]["momentum"] = mu
        if kind == "sgd" and s == 3:
            fused._buf[poisoned] = float("nan")
        fused.zero_grad()
        model(x, labels=labels).loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(_hand_over_grads(model, twins), MAX_NORM)
        fused.step()
        ref.step()
        got = float(fused.last_grad_norm.sqrt())
        assert abs(got - float(norm)) <= 1e-6 * float(norm), (s, got, float(norm))
        _assert_same(model, twins, start, s)
        if kind == "sgd" and s == 0:
            assert fused._buf is None
        if kind == "sgd" and s == 2:  # the buffer torch keeps, before a slice of ours is poisoned
            lay = model.engine.layout
            for (name, p), tw in zip(model.named_parameters(), twins):
                if p.grad is not None:
                    off = lay.entries[name][0]
                    e = rel(fused._buf[off:off + p.numel()], ref.state[tw]["momentum_buffer"].reshape(-1))
                    assert e < 2e-6, (name, e)
    t = fused._partition()[2]
    assert (t.n_segments, t.n_groups) == (1, 1)
    if kind == "sgd":
        assert torch.isnan(fused._buf[poisoned]).all() and torch.isfinite(model.engine.flat).all()
        rest = fused._buf.clone()
        rest[poisoned] = 0
        assert torch.isfinite(rest).all() and float(rest.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------- state and trainer
@pytest.mark.parametrize("kind", ["sgd_momentum", "adam_l2"])
def test_fused_state_is_torch_state(dev, kind):
    """state_dict() after two steps loads into the torch class over the twin, and torch's loads back: the third step of both
    agrees at the model-level gate, and a fresh fused optimizer that loads torch's state holds the same buffers."""
    from test_parity_gpu import setup

    rc, g, sd, model, x, labels = setup("c1", dev)
    model.eval()
    fused, _ = _fused_and_torch(kind, model, [torch.nn.Parameter(torch.zeros(1))])
    for s in range(2):
        fused.zero_grad()
        model(x, labels=labels).loss.backward()
        fused.step()
    twins = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    start = [p.detach().clone() for p in model.parameters()]
    _, ref = _fused_and_torch(kind, model, twins)
    ref.load_state_dict(copy.deepcopy(fused.state_dict()))
    fused.zero_grad()
    model(x, labels=labels).loss.backward()
    _hand_over_grads(model, twins)
    fused.step()
    ref.step()
    _assert_same(model, twins, start, 2)
    # and back
    fresh, _ = _fused_and_torch(kind, model, [torch.nn.Parameter(torch.zeros(1))])
    fresh.load_state_dict(ref.state_dict())
    # the load is a copy: what the fresh optimizer now holds IS torch's state, tensor for tensor
    sd1, sd2 = fresh.state_dict(), ref.state_dict()
    assert sorted(sd1["state"]) == sorted(sd2["state"]) and len(sd1["state"]) > 10
    for i, st in sd2["state"].items():
        assert set(sd1["state"][i]) == set(st), i
        for k, t in st.items():
            assert torch.equal(sd1["state"][i][k].float().cpu(), t.float().cpu()), (i, k)
    if kind == "adam_l2":
        assert fresh._step == 3 and fresh.adam_l2
    else:
        assert fresh.param_groups[0]["momentum"] == 0.9
        assert all(set(st) == {"momentum_buffer"} for st in sd1["state"].values())


def test_trainer_runs_sgd_under_one_cycle_as_fused_sgd_with_momentum(dev):
    """`opt: {type: SGD, lr_sch: onecycle}`: OneCycleLR cycles SGD's momentum (0.95 -> 0.85 -> ...), so this is SGD WITH
    momentum although the reference constructs it with momentum 0; the (lr, momentum) trace is torch's own."""
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.optimizer import FusedSGD

    cfg = c1_config(precision="bf16-mixed")
    cfg["opt"] = {"type": "SGD", "lr": 1e-2, "lr_sch": "onecycle"}
    cfg["data"]["num_samples"] = 64
    module, trainer = make(cfg)
    trainer._setup(module)
    module.train()
    opt = trainer.optimizer
    assert type(opt) is FusedSGD and opt._buf is None
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    sched = torch.optim.lr_scheduler.OneCycleLR(dummy, max_lr=1e-2, steps_per_epoch=4, epochs=2)
    batches = [tuple(t.to(dev) for t in b) for b in Batches(64, 5)]
    for i in range(4):
        before = module.model.engine.flat.detach().clone()
        assert (opt.param_groups[0]["lr"], opt.param_groups[0]["momentum"]) == \
               (dummy.param_groups[0]["lr"], dummy.param_groups[0]["momentum"]), i
        loss = trainer.training_step(module, batches[i], i)
        dummy.step()
        sched.step()
        assert torch.isfinite(loss) and not torch.equal(before, module.model.engine.flat)
        assert opt._buf is not None and float(opt._buf.abs().max()) > 0  # exists after step 1
    assert trainer.global_step == 4


def test_snapshot_restore_puts_the_sgd_buffer_back(dev):
    from test_trainer_gpu import Batches, c1_config, make

    cfg = c1_config(precision="bf16-mixed")
    cfg["opt"] = {"type": "SGD", "lr": 1e-2, "lr_sch": "onecycle"}
    cfg["data"]["num_samples"] = 64
    module, trainer = make(cfg)
    trainer._setup(module)
    module.train()
    batches = [tuple(t.to(dev) for t in b) for b in Batches(64, 5)]
    snap0 = trainer._snapshot(module)  # before any step: no buffer yet
    trainer.training_step(module, batches[0], 0)
    opt = trainer.optimizer
    kept = (opt._buf.clone(), module.model.engine.flat.clone(), opt._step, dict(opt.param_groups[0], params=None))
    snap = trainer._snapshot(module)
    for i in range(2):
        trainer.training_step(module, batches[1 + i], i)
    assert not torch.equal(opt._buf, kept[0])
    trainer._restore(module, snap)
    assert torch.equal(opt._buf, kept[0]) and torch.equal(module.model.engine.flat, kept[1]) and opt._step == kept[2]
    assert dict(opt.param_groups[0], params=None) == kept[3]
    trainer._restore(module, snap0)
    assert opt._buf is None and opt._step == 0


# ------------------------------------------------------------------------------------------------------------------ graph
def _graph_vs_eager(dev, precision, opt_cfg, mid_run_lr):
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedOptimizer

    batches = list(Batches(64, 5))
    finals = {}
    for mode in ("eager", "graph"):
        cfg = c1_config(precision=precision, hip_graph=(mode == "graph"))
        cfg["opt"] = dict(opt_cfg)
        cfg["data"]["num_samples"] = 64
        module, trainer = make(cfg)
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        opt = trainer.optimizer
        assert isinstance(opt, FusedOptimizer)
        losses, trace = [], []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for i in range(4):
                if mid_run_lr is not None and i == 2:
                    opt.param_groups[0]["lr"] = mid_run_lr
                trace.append((opt.param_groups[0]["lr"], opt.param_groups[0].get("momentum")))
                b = tuple(t.cuda() for t in batches[i % 2])
                losses.append(float(trainer.training_step(module, b, i)))
        assert not [w for w in caught if "hip_graph" in str(w.message)], [str(w.message) for w in caught]
        state = [getattr(opt, name).detach().cpu().clone() for name in opt._STATE]
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in module.model.state_dict().items()}, state,
                        float(opt.last_grad_norm), opt._step, trace)
        if mode == "graph":
            assert trainer.use_graph
            assert len(trainer._graphed) == 1 and all(isinstance(g, GraphedTrainStep) for g in trainer._graphed.values())
    e, g = finals["eager"], finals["graph"]
    assert e[0] == g[0], (e[0], g[0])
    for k in e[1]:
        assert torch.equal(e[1][k], g[1][k]), k
    assert len(e[2]) == len(g[2]) >= 1 and all(torch.equal(a, b) for a, b in zip(e[2], g[2]))
    assert e[3] == g[3] and e[4] == g[4] == 4 and e[5] == g[5]
    assert e[0][0] != e[0][2]  # the parameters moved: the same batch gives another loss two steps later
    return e


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_hip_graph_sgd_one_cycle_equals_eager(dev, precision):
    """lr AND momentum change on every replay (both read from the group table): four replays == four eager steps bit for
    bit in losses, parameters, momentum buffer and clipping norm."""
    e = _graph_vs_eager(dev, precision, {"type": "SGD", "lr": 1e-2, "lr_sch": "onecycle"}, None)
    assert len({t for t in e[5]}) == 4 and all(mu for _, mu in e[5])


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_hip_graph_adam_l2_equals_eager(dev, precision):
    _graph_vs_eager(dev, precision, {"type": "Adam", "lr": 1e-3, "weight_decay": 0.01}, 3e-4)


def test_hip_graph_refuses_a_momentum_that_appears_after_capture(dev):
    """Captured without a momentum buffer, the step cannot take a momentum later: one warning, eager launches from then on."""
    from test_trainer_gpu import Batches, c1_config, make

    cfg = c1_config(precision="bf16-mixed", hip_graph=True)
    cfg["opt"] = {"type": "SGD", "lr": 1e-2}
    module, trainer = make(cfg)
    trainer._setup(module)
    module.train()
    b = tuple(t.to(dev) for t in next(iter(Batches(16, 5))))
    trainer.training_step(module, b, 0)
    assert trainer.use_graph and trainer.optimizer._buf is None
    trainer.optimizer.param_groups[0]["momentum"] = 0.9
    with pytest.warns(UserWarning, match="momentum"):
        loss = trainer.training_step(module, b, 1)
    assert not trainer.use_graph and torch.isfinite(loss) and trainer.optimizer._buf is not None
    assert trainer.global_step == 2


def test_hip_graph_keeps_a_momentum_that_becomes_zero_on_the_graph(dev):
    """Captured with a momentum buffer, a momentum that becomes 0 stays on the graph: the kernel skips a zero-momentum row's
    buffer itself.  No warning, the buffer keeps its bits over the replay, and the parameters are the eager twin's bit for bit."""
    from test_trainer_gpu import Batches, c1_config, make

    b = tuple(t.to(dev) for t in next(iter(Batches(16, 5))))
    finals = {}
    for mode in ("eager", "graph"):
        cfg = c1_config(precision="bf16-mixed", hip_graph=(mode == "graph"))
        cfg["opt"] = {"type": "SGD", "lr": 1e-2}
        module, trainer = make(cfg)
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        opt = trainer.optimizer
        opt.param_groups[0]["momentum"] = 0.9
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            trainer.training_step(module, b, 0)
            assert opt._buf is not None and float(opt._buf.abs().max()) > 0
            before = opt._buf.detach().clone()
            opt.param_groups[0]["momentum"] = 0
            loss = trainer.training_step(module, b, 1)
        assert not [w for w in caught if "hip_graph" in str(w.message)], [str(w.message) for w in caught]
        assert trainer.use_graph == (mode == "graph") and torch.isfinite(loss) and trainer.global_step == 2
        assert torch.equal(opt._buf, before)
        finals[mode] = (module.model.engine.flat.detach().clone(), before, float(loss))
    assert torch.equal(finals["eager"][0], finals["graph"][0]) and torch.equal(finals["eager"][1], finals["graph"][1])
    assert finals["eager"][2] == finals["graph"][2]


# -------------------------------------------------------------------------------------------------------- data parallelism
def test_sgd_zero1_matches_allreduce(tmp_path):
    """Two gloo ranks on the one GPU, SGD with momentum 0.9: reduce-scatter -> update of the owned shard -> all-gather leaves
    the parameters of all-reduce + full update (the gate of test_ddp_gpu.py::test_zero1_exchange_matches_allreduce), on both
    ranks, and the gathered momentum buffer is the all-reduce run's."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    child = os.path.join(ROOT, "tests", "_optim_ddp_child.py")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VIT_DIST_BACKEND="gloo")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, child, str(tmp_path), "allreduce", "zero1"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[-2000:] for o in outs)
    ranks = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2)]
    a, z = ranks[0]["allreduce"], ranks[0]["zero1"]
    assert a["mode"] == "allreduce" and z["mode"] == "zero1" and z["world"] == 2
    n = a["n_trainable"]
    print(f"[sgd ddp] norms allreduce {a['norms']} zero1 {z['norms']}; "
          f"max |dp| {float((a['params'][:n] - z['params'][:n]).abs().max()):.3e}")
    for ex in ("allreduce", "zero1"):
        assert torch.equal(ranks[0][ex]["params"], ranks[1][ex]["params"]), ex
        assert torch.equal(ranks[0][ex]["buf"][:n], ranks[1][ex]["buf"][:n]), ex
    for na, nz in zip(a["norms"], z["norms"]):
        assert abs(na - nz) <= 1e-6 * na
    assert torch.equal(a["params"][:n], z["params"][:n])
    assert torch.equal(a["buf"][:n], z["buf"][:n])
    assert float(a["buf"][:n].abs().max()) > 0
