"""The exponential moving average of the weights on the MI355X (`train.ema_decay`), from the kernels (vit_amd/csrc/ema.hip) up
to the trainer: vit_ema_update against torch.lerp on the same values, vit_ema_swap bit for bit, the averager against a
torch.optim.swa_utils.AveragedModel twin fed clones of the run's own parameters, validation / checkpoints / resume on the
averaged weights, the captured step against the eager one, accumulation, a trainable input preprocessor, two ranks.

Gates.  Kernel level: rel(ema, torch.lerp twin) < 1e-6 after every update -- the project's gate for the optimizer kernels
(test_optim_gpu.py); a two-rounding f32 restatement of the formula stays within 3.4e-8 of AveragedModel over 5 updates, so the
gate leaves room for torch's choice of fused or unfused rounding and nothing else.  Model level: rel < 2e-6 per parameter (the
model-level optimizer gate).  Everything that compares two runs of this library -- averaging on and off, graph and eager,
straight and resumed, rank 0 and rank 1 -- is bit for bit."""
import os
import socket
import subprocess
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tail only | tail only | exactly one 16-byte vector | vector + tail | many blocks, tail 3 | many blocks, tail 1 | one element
# past ... a full pass of the launch's grid (4096 blocks x 256 lanes x 4 floats, + a tail of 3): the stride loop runs again
SIZES = [1, 3, 4, 5, 1023, 1025, 4 * 256 * 4096 + 7]
WEIGHTS = [1 - 0.999, 1 - 0.9, 0.5, 0.7]  # both branches of lerp (w < 0.5, w >= 0.5), and the boundary
PRECISIONS = ["32", "bf16-mixed"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _values(n, k, seed=0):
    gen = torch.Generator().manual_seed(2000 + n % 991 + seed)
    return [torch.randn(n, generator=gen) for _ in range(k)]


# ---------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_equals_torch_lerp(dev, n, w):
    import vit_amd.functional as vf

    e0, *ps = _values(n, 6)
    ema, twin = e0.to(dev), e0.to(dev)
    for s, p in enumerate(ps):
        p = p.to(dev)
        keep = p.clone()
        vf.ema_update(ema, p, w)
        twin = torch.lerp(twin, p, w)
        assert torch.equal(p, keep)  # p is only read
        e = rel(ema, twin)
        assert e < 1e-6, (s, e)
    assert not torch.equal(ema.cpu(), e0)


@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_weight_one_copies_and_weight_zero_keeps_every_bit(dev, n):
    import vit_amd.functional as vf

    e0, p = _values(n, 2)
    e0[0], p[-1] = float("inf"), -0.0  # p - (p - ema) * 0 would not be p here; a copy is
    ema, pd = e0.to(dev), p.to(dev)
    vf.ema_update(ema, pd, 0.0)
    assert torch.equal(ema.view(torch.int32).cpu(), e0.view(torch.int32))
    vf.ema_update(ema, pd, 1.0)
    assert torch.equal(ema, pd) and torch.equal(ema.view(torch.int32).cpu(), p.view(torch.int32))


@pytest.mark.parametrize("w", [1 - 0.9, 0.7])
def test_update_kernel_on_an_aligned_slice(dev, w):
    """A call on buffer[lo : lo + m] (lo a multiple of 4 elements, m with a scalar tail) leaves the guard bands on both sides
    bit-unchanged and gives, on the slice, the bits of the whole-buffer call."""
    import vit_amd.functional as vf

    n, lo, m = 1100, 8, 1021
    e0, p = _values(n, 2)
    whole, pd = e0.to(dev), p.to(dev)
    vf.ema_update(whole, pd, w)
    part = e0.to(dev)
    vf.ema_update(part[lo:lo + m], pd[lo:lo + m], w)
    assert torch.equal(part[:lo].cpu(), e0[:lo]) and torch.equal(part[lo + m:].cpu(), e0[lo + m:])
    assert torch.equal(part[lo:lo + m], whole[lo:lo + m])
    assert not torch.equal(part[lo:lo + m].cpu(), e0[lo:lo + m])


@pytest.mark.parametrize("n", [5, 1025, 4 * 256 * 4096 + 7])
def test_update_kernel_weight_from_device_memory_gives_the_by_value_bits(dev, n):
    import vit_amd.functional as vf

    e0, p = _values(n, 2)
    pd = p.to(dev)
    cell = torch.zeros(1, 4, dtype=torch.float32, device=dev)
    for w in (1 - 0.999, 0.7, 1.0, 0.0):
        by_value, from_cell = e0.to(dev), e0.to(dev)
        vf.ema_update(by_value, pd, w)
        vf.ema_weight_write(cell, w)
        vf.ema_update(from_cell, pd, 123.0, weight_dev=cell)  # the by-value argument is ignored (and not range-checked)
        assert torch.equal(by_value.view(torch.int32), from_cell.view(torch.int32)), w
        assert float(cell[0, 0]) == float(torch.tensor(w, dtype=torch.float32))


@pytest.mark.parametrize("n", SIZES)
def test_swap_kernel_exchanges_and_writes_the_shadow(dev, n):
    import vit_amd.functional as vf

    p0, e0 = _values(n, 2, seed=1)
    p, ema = p0.to(dev), e0.to(dev)
    shadow = vf.cast_f32_bf16(p)
    shadow0 = shadow.clone()
    vf.ema_swap(p, ema, shadow)
    assert torch.equal(p.cpu(), e0) and torch.equal(ema.cpu(), p0)
    assert torch.equal(shadow, vf.cast_f32_bf16(p)) and (n < 4 or not torch.equal(shadow, shadow0))
    vf.ema_swap(p, ema, shadow)
    assert torch.equal(p.cpu(), p0) and torch.equal(ema.cpu(), e0) and torch.equal(shadow, shadow0)
    vf.ema_swap(p, ema, None)  # no shadow (f32 mode)
    assert torch.equal(p.cpu(), e0) and torch.equal(ema.cpu(), p0) and torch.equal(shadow, shadow0)


# ----------------------------------------------------------------------------------------------------------- model level
def _c1(precision, **train):
    from test_trainer_gpu import c1_config

    return c1_config(precision=precision, batch_size=8, **train)


def _ready(cfg):
    from test_trainer_gpu import make

    module, trainer = make(cfg)
    trainer._setup(module)
    module.train()
    return module, trainer


class _Twin:
    """torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay) over clones of the run's own parameters: the twin
    is never trained, only handed the model's current values before each update."""

    def __init__(self, params, decay):
        from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

        self.src = params
        self.holder = torch.nn.Module()
        self.holder.ps = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in params])
        self.avg = AveragedModel(self.holder, multi_avg_fn=get_ema_multi_avg_fn(decay))

    def update(self):
        with torch.no_grad():
            for tw, p in zip(self.holder.ps, self.src):
                tw.copy_(p.detach())
        self.avg.update_parameters(self.holder)

    def averaged(self):
        return [p.detach() for p in self.avg.module.ps]


def _averaged_params(trainer, module):
    """The averager's values in model.named_parameters() order."""
    sd = trainer.averager.averaged_state_dict(module.model)
    return [(name, sd[name]) for name, _ in module.model.named_parameters()]


def _assert_twin(trainer, module, twin, step):
    for (name, got), want in zip(_averaged_params(trainer, module), twin.averaged()):
        e = rel(got, want)
        assert e < 2e-6, (step, name, e)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_training_trajectory_is_untouched_and_average_equals_averaged_model(dev, precision):
    """(a) averaging reads the parameters and writes nothing the training path reads: losses and final weights of a run with
    `ema_decay` are those of a run without, bit for bit.  (b) after each of 6 steps the averaged weights are the twin's."""
    from test_trainer_gpu import Batches

    batches = [tuple(t.cuda() for t in b) for b in Batches(48, 5, bs=8)]
    runs = {}
    for ema in (False, True):
        module, trainer = _ready(_c1(precision, **({"ema_decay": 0.9} if ema else {})))
        assert (trainer.averager is not None) == ema
        twin = _Twin(list(module.model.parameters()), 0.9) if ema else None
        losses = []
        for i, b in enumerate(batches):
            losses.append(float(trainer.training_step(module, b, i).detach()))
            if ema:
                twin.update()
                assert trainer.averager.n_averaged == i + 1
                _assert_twin(trainer, module, twin, i)
        runs[ema] = (losses, module.model.engine.flat.detach().clone())
        if ema:
            n = module.model.engine.layout.n_trainable
            moved = rel(trainer.averager.flat[:n], module.model.engine.flat[:n])
            assert moved > 1e-4, moved  # the average lags the weights visibly
    assert runs[False][0] == runs[True][0], (runs[False][0], runs[True][0])
    assert torch.equal(runs[False][1], runs[True][1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_and_start_step_follow_the_schedule(dev, precision):
    """ema_every 2, ema_start_step 3: updates after steps 5 and 7 (the first is the copy), nothing before or between."""
    from test_trainer_gpu import Batches

    batches = [tuple(t.cuda() for t in b) for b in Batches(64, 5, bs=8)]
    module, trainer = _ready(_c1(precision, ema_decay=0.9, ema_every=2, ema_start_step=3))
    twin = _Twin(list(module.model.parameters()), 0.9)
    want = [0, 0, 0, 0, 1, 1, 2, 2]
    for i, b in enumerate(batches):
        trainer.training_step(module, b, i)
        if want[i] != (want[i - 1] if i else 0):
            twin.update()
        assert trainer.averager.n_averaged == want[i], (i, trainer.averager.n_averaged)
        if want[i]:
            _assert_twin(trainer, module, twin, i)
    assert trainer.global_step == 8


def test_accumulated_micro_batches_average_once_per_optimizer_step(dev):
    from test_trainer_gpu import Batches

    batches = [tuple(t.cuda() for t in b) for b in Batches(48, 5, bs=8)]
    module, trainer = _ready(_c1("32", ema_decay=0.9, accumulate_grad_batches=2))
    twin = _Twin(list(module.model.parameters()), 0.9)
    for i, b in enumerate(batches):
        trainer.training_step(module, b, i, is_last=(i == len(batches) - 1))
        if i % 2 == 1:
            twin.update()
        assert trainer.averager.n_averaged == (i + 1) // 2
    assert trainer.averager.n_averaged == 3 and trainer.global_step == 3
    _assert_twin(trainer, module, twin, 5)


# ------------------------------------------------------------------------------------------- validation, checkpoints, resume
def _val_logs(logs, prefix="val_"):
    return {k: v for k, v in logs.items() if k.startswith(prefix)}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_validation_sees_the_average_and_puts_the_weights_back(dev, precision):
    """fit()'s validation logs are those of a fresh model loaded with the averaged weights; the bracket around validate()
    restores every bit (the run continues like one without averaging: raw weights and bf16 shadow after 2 epochs, the second
    trained behind a validation); after fit() the model holds the average, and test() without a checkpoint reports it."""
    from test_trainer_gpu import Batches, make

    train, val = Batches(32, 1, bs=8), Batches(16, 2, bs=8, four=True)
    module, trainer = make(_c1(precision, ema_decay=0.9))
    hist = trainer.fit(module, train, val)
    avg, eng = trainer.averager, module.model.engine
    assert len(hist) == 2 and avg.n_averaged == 8 and avg.swapped
    averaged = avg.averaged_state_dict(module.model)
    for k, v in module.model.state_dict().items():
        assert torch.equal(v.cpu(), averaged[k]), k  # the model holds the averaged weights
    fresh, t2 = make(_c1(precision), seed=7)
    fresh.model.load_state_dict(averaged)
    t2._setup(fresh, for_training=False)
    want = t2.validate(fresh, val)
    got = _val_logs(hist[-1])
    assert got and got == _val_logs(want), (got, want)
    # test() with no checkpoint: the averaged model's metrics
    assert _val_logs(trainer.test(module, val), "test_") == _val_logs(t2.test(fresh, val), "test_")
    # the same run without averaging: its weights are this run's raw weights, which a swap brings back
    plain_m, plain_t = make(_c1(precision))
    plain_hist = plain_t.fit(plain_m, train, val)
    assert _val_logs(plain_hist[-1]) != got  # the raw model validates differently: the average really was what fit() validated
    avg.swap(eng)
    assert not avg.swapped and torch.equal(eng.flat, plain_m.model.engine.flat)
    if precision == "bf16-mixed":
        assert torch.equal(eng.shadow, plain_m.model.engine.shadow)
    assert [h["mae_loss"] for h in hist] == [h["mae_loss"] for h in plain_hist]


def test_second_fit_swaps_the_training_weights_back_first(dev):
    """fit() leaves the average in the model; a following fit() on the same trainer continues from the raw weights: two fits of
    one epoch are one fit of two (the epoch counter restarts, so the comparison is through epoch-independent state)."""
    from test_trainer_gpu import Batches, make

    train, val = Batches(32, 1, bs=8), Batches(16, 2, bs=8)
    module, trainer = make(_c1("bf16-mixed", ema_decay=0.9, ep=1))
    trainer.fit(module, train, val)
    assert trainer.averager.swapped
    raw = trainer.averager.train_state_dict()
    seen = {}
    step0 = module.training_step

    def spy(batch, idx):
        seen.setdefault("flat", {k: v.detach().cpu().clone() for k, v in module.model.state_dict().items()})
        return step0(batch, idx)

    module.training_step = spy
    trainer.fit(module, train, val)
    assert trainer.averager.swapped and trainer.averager.n_averaged == 8 and trainer.global_step == 8
    for k, v in seen["flat"].items():
        assert torch.equal(v, raw[k]), k  # the second fit's first step saw the raw weights, not the average


def test_checkpoint_holds_the_average_and_resume_continues_both_sequences(dev, tmp_path, monkeypatch):
    from test_trainer_gpu import Batches, make
    from vit_amd.trainer import load_checkpoint_file, model_state_from_checkpoint

    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "ck"))
    train, val = Batches(24, 1, bs=8), Batches(16, 2, bs=8)
    kw = dict(ema_decay=0.9, ema_every=2, ema_start_step=1)
    m_full, t_full = make(_c1("bf16-mixed", ep=4, save=False, **kw))
    t_full.fit(m_full, train, val)
    m_a, t_a = make(_c1("bf16-mixed", ep=2, save=True, **kw))
    t_a.fit(m_a, train, val)
    raw = load_checkpoint_file(t_a.checkpointer.last_path)  # weights_only=True loader
    own = raw["vit_amd"]
    assert own["version"] == 2 and set(own["ema"]) == {"decay", "every", "start_step", "n_averaged", "train_state"}
    assert (own["ema"]["decay"], own["ema"]["every"], own["ema"]["start_step"]) == (0.9, 2, 1)
    assert own["ema"]["n_averaged"] == t_a.averager.n_averaged == 2  # after steps 3 and 5 of 6
    averaged, trained = t_a.averager.averaged_state_dict(m_a.model), t_a.averager.train_state_dict()
    ck_sd = model_state_from_checkpoint(raw)
    assert set(ck_sd) == set(averaged) == set(own["ema"]["train_state"])
    for k in averaged:
        assert torch.equal(ck_sd[k], averaged[k]), k
        assert torch.equal(own["ema"]["train_state"][k], trained[k]), k
    assert any(not torch.equal(averaged[k], trained[k]) for k in averaged)
    m_b, t_b = make(_c1("bf16-mixed", ep=4, save=False, **kw))
    hist = t_b.fit(m_b, train, val, ckpt_path=t_a.checkpointer.last_path)
    assert len(hist) == 2 and t_b.global_step == 12 and t_b.averager.n_averaged == t_full.averager.n_averaged == 5
    for which in ("averaged_state_dict", "train_state_dict"):
        a, b = getattr(t_full.averager, which)(), getattr(t_b.averager, which)()
        for k in a:
            assert torch.equal(a[k], b[k]), (which, k)
    assert [h["val_mae"] for h in t_full.history[2:]] == [h["val_mae"] for h in hist]


def test_checkpoint_without_averaging_has_no_ema_entry(dev, tmp_path, monkeypatch):
    from test_trainer_gpu import Batches, make
    from vit_amd.trainer import load_checkpoint_file

    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "ck"))
    module, trainer = make(_c1("32", ep=1, save=True))
    trainer.fit(module, Batches(16, 1, bs=8), Batches(8, 2, bs=8))
    raw = load_checkpoint_file(trainer.checkpointer.last_path)
    assert set(raw["vit_amd"]) == {"version", "dropout_base_seed", "dropout_step"} and raw["vit_amd"]["version"] == 2
    for k, v in module.model.state_dict().items():
        assert torch.equal(raw["state_dict"]["model." + k], v.cpu()), k
    # averaging configured but not begun (ema_start_step beyond the run): still today's layout, and nothing is swapped
    module, trainer = make(_c1("32", ep=1, save=True, ema_decay=0.9, ema_start_step=100))
    trainer.fit(module, Batches(16, 1, bs=8), Batches(8, 2, bs=8))
    raw = load_checkpoint_file(trainer.checkpointer.last_path)
    assert "ema" not in raw["vit_amd"] and trainer.averager.n_averaged == 0 and not trainer.averager.swapped


# ------------------------------------------------------------------------------------------------------- the captured step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_graph_with_averaging_equals_eager(dev, precision):
    """The update rides in the captured step as its last node; its weight (0 / 1 / 1 - decay) is rewritten in a device cell ahead
    of a replay.  Dropout off (as test_hip_graph_step_equals_eager), ema_every 2: five steps, updates after steps 2 and 4."""
    from test_trainer_gpu import Batches, make
    from vit_amd.graph import GraphedTrainStep

    batches = [tuple(t.cuda() for t in b) for b in Batches(16, 5, bs=8)]
    finals = {}
    for mode in ("eager", "graph"):
        module, trainer = make(_c1(precision, hip_graph=(mode == "graph"), ema_decay=0.9, ema_every=2))
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            losses = [float(trainer.training_step(module, batches[i % 2], i).detach()) for i in range(5)]
        assert not [w for w in caught if "hip_graph" in str(w.message)], [str(w.message) for w in caught]
        assert trainer.use_graph == (mode == "graph") and trainer.global_step == 5 and trainer.averager.n_averaged == 2
        if mode == "graph":
            assert len(trainer._graphed) == 1 and all(isinstance(g, GraphedTrainStep) for g in trainer._graphed.values())
        n = module.model.engine.layout.n_trainable
        finals[mode] = (losses, module.model.engine.flat.detach().clone(), trainer.averager.flat[:n].detach().clone())
    assert finals["eager"][0] == finals["graph"][0], (finals["eager"][0], finals["graph"][0])
    assert torch.equal(finals["eager"][1], finals["graph"][1])
    assert torch.equal(finals["eager"][2], finals["graph"][2])
    assert not torch.equal(finals["graph"][2], finals["graph"][1][:finals["graph"][2].numel()])


# ------------------------------------------------------------------------------------------- a trainable input preprocessor
def test_trainable_preprocessor_is_averaged_and_swapped_with_the_rest(dev, tmp_path):
    """A ZCA front end (48 x 48, trainable from the start) lives outside the flat buffer: the optimizer's `_extras`.  The same
    kernels run on its storage: its matrix and bias follow the twin, and a swap exchanges them with the rest."""
    from test_trainer_gpu import make

    L = 48
    gen = torch.Generator().manual_seed(5)
    q, _ = torch.linalg.qr(torch.randn(L, L, generator=gen))
    cov_path = tmp_path / "cov.pt"
    torch.save({"eigvecs": q.contiguous(), "eigvals": torch.logspace(0, -2, L), "mean": 0.01 * torch.randn(L, generator=gen)}, cov_path)
    cfg = _c1("32", ema_decay=0.9)
    cfg["model"].update(image_size=L, patch_size=8, stride_size=8)
    cfg["warmup"] = dict(preprocessor="zca", cov_path=str(cov_path), shrinkage=0.1, freeze_epochs=0)
    module, trainer = make(cfg)
    trainer._setup(module)
    module.train()
    pre = module.model.preprocessor
    assert pre.linear.weight.shape == (L, L) and isinstance(pre.linear.weight, torch.nn.Parameter)
    assert len(trainer.optimizer._extras) == 2 and len(trainer.averager.extras) == 2
    twin = _Twin(list(module.model.parameters()), 0.9)
    w0 = pre.linear.weight.detach().clone()
    for i in range(3):
        b = (torch.randn(8, L, generator=gen).cuda(), torch.rand(8, L, generator=gen).cuda(), torch.rand(8, generator=gen).cuda())
        trainer.training_step(module, b, i)
        twin.update()
        _assert_twin(trainer, module, twin, i)
    assert not torch.equal(pre.linear.weight.detach(), w0)  # the matrix trains
    averaged, trained = trainer.averager.averaged_state_dict(module.model), trainer.averager.train_state_dict()
    assert not torch.equal(averaged["preprocessor.linear.weight"], trained["preprocessor.linear.weight"])
    trainer.averager.swap(module.model.engine)
    held = {k: v.detach().cpu() for k, v in module.model.state_dict().items()}
    for k in averaged:
        assert torch.equal(held[k], averaged[k]), k
    assert torch.equal(trainer.averager.extra_bufs[0].view(L, L).cpu(), trained["preprocessor.linear.weight"])
    trainer.averager.swap(module.model.engine)
    for k, v in module.model.state_dict().items():
        assert torch.equal(v.detach().cpu(), trained[k]), k


# -------------------------------------------------------------------------------------------------------- data parallelism
def _ranks(tmp_path, world, exchanges):
    child = os.path.join(ROOT, "tests", "_ema_ddp_child.py")
    out = tmp_path / f"w{world}"
    out.mkdir()
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "VIT_DIST_SINGLE", "VIT_DIST_BACKEND")}
    procs = []
    if world == 1:
        envs = [base]
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        envs = [dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
                     MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), VIT_DIST_BACKEND="gloo") for r in range(world)]
        for env in envs:
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for env in envs:
        procs.append(subprocess.Popen([sys.executable, child, str(out), *exchanges], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0] * world, "\n".join(o[-2000:] for o in outs)
    return [torch.load(out / f"rank{r}.pt", weights_only=True) for r in range(world)]


def test_ema_under_data_parallelism(tmp_path):
    """Two gloo ranks on the one GPU, under `allreduce` and under `zero1`: every rank averages the full buffer (no collective,
    nothing sharded), so the averages are bit-identical across ranks; against the single-process run on the whole batch they
    agree like the parameters do (the bounds of test_ddp_gpu.py::test_two_ranks_average_equals_single_process_on_full_batch)."""
    single = _ranks(tmp_path, 1, ["allreduce"])[0]["allreduce"]
    two = _ranks(tmp_path, 2, ["allreduce", "zero1"])
    n = single["n_trainable"]
    assert single["world"] == 1 and single["n_averaged"] == 3
    for ex in ("allreduce", "zero1"):
        r0, r1 = two[0][ex], two[1][ex]
        assert r0["mode"] == ex and r0["world"] == 2 and r0["n_averaged"] == r1["n_averaged"] == 3
        assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["ema"], r1["ema"]), ex
        assert not torch.equal(r0["ema"][:n], r0["params"][:n])
        d = (single["ema"][:n].double() - r1["ema"][:n].double()).abs()
        agree = float((d < 1e-5).double().mean())
        print(f"[ema ddp {ex}] max |d ema| vs single process {float(d.max()):.3e}, agree on {agree:.4%}")
        assert float(d.max()) <= 2.1e-3 and agree > 0.999, (ex, float(d.max()), agree)
    assert torch.equal(two[0]["allreduce"]["ema"][:n], two[0]["zero1"]["ema"][:n])
