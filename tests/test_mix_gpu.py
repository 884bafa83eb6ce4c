"""Mixup / CutMix on the GPU (include/vit_amd_mix.h, vit_amd/mix.py): the signal and target kernels against the float64 yardstick
of tests/_mix_ref.py, the soft-target head losses against torch, one training step against the CPU oracle, and the trainer's
use of the mixer (off path, captured step, resume, accumulation, snapshot).

Bounds.  A mixed element is fma(w, x_b, u * x_p) (or a product, a product and a sum): at most three f32 roundings, each at most
2^-24 relative to a quantity no larger than |w x_b| + |u x_p|, so |out - ref64| <= 2^-22 (|w x_b| + |u x_p|) with room for either
form.  Everything else is a bit copy.  The soft losses are held to the figure tests/test_kernels_gpu.py::test_head_loss holds
the hard ones to (relative 1e-5: the same arithmetic class), the model-level step to the eval-mode gates of
tests/test_parity_gpu.py for the same precision."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mix_ref as ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -22
GUARD = 64  # floats on both sides of an output
PRECISIONS = ["32", "bf16-mixed"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int32)


def f32(v):
    return ref.f32(v)


def plan_rows(L):
    """identity, Mixup w = 0.37, an empty span, the full span, a span across a vector boundary, one across a chunk boundary
    (L = 4096: elements 2047 .. 2053 straddle chunk 7 | 8 of 256; L = 203: the rows are not 16-byte multiples at all)."""
    w = f32(0.37)
    return [ref.IDENTITY, (w, f32(1.0 - 0.37), 0, 0, w, f32(1.0 - 0.37)), (1.0, 0.0, 7, 7, 1.0, 0.0),
            (1.0, 0.0, 0, L, 0.0, 1.0), (1.0, 0.0, 3, 10, f32(1 - 7 / L), f32(7 / L)),
            (1.0, 0.0, L // 2 - 1, L // 2 + 6, f32(1 - 7 / L), f32(7 / L))]


def device_plan(dev, rows):
    import vit_amd.functional as vf

    plan = torch.zeros(len(rows) * vf.MIX_ROW_BYTES, dtype=torch.uint8, device=dev)
    vf.mix_plan_write(plan, rows)
    return plan


def guarded(dev, shape, fill=None):
    """A tensor of `shape` inside a buffer with GUARD floats of a known pattern on both sides (16-byte aligned: 256 bytes)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), -12345.0, device=dev)
    view = buf[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == -12345.0).all() and (buf[-GUARD:] == -12345.0).all())


def check_signal(x_host, out, rows, tag):
    want, kind, bound = ref.mix_signal(x_host.numpy(), rows)
    B = x_host.shape[0]
    got = out.cpu()
    partner = x_host.flip(0)
    k = torch.from_numpy(kind)
    own_ok = bits(got)[k == 0] == bits(x_host)[k == 0]
    par_ok = bits(got)[k == 1] == bits(partner)[k == 1]
    assert bool(own_ok.all()), f"{tag}: {int((~own_ok).sum())} elements that are the sample's own are not bit copies"
    assert bool(par_ok.all()), f"{tag}: {int((~par_ok).sum())} span elements are not the partner's bits"
    err = (got.double() - torch.from_numpy(want)).abs()[k == 2]
    lim = EPS * torch.from_numpy(bound)[k == 2]
    assert bool((err <= lim).all()), (tag, float((err / lim.clamp_min(1e-300)).max()))
    if B % 2:  # the middle row is its own partner
        assert torch.equal(bits(got[B // 2]), bits(x_host[B // 2])), tag
    return float((err / lim.clamp_min(1e-300)).max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------ vit_mix_signal
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("L", [203, 4096])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_mix_signal_against_the_yardstick(dev, B, L, inplace, per_sample):
    import vit_amd.functional as vf

    gen = torch.Generator().manual_seed(100 + B + L)
    x_host = torch.randn(B, L, generator=gen)
    base = plan_rows(L)
    worst = 0.0
    for v in range(len(base)):
        rows = [base[(v + b) % len(base)] for b in range(B)] if per_sample else [base[v]]
        plan = device_plan(dev, rows)
        xbuf, x = guarded(dev, (B, L), x_host)
        if inplace:
            out = vf.mix_signal(x, plan, len(rows), out=x)
            assert out is x and guards_intact(xbuf)
        else:
            obuf, o = guarded(dev, (B, L))
            out = vf.mix_signal(x, plan, len(rows), out=o)
            assert guards_intact(obuf) and guards_intact(xbuf)
            assert torch.equal(bits(x.cpu()), bits(x_host)), "the copy form changed x"
        worst = max(worst, check_signal(x_host, out, rows, f"B={B} L={L} inplace={inplace} per_sample={per_sample} v={v}"))
    print(f"[mix_signal B={B} L={L} inplace={inplace} per_sample={per_sample}] worst mixed |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("L", [203, 4096])
def test_identity_rows_do_not_read_their_partner(dev, L, inplace):
    """Row 0 is the identity, its partner row is all NaN (and is itself mixed / cut): out[0] is x[0], bit for bit."""
    import vit_amd.functional as vf

    gen = torch.Generator().manual_seed(7)
    for B, other in ((2, plan_rows(L)[1]), (2, plan_rows(L)[5]), (5, plan_rows(L)[1])):
        x_host = torch.randn(B, L, generator=gen)
        x_host[B - 1] = float("nan")
        rows = [ref.IDENTITY] + [other] * (B - 1)
        x = x_host.to(dev)
        out = vf.mix_signal(x, device_plan(dev, rows), B, out=x if inplace else None)
        assert torch.equal(bits(out[0].cpu()), bits(x_host[0]))
        assert bool(torch.isfinite(out[0]).all())
    # a one-row identity plan: nothing of any partner reaches any row
    x_host = torch.randn(2, L, generator=gen)
    x_host[1] = float("nan")
    x = x_host.to(dev)
    out = vf.mix_signal(x, device_plan(dev, [ref.IDENTITY]), 1, out=x if inplace else None)
    assert torch.equal(bits(out.cpu()), bits(x_host))


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("L", [203, 4096])
def test_out_of_range_span_is_clamped(dev, L, inplace):
    import vit_amd.functional as vf

    B = 5
    x_host = torch.randn(B, L, generator=torch.Generator().manual_seed(9))
    xbuf, x = guarded(dev, (B, L), x_host)
    obuf, o = guarded(dev, (B, L))
    out = vf.mix_signal(x, device_plan(dev, [(1.0, 0.0, -5, L + 9, 0.0, 1.0)]), 1, out=x if inplace else o)
    assert torch.equal(bits(out.cpu()), bits(x_host.flip(0)))  # as [0, L): every row is its partner
    assert guards_intact(xbuf) and guards_intact(obuf)


# ------------------------------------------------------------------------------------------------------------ vit_mix_targets
def target_rows(B):
    w = f32(0.37)
    pool = [(w, f32(1 - 0.37), 0, 0, w, f32(1 - 0.37)), ref.IDENTITY, (1.0, 0.0, 3, 10, f32(0.75), f32(0.25)),
            (1.0, 0.0, 7, 7, 1.0, 0.0), (1.0, 0.0, 0, 99, 0.0, 1.0)]
    return [pool[b % len(pool)] for b in range(B)]


def check_targets(got, want, bound, copied, tag):
    got = got.double().cpu().reshape(want.shape)
    want_t, lim = torch.from_numpy(want), EPS * torch.from_numpy(bound)
    for b in range(want.shape[0]):
        if copied[b]:
            assert torch.equal(got[b].float(), want_t[b].float()), f"{tag}: row {b} (uy == 0) is not a bit copy"
        else:
            assert bool(((got[b] - want_t[b]).abs() <= lim[b]).all()), (tag, b)


@pytest.mark.parametrize("k", [1, 3])
def test_mix_targets_regression(dev, k):
    import vit_amd.functional as vf

    B = 5
    y_host = torch.rand(B, k, generator=torch.Generator().manual_seed(20 + k))
    for rows in (target_rows(B), [target_rows(B)[0]], [ref.IDENTITY]):
        want, bound, copied = ref.mix_targets_reg(y_host.numpy(), rows)
        obuf, o = guarded(dev, (B, k))
        got = vf.mix_targets(y_host.to(dev), device_plan(dev, rows), len(rows), out=o)
        check_targets(got, want, bound, copied, f"reg k={k} rows={len(rows)}")
        assert guards_intact(obuf)
    y1 = y_host[:, 0].contiguous().to(dev)  # labels [B] keep their shape
    assert vf.mix_targets(y1, device_plan(dev, [ref.IDENTITY]), 1).shape == (B,)


@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("C", [1, 7, 1000])
def test_mix_targets_classes(dev, C, s):
    import vit_amd.functional as vf

    B = 5
    y_host = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(30 + C))
    on, off = ref.on_off(s, C)
    for rows in (target_rows(B), [target_rows(B)[0]], [ref.IDENTITY]):
        want, bound, copied = ref.mix_targets_cls(y_host.numpy(), rows, C, s)
        obuf, o = guarded(dev, (B, C))
        got = vf.mix_targets(y_host.to(dev), device_plan(dev, rows), len(rows), C, on, off, out=o)
        check_targets(got, want, bound, copied, f"cls C={C} s={s} rows={len(rows)}")
        assert guards_intact(obuf)
        assert float((got.double().sum(1) - 1.0).abs().max()) < 1e-5
    # one label equal to C: no `on` entry anywhere in its own row, nothing outside `out` is touched
    y_bad = y_host.clone()
    y_bad[1] = C
    obuf, o = guarded(dev, (B, C))
    got = vf.mix_targets(y_bad.to(dev), device_plan(dev, [ref.IDENTITY]), 1, C, on, off, out=o).cpu()
    assert guards_intact(obuf)
    assert torch.equal(got[1], torch.full((C,), float(np.float32(off))))
    assert torch.equal(got, torch.from_numpy(ref.one_hot(y_bad.numpy(), C, on, off)).float())


# ------------------------------------------------------------------------------------------------------------ soft losses
def soft_targets(B, C, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.rand(B, C, generator=gen) + 0.01
    return t / t.sum(1, keepdim=True)


def torch_soft_loss(kind, lg, t):
    return F.cross_entropy(lg, t) if kind == "soft_ce" else F.binary_cross_entropy_with_logits(lg, t)


@pytest.mark.parametrize("kind", ["soft_ce", "bce"])
@pytest.mark.parametrize("B,C", [(3, 1), (37, 7), (4, 1000), (300, 10)])
def test_soft_head_loss(dev, kind, B, C):
    """As test_kernels_gpu.py::test_head_loss: forward and backward through vf.head_loss_fwd / _bwd against torch, dloss = 1.7.
    (4, 1000): more than one stride per lane, not a multiple of 64; (300, 10): more rows than the final reduce's block."""
    import vit_amd.functional as vf
    from test_kernels_gpu import randn
    from vit_amd._cabi import LOSS_BCE, LOSS_SOFT_CE

    T, D = 6, 192
    code = LOSS_SOFT_CE if kind == "soft_ce" else LOSS_BCE
    last = randn((B, T, D), dev, 60)
    W, b = randn((C, D), dev, 61, 0.1), randn((C,), dev, 62, 0.1)
    t = soft_targets(B, C, 63).to(dev)
    if kind == "bce":
        t = (t * min(C, 3)).clamp(0, 1)  # BCE targets need not sum to 1
    logits, loss = vf.head_loss_fwd(last, W, b, t, code)
    l32 = last.clone().requires_grad_(True)
    W32, b32 = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lg = F.linear(l32[:, 0], W32, b32)
    want = torch_soft_loss(kind, lg, t)
    print(f"[{kind} B={B} C={C}] loss {loss.item():.7f} torch {want.item():.7f}")
    assert rel(logits, lg) < 1e-5 and abs(loss.item() - want.item()) < 1e-5 * max(1, abs(want.item()))
    (want * 1.7).backward()
    dloss = torch.full((1,), 1.7, device=dev)
    dlast, dW, db = vf.head_loss_bwd(last, W, logits, t, dloss, code)
    errs = (rel(dlast, l32.grad), rel(dW, W32.grad), rel(db, b32.grad))
    print(f"[{kind} B={B} C={C}] rel errors dlast {errs[0]:.2e} dW {errs[1]:.2e} db {errs[2]:.2e}")
    assert max(errs) < 1e-5, errs
    # a second run is bit-identical
    logits2, loss2 = vf.head_loss_fwd(last, W, b, t, code)
    again = vf.head_loss_bwd(last, W, logits2, t, dloss, code)
    assert torch.equal(loss, loss2) and torch.equal(logits, logits2)
    assert all(torch.equal(a, c) for a, c in zip((dlast, dW, db), again))


@pytest.mark.parametrize("B,C", [(37, 7), (4, 1000)])
def test_one_hot_targets_through_soft_ce_give_the_hard_ce_loss(dev, B, C):
    import vit_amd.functional as vf
    from test_kernels_gpu import randn
    from vit_amd._cabi import LOSS_CE, LOSS_SOFT_CE

    last = randn((B, 6, 192), dev, 60)
    W, b = randn((C, 192), dev, 61, 0.1), randn((C,), dev, 62, 0.1)
    y = torch.randint(0, C, (B,), device=dev)
    _, hard = vf.head_loss_fwd(last, W, b, y, LOSS_CE)
    _, soft = vf.head_loss_fwd(last, W, b, F.one_hot(y, C).float(), LOSS_SOFT_CE)
    assert abs(soft.item() - hard.item()) < 1e-5 * max(1, abs(hard.item())), (soft.item(), hard.item())


@pytest.mark.parametrize("kind", ["soft_ce", "bce"])
def test_soft_head_loss_bwd_accumulates_into_dW_and_db(dev, kind):
    import vit_amd.functional as vf
    from test_accum_gpu import writer_contract
    from test_kernels_gpu import randn
    from vit_amd._cabi import LOSS_BCE, LOSS_SOFT_CE

    B, T, D, C = 37, 6, 192, 7
    code = LOSS_SOFT_CE if kind == "soft_ce" else LOSS_BCE
    last = randn((B, T, D), dev, 60)
    W, b = randn((C, D), dev, 61, 0.1), randn((C,), dev, 62, 0.1)
    t = soft_targets(B, C, 64).to(dev)
    logits, _ = vf.head_loss_fwd(last, W, b, t, code)
    dloss = torch.full((1,), 1.7, device=dev)
    dlast, dW, db = torch.empty_like(last), torch.empty_like(W), torch.empty_like(b)
    writer_contract(dev, lambda: vf.head_loss_bwd(last, W, logits, t, dloss, code, dlast=dlast, dW=dW, db=db), [dW, db],
                    f"head_loss_bwd {kind}")


# ------------------------------------------------------------------------------------------------------------ model level
def model_config(task, precision, augment, **model):
    return {
        "model": dict(name="vit", task_type=task, image_size=512, patch_size=32, hidden_size=32, num_hidden_layers=1,
                      num_attention_heads=2, stride_size=32, proj_fn="SW", **model),
        "train": dict(batch_size=6, ep=1, precision=precision),
        "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0},
        "augment": augment,
    }


def run_step_against_oracle(dev, cfg, rows, precision, soft=None):
    """One eager training forward + backward of the module on a fixed plan, against oracle.refvit.forward on the yardstick's
    mixed input with the soft loss formed here in torch.  Gates: the eval-mode ones of tests/test_parity_gpu.py for the
    precision ('32': 1e-4 forward, 2e-4 per gradient tensor; bf16-mixed: logits 2e-2, loss 3e-2 relative + 1e-4, gradients
    4e-2 with cosine > 0.999).  Dropout off, the way that file's gradient tests run."""
    from oracle import refvit
    from vit_amd.module import ViTLModule

    rc = refvit.config_from_dict(cfg)
    B, L, C = 6, rc.image_size, rc.num_labels
    sd = refvit.make_state_dict(rc, 11)
    flux, error, labels = refvit.make_inputs(rc, B, 12)
    module = ViTLModule(config=cfg)
    module.model.load_state_dict(sd, strict=True)
    module.to(dev)
    module.model.set_precision(precision)
    module.model.config.hidden_dropout_prob = 0.0
    module.model.config.attention_probs_dropout_prob = 0.0
    module.train()
    assert module.mixer is not None
    module.mixer.draw = lambda b, l: rows  # the fixed plan
    loss = module.training_step((flux.to(dev), error.to(dev), labels.to(dev)), 0)
    loss.backward()
    assert module.mixer.last_rows == rows
    # the oracle on the yardstick's mixed batch
    x_mix = torch.from_numpy(ref.mix_signal(flux.numpy(), rows)[0]).float()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = refvit.forward(rc, params, x_mix, labels=None, training=False)
    if soft is None:
        y_mix = torch.from_numpy(ref.mix_targets_reg(labels.numpy(), rows)[0]).float()
        want = refvit.loss_fn(rc, out.logits, y_mix)
    else:
        t_mix = torch.from_numpy(ref.mix_targets_cls(labels.numpy(), rows, C, cfg["augment"].get("label_smoothing", 0.0))[0]).float()
        want = torch_soft_loss(soft, out.logits.view(-1, C), t_mix)
    want.backward()
    tight = precision == "32"
    e_loss = abs(float(loss) - float(want))
    print(f"[{cfg['model']['task_type']} {soft} {precision}] loss {float(loss):.6f} oracle {float(want):.6f}")
    assert e_loss <= (2e-4 if tight else 3e-2) * abs(float(want)) + (1e-5 if tight else 1e-4)
    gtol, worst = (2e-4 if tight else 4e-2), 0.0
    for name, p in module.model.named_parameters():
        g = params[name].grad
        if g is None or float(g.norm()) < 1e-6:
            continue
        mine = p.grad.detach().cpu().reshape(g.shape)
        e = rel(mine, g)
        cos = float(torch.dot(mine.double().flatten(), g.double().flatten()) / (mine.double().norm() * g.double().norm() + 1e-30))
        assert e < gtol and cos > 0.999, (name, e, cos)
        worst = max(worst, e)
    print(f"[{cfg['model']['task_type']} {soft} {precision}] worst gradient rel err {worst:.2e}")
    return module


@pytest.mark.parametrize("precision", PRECISIONS)
def test_training_step_regression_mixup_against_the_oracle(dev, precision):
    w = f32(0.37)
    rows = [(w, f32(1 - 0.37), 0, 0, w, f32(1 - 0.37))]
    run_step_against_oracle(dev, model_config("reg", precision, dict(mixup_alpha=0.8)), rows, precision)


@pytest.mark.parametrize("soft", ["ce", "bce"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_training_step_classes_cutmix_smoothing_against_the_oracle(dev, precision, soft):
    L = 512
    rows = [(1.0, 0.0, 100, 300, f32(1 - 200 / L), f32(200 / L))]
    cfg = model_config("cls", precision, dict(cutmix_alpha=1.0, label_smoothing=0.1, soft_loss=soft), num_labels=5)
    module = run_step_against_oracle(dev, cfg, rows, precision, soft="soft_ce" if soft == "ce" else "bce")
    # validation on the same module with int64 labels still reports plain cross-entropy
    from oracle import refvit

    rc = refvit.config_from_dict(cfg)
    flux, error, labels = refvit.make_inputs(rc, 6, 13)
    module.eval()
    with torch.no_grad():
        out = module.model(flux.to(dev), labels=labels.to(dev))
    want = F.cross_entropy(out.logits.float().cpu(), labels)
    assert abs(float(out.loss) - float(want)) < 1e-5 * max(1.0, float(want))
    assert module.loss_name == "ce" and module.mixer.n == 0  # the fixed plan drew nothing; evaluation never mixes


# ------------------------------------------------------------------------------------------------------------ trainer
MIXING = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", seed=5)


def _cfg(precision="32", augment=None, **train):
    from test_trainer_gpu import c1_config

    cfg = c1_config(precision=precision, batch_size=8, **train)
    if augment is not None:
        cfg["augment"] = augment
    return cfg


def test_off_path_all_zero_block_equals_no_block(dev):
    """(a) A 2-epoch fit with `augment` all zero is the fit without the block: losses and final weights bit for bit."""
    from test_trainer_gpu import Batches, make

    runs = []
    for augment in (None, dict(mixup_alpha=0, cutmix_alpha=0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.0)):
        module, trainer = make(_cfg("32", augment, ep=2))
        assert module.mixer is None
        hist = trainer.fit(module, Batches(24, 1, bs=8), Batches(8, 2, bs=8))
        runs.append(([(h["mae_loss"], h["val_mae"]) for h in hist], module.model.engine.flat.detach().clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_graph_with_mixing_equals_eager(dev, precision):
    """(b) Set up as test_ema_gpu.py::test_hip_graph_with_averaging_equals_eager: dropout off, five steps over two batches.
    The mix launches are the copy into the captured step's static buffers; the dataset tensors stay what they were."""
    from test_trainer_gpu import Batches, make
    from vit_amd.graph import GraphedTrainStep

    batches = [tuple(t.cuda() for t in b) for b in Batches(16, 5, bs=8)]
    before = [tuple(t.clone() for t in b) for b in batches]
    finals = {}
    for mode in ("eager", "graph"):
        module, trainer = make(_cfg(precision, dict(MIXING), hip_graph=(mode == "graph")))
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            losses = [float(trainer.training_step(module, batches[i % 2], i).detach()) for i in range(5)]
        assert not [w for w in caught if "hip_graph" in str(w.message)], [str(w.message) for w in caught]
        assert trainer.use_graph == (mode == "graph") and trainer.global_step == 5 and module.mixer.n == 5
        if mode == "graph":
            assert len(trainer._graphed) == 1 and all(isinstance(g, GraphedTrainStep) for g in trainer._graphed.values())
        finals[mode] = (losses, module.model.engine.flat.detach().clone(), module.mixer.last_rows)
    assert finals["eager"][0] == finals["graph"][0], (finals["eager"][0], finals["graph"][0])
    assert torch.equal(finals["eager"][1], finals["graph"][1])
    assert finals["eager"][2] == finals["graph"][2] and len(finals["graph"][2]) == 8
    for b, c in zip(batches, before):
        assert all(torch.equal(t, u) for t, u in zip(b, c)), "a training step wrote into the loader's tensors"


def test_mixing_changes_the_run_and_is_seeded(dev):
    """The mixed run differs from the plain one, and a second mixed run repeats the first."""
    from test_trainer_gpu import Batches, make

    batches = [tuple(t.cuda() for t in b) for b in Batches(16, 5, bs=8)]
    losses = []
    for augment in (None, dict(MIXING), dict(MIXING)):
        module, trainer = make(_cfg("32", augment))
        trainer._setup(module)
        module.train()
        losses.append([float(trainer.training_step(module, batches[i % 2], i).detach()) for i in range(3)])
    assert losses[1] == losses[2] and losses[0] != losses[1]


def test_resume_continues_the_draws(dev, tmp_path, monkeypatch):
    """(c) Checkpoint after epoch 1 and resume: epoch 2's losses are the uninterrupted run's; the checkpoint carries the mixer's
    counter, and one of a run without mixing has no `mix` entry."""
    from test_trainer_gpu import Batches, make
    from vit_amd.trainer import load_checkpoint_file

    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "ck"))
    train, val = Batches(24, 1, bs=8), Batches(8, 2, bs=8)
    m_full, t_full = make(_cfg("32", dict(MIXING), ep=2))
    t_full.fit(m_full, train, val)
    m_a, t_a = make(_cfg("32", dict(MIXING), ep=1, save=True))
    t_a.fit(m_a, train, val)
    raw = load_checkpoint_file(t_a.checkpointer.last_path)
    assert raw["vit_amd"]["mix"] == {"n": 3} and m_a.mixer.n == 3
    m_b, t_b = make(_cfg("32", dict(MIXING), ep=2))
    hist = t_b.fit(m_b, train, val, ckpt_path=t_a.checkpointer.last_path)
    assert len(hist) == 1 and m_b.mixer.n == m_full.mixer.n == 6
    assert (hist[0]["mae_loss"], hist[0]["val_mae"]) == (t_full.history[1]["mae_loss"], t_full.history[1]["val_mae"])
    assert torch.equal(m_b.model.engine.flat, m_full.model.engine.flat)
    # without mixing the file is laid out as it always was
    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "plain"))
    module, trainer = make(_cfg("32", None, ep=1, save=True))
    trainer.fit(module, train, val)
    own = load_checkpoint_file(trainer.checkpointer.last_path)["vit_amd"]
    assert set(own) == {"version", "dropout_base_seed", "dropout_step"}


def test_accumulation_draws_once_per_micro_batch(dev):
    """(d) accumulate_grad_batches = 2: every micro-batch is mixed by a draw of its own, inside the micro-batch."""
    from test_trainer_gpu import Batches, make

    batches = [tuple(t.cuda() for t in b) for b in Batches(32, 5, bs=8)]
    module, trainer = make(_cfg("32", dict(MIXING), accumulate_grad_batches=2))
    trainer._setup(module)
    module.train()
    plans = []
    for i, b in enumerate(batches):
        trainer.training_step(module, b, i, is_last=(i == len(batches) - 1))
        plans.append(module.mixer.last_rows)
    assert module.mixer.n == 4 and trainer.global_step == 2
    twin = type(module.mixer)(**{k: MIXING[k] for k in ("mixup_alpha", "cutmix_alpha", "mode", "seed")})
    assert plans == [twin.draw(8, 4096) for _ in range(4)]


def test_snapshot_and_restore_leave_the_counter_where_it_was(dev):
    """(e) What autotune_reserve_cus does around its probe steps, called directly: the probe's draws are given back."""
    from test_trainer_gpu import Batches, make

    batches = [tuple(t.cuda() for t in b) for b in Batches(16, 5, bs=8)]
    module, trainer = make(_cfg("32", dict(MIXING)))
    trainer._setup(module)
    module.train()
    trainer.training_step(module, batches[0], 0)
    snap = trainer._snapshot(module)
    assert snap["mix"] == {"n": 1}
    flat = module.model.engine.flat.detach().clone()
    for i in range(3):
        trainer.training_step(module, batches[1], i)
    assert module.mixer.n == 4
    trainer._restore(module, snap)
    assert module.mixer.n == 1 and torch.equal(module.model.engine.flat, flat)
    a = float(trainer.training_step(module, batches[1], 1).detach())
    # the same step from a run that never probed
    module2, trainer2 = make(_cfg("32", dict(MIXING)))
    trainer2._setup(module2)
    module2.train()
    trainer2.training_step(module2, batches[0], 0)
    assert float(trainer2.training_step(module2, batches[1], 1).detach()) == a
