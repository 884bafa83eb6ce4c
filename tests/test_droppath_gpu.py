"""Stochastic depth (`model.drop_path_rate`, include/vit_amd_droppath.h) on the GPU: the two path kernels against the host
restatement of the gate (tests/test_droppath_cpu.py: path_multiplier, three lines over oracle/dropmask.py), bit for bit; the
model against the CPU oracle run with the restated masks, at the project's existing train-mode gates
(tests/test_parity_gpu.py: check_train_parity); the CLS tail's bits; rate 0 and eval mode; the captured step; the trainer.

Kernel arithmetic the bitwise checks rest on:
  forward   xsum = x + scale * delta for a kept sample (at p = 0.5 the scale is exactly 2, so the fused and the unfused form
            round once to the same value; at p = 0.25 either form is accepted), xsum = x for a dropped one, whose delta is
            not read (its rows hold NaN here); mean / rstd / y are vit_layernorm_fwd's of that xsum.
  backward  dyn = bf16(dx * k), k = dropout multiplier x path multiplier, the product taken in float32; dx, dgamma, dbeta are
            vit_layernorm_bwd_rows' on the same inputs."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import dropmask as dm
from test_droppath_cpu import path_masks, path_multiplier, path_rates

pytestmark = pytest.mark.gpu

BASE_SEED = 0x5DEECE66D2468ACE
STEP = 3
SITE, DSITE = 4 + 4 * 5, 1 + 4 * 5 + 2  # a path site and a dropout site of one layer
EPS = 1e-12
SHAPES = [(6 * 129, 32, 129), (5 * 17, 64, 17), (4 * 197, 768, 197), (2 * 577, 1024, 577)]


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def equal_either(out, e_plain, e_fma):  # as in tests/test_dropout_gpu.py: the compiler may contract x + k * d
    return bool(((out == e_plain) | (out == e_fma)).all())


def seed_for(p, B, keys_xor=None):
    """The first seed from 1000 at which both branches have a kept and a dropped sample among B (found on the host)."""
    for seed in range(1000, 2000):
        m = path_multiplier(p, seed, SITE, B, keys_xor) != 0
        if all(0 < int(m[:, br].sum()) < B for br in (0, 1)):
            return seed
    raise AssertionError("no seed")


def row_mult(p, seed, B, T, br, dev, keys_xor=None):
    """float32 [B * T, 1]: the path multiplier of every token row."""
    m = path_multiplier(p, seed, SITE, B, keys_xor)[:, br]
    return torch.from_numpy(np.repeat(m, T)).to(dev).view(-1, 1)


def affine(D, dev):
    return randn((D,), dev, 252) * 0.1 + 1, randn((D,), dev, 253) * 0.1


def E(dev, *s, dt=torch.float32):
    return torch.empty(s, dtype=dt, device=dev)


# ------------------------------------------------------------------ 1. forward kernel
def check_fwd(vf, x, delta, mrow, p, seed, T, br, out_dtype, x_row_stride=1, handle=None):
    """One path forward over compact rows (x read with `x_row_stride`) against the host expression; returns xsum."""
    dev, (rows, D) = x.device, delta.shape
    g, b = affine(D, dev)
    xr = x.view(-1, D)[::x_row_stride][:rows]
    dropped = (mrow == 0).view(-1)
    assert 0 < int(dropped.sum()) < rows
    dl = delta.clone()
    dl[dropped] = float("nan")  # a dropped sample's delta is never read
    xsum = E(dev, rows, D)
    call = lambda: vf.layernorm_fwd_residual_path(x, dl, xsum, g, b, EPS, (p, SITE, T, br), seed, out_dtype=out_dtype,
                                                  x_row_stride=x_row_stride)
    if handle is not None:
        with vf.use_handle(handle):
            y, mean, rstd = call()
    else:
        y, mean, rstd = call()
    d32 = delta.float()
    e_plain = torch.where(dropped.view(-1, 1), xr, xr + d32 * mrow)
    e_fma = torch.where(dropped.view(-1, 1), xr, (xr.double() + d32.double() * mrow.double()).float())
    assert bool(torch.isfinite(xsum).all()) and bool(torch.isfinite(y.float()).all())
    assert torch.equal(xsum[dropped], xr[dropped])
    if p == 0.5:
        assert float(mrow.max()) == 2.0 and torch.equal(xsum, e_plain)
    else:
        assert equal_either(xsum, e_plain, e_fma)
    y2, mean2, rstd2 = vf.layernorm_fwd(xsum, g, b, EPS, out_dtype=out_dtype)
    assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2) and torch.equal(y, y2)
    return xsum


@pytest.mark.parametrize("ddt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,D,T", SHAPES)
def test_forward_kernel_bit_for_bit(dev, rows, D, T, ddt):
    import vit_amd.functional as vf

    B = rows // T
    x = randn((rows, D), dev, 11)
    delta = randn((rows, D), dev, 12).to(ddt)
    g, b = affine(D, dev)
    for p, br in ((0.5, 0), (0.5, 1), (0.25, 0), (0.25, 1)):
        seed = seed_for(p, B)
        check_fwd(vf, x, delta, row_mult(p, seed, B, T, br, dev), p, seed, T, br, ddt)
    # the strided form: B compact rows read from the rows b * T of x, compact row b draws sample b
    dc = delta[:B].contiguous()
    for p, br in ((0.5, 1), (0.25, 0)):
        seed = seed_for(p, B)
        check_fwd(vf, x, dc, row_mult(p, seed, B, 1, br, dev), p, seed, T, br, ddt, x_row_stride=T)
    # rate 0: the plain forms' bits, full and strided
    for stride, d_ in ((1, delta), (T, dc)):
        n = d_.shape[0]
        xs0, xs1 = E(dev, n, D), E(dev, n, D)
        a = vf.layernorm_fwd_residual(x, d_, xs0, g, b, EPS, out_dtype=ddt, x_row_stride=stride)
        c = vf.layernorm_fwd_residual_path(x, d_, xs1, g, b, EPS, (0.0, SITE, T, 1), 77, out_dtype=ddt, x_row_stride=stride)
        assert torch.equal(xs0, xs1) and all(torch.equal(u, v) for u, v in zip(a, c))


# ------------------------------------------------------------------ 2. backward kernel
def bwd_inputs(rows, D, dev):
    import vit_amd.functional as vf

    x = randn((rows, D), dev, 21)
    g, b = affine(D, dev)
    _, mean, rstd = vf.layernorm_fwd(x, g, b, EPS, out_dtype=torch.float32)
    dy = randn((rows, D), dev, 22).to(torch.bfloat16)
    dres = randn((rows, D), dev, 23)
    return x, g, mean, rstd, dy, dres


def run_bwd(vf, dev, t, path, dropout, old=None, **kw):
    """(dx, dgamma, dbeta, dyn, dbias) of the path form (path given) or of vit_layernorm_bwd_rows; `old`: what the parameter
    gradients hold before the call (grad_accumulate)."""
    x, g, mean, rstd, dy, dres = t
    n, D = x.shape
    dx, dyn = E(dev, n, D), E(dev, n, D, dt=torch.bfloat16)
    dg, db, dbias = (torch.zeros(D, device=dev) if old is None else old.clone() for _ in range(3))
    if path is None:
        vf.layernorm_bwd_rows(dy, x, g, mean, rstd, dres, dx, dg, db, dyn=dyn, dbias=dbias, dropout=dropout, **kw)
    else:
        vf.layernorm_bwd_path(dy, x, g, mean, rstd, dres, dx, dg, db, dyn, dbias, path, dropout=dropout, **kw)
    return dx, dg, db, dyn, dbias


def check_bwd(got, plain, k):
    dx, dg, db, dyn, dbias = got
    assert torch.equal(dx, plain[0]) and torch.equal(dg, plain[1]) and torch.equal(db, plain[2])
    assert torch.equal(dyn, (dx * k).to(torch.bfloat16))
    assert bool((dyn[(k == 0).all(dim=1)] == 0).all())
    return dbias


@pytest.mark.parametrize("ph", [0.1, 0.0])
@pytest.mark.parametrize("rows,D,T", SHAPES)
def test_backward_kernel(dev, rows, D, T, ph):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    B, p = rows // T, 0.25
    seed = seed_for(p, B)
    drop = (ph, seed, DSITE)
    t = bwd_inputs(rows, D, dev)
    x, g, mean, rstd, dy, dres = t
    dmult = torch.from_numpy(dm.multiplier(dm.drop_cfg(ph, seed, DSITE), rows, D)).to(dev)
    for br in (0, 1):
        mrow = row_mult(p, seed, B, T, br, dev)
        assert 0 < int((mrow == 0).sum()) < rows
        k = dmult * mrow  # float32: the row's single multiplier drop.scale * path.scale, or 0
        path = (p, SITE, T, br)
        plain = run_bwd(vf, dev, t, None, drop)
        got = run_bwd(vf, dev, t, path, drop)
        dbias = check_bwd(got, plain, k)
        assert rel(dbias, got[3].double().sum(0)) < 1e-5
        if br:
            continue
        # dres compact, one row per sample at the rows b * T (where the CLS rows' gradient rejoins the token stream)
        tc = (x, g, mean, rstd, dy, dres[:B].contiguous())
        got2 = run_bwd(vf, dev, tc, path, drop, dres_row_stride=T)
        check_bwd(got2, run_bwd(vf, dev, tc, None, drop, dres_row_stride=T), k)
        # the compact form: the tensors hold the rows b * T only; the masks and the sample are those of the original rows
        tt = (x[::T].contiguous(), g, mean[::T].contiguous(), rstd[::T].contiguous(), dy[::T].contiguous(), dres[::T].contiguous())
        got3 = run_bwd(vf, dev, tt, path, drop, row_stride=T, full_rows=rows)
        db3 = check_bwd(got3, run_bwd(vf, dev, tt, None, drop, row_stride=T, full_rows=rows), k[::T])
        assert rel(db3, got3[3].double().sum(0)) < 1e-5
        # grad_accumulate: the parameter gradients receive old + what overwrite mode stores
        h = _cabi.Handle(dev.index or 0)
        h.set_option("grad_accumulate", 1)
        old = randn((D,), dev, 24)
        with vf.use_handle(h):
            acc = run_bwd(vf, dev, t, path, drop, old=old)
            acc_plain = run_bwd(vf, dev, t, None, drop, old=old)
        check_bwd(acc, acc_plain, k)
        assert torch.equal(acc[1], old + got[1]) and torch.equal(acc[2], old + got[2]) and torch.equal(acc[4], old + got[4])
        assert rel(acc[4].double() - old.double(), acc[3].double().sum(0)) < 1e-5


# ------------------------------------------------------------------ 3. bound record
def test_bound_record_keys_reach_both_kernels(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    rows, D, T = SHAPES[0]
    B, p, br = rows // T, 0.25, 1
    h = _cabi.Handle(dev.index or 0)
    base, step = 0x1234567, 7
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    state[5] = step - 1
    kx = dm.step_keys(base, step)
    seed = seed_for(p, B, kx)
    bound, free = row_mult(p, seed, B, T, br, dev, kx), row_mult(p, seed, B, T, br, dev)
    assert not torch.equal(bound, free)
    x, delta = randn((rows, D), dev, 31), randn((rows, D), dev, 32).to(torch.bfloat16)
    g, b = affine(D, dev)
    t = bwd_inputs(rows, D, dev)
    drop = (0.1, seed, DSITE)
    plain_fwd = vf.layernorm_fwd_residual(x, delta, E(dev, rows, D), g, b, EPS)
    plain_bwd = run_bwd(vf, dev, t, None, drop)
    _cabi.check(h.lib.vit_step_state_bind(h.h, state.data_ptr()), "vit_step_state_bind")
    try:
        with vf.use_handle(h):
            _cabi.check(h.lib.vit_step_advance(h.h, base, 0.9, 0.999, vf._stream(state)), "vit_step_advance")
            check_fwd(vf, x, delta, bound, p, seed, T, br, torch.bfloat16, handle=h)
            k = torch.from_numpy(dm.multiplier(dm.drop_cfg(0.1, seed, DSITE), rows, D, keys_xor=kx)).to(dev) * bound
            check_bwd(run_bwd(vf, dev, t, (p, SITE, T, br), drop), run_bwd(vf, dev, t, None, drop), k)
            # rate 0 (and dropout 0): the record is not consulted
            xs = E(dev, rows, D)
            f0 = vf.layernorm_fwd_residual_path(x, delta, xs, g, b, EPS, (0.0, SITE, T, br), seed)
            b0 = run_bwd(vf, dev, t, (0.0, SITE, T, br), (0.0, seed, DSITE))
        torch.cuda.synchronize(dev)
    finally:
        _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
    assert all(torch.equal(u, v) for u, v in zip(f0, plain_fwd))
    free_b0 = run_bwd(vf, dev, t, None, (0.0, seed, DSITE))
    assert all(torch.equal(u, v) for u, v in zip(b0, free_b0))
    assert not torch.equal(plain_bwd[3], free_b0[3])  # the unbound dropout of `drop` is on: another dyn


# ------------------------------------------------------------------ 4. model parity against the oracle
RATE = 0.5
_oracle = {}


def oracle(tag, rc, sd, flux, labels):
    """One CPU oracle forward + backward with the right path masks, and one forward with the two branches' gates swapped."""
    from oracle import refvit

    if tag not in _oracle:
        _oracle.clear()
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        L, seed = rc.num_hidden_layers, dm.step_seed(BASE_SEED, STEP)
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        out = refvit.forward(rc, params, flux, labels, training=True, output_hidden_states=True,
                             masks=path_masks(RATE, L, rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, seed))
        out.loss.backward()
        with torch.no_grad():
            wrong = refvit.forward(rc, sd, flux, labels, training=True, output_hidden_states=True,
                                   masks=path_masks(RATE, L, rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, seed,
                                                    swap=True))
        _oracle[tag] = dict(loss=float(out.loss.detach()), logits=out.logits.detach(), hs=[h.detach() for h in out.hidden_states],
                            wrong_hs=[h.detach() for h in wrong.hidden_states],
                            grads={k: p.grad for k, p in params.items() if p.grad is not None})
    return _oracle[tag]


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
@pytest.mark.parametrize("tag", ["l3", "rope"])
def test_model_matches_oracle_with_restated_path_masks(dev, tag, precision):
    from test_cls_tail_gpu import build, case, errors, hip_pass

    rc, sd, flux, labels, _, gtol = case(tag)
    B, L = flux.shape[0], rc.num_hidden_layers
    # the restatement: every layer that can drop has a kept and a dropped sample in each branch at this seed
    rates = path_rates(RATE, L)
    for i in range(1, L):
        m = path_multiplier(rates[i], dm.step_seed(BASE_SEED, STEP), dm.site_of(i, 3), B) != 0
        assert rates[i] > 0 and all(0 < int(m[:, br].sum()) < B for br in (0, 1)), (i, m)
    o = oracle(tag, rc, sd, flux, labels)
    model = build(rc, sd, dev, precision)
    model.engine.cfg.drop_path_rate = RATE
    x, y = flux.to(dev), labels.to(dev)
    full = hip_pass(model, x, y, True, tail=False, output_hidden_states=True)
    tail = hip_pass(model, x, y, True, tail=True)
    assert full["tail"] is False and tail["tail"] is True
    assert model.engine._last["pd"] == rates
    hs = [h.detach().cpu() for h in full["out"].hidden_states]
    e_hs = max(rel(a, b) for a, b in zip(hs, o["hs"]))
    cat = lambda ts: torch.cat([t_.flatten() for t_ in ts])
    right, wrong = rel(cat(hs), cat(o["hs"])), rel(cat(hs), cat(o["wrong_hs"]))
    ef, et = errors(full, o), errors(tail, o)
    for name, e in (("full", ef), ("tail", et)):
        print(f"[drop path {tag} {precision} {name}] hidden states {e_hs:.2e}, logits {e['logits']:.2e}, loss {e['loss']:.2e}, "
              f"worst gradient {max(v[0] for v in e['grads'].values()):.2e}; hidden states against swapped branches {wrong:.2e} "
              f"(right masks {right:.2e})")
    assert wrong >= 10 * right, (right, wrong)
    if precision == "32":
        assert e_hs < 1e-4
        for name, e in (("full", ef), ("tail", et)):
            assert e["logits"] < 1e-4 and e["loss"] < 1e-4, (name, e["logits"], e["loss"])
            for pname, (r, _) in e["grads"].items():
                assert r < 2e-4, (name, pname, r)
        return
    loss_tol = 3e-2
    if tag == "rope":  # tests/test_parity_gpu.py: test_rope_train_mode_dropout_matches_oracle
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "rope.npz"))
        loss_tol = 2 * float(g["p1_loss"]) ** -0.5 * 1.5e-2
    assert e_hs < 1.5e-2
    for name, e in (("full", ef), ("tail", et)):
        assert e["loss"] <= loss_tol and e["logits"] <= 1.5e-2, (name, e["loss"], e["logits"])
        for pname, (r, c) in e["grads"].items():
            assert r < gtol and c > 0.999, (name, pname, r, c)


# ------------------------------------------------------------------ 5. the CLS tail keeps its bits
def test_cls_tail_same_bits_with_drop_path(dev):
    from test_cls_tail_gpu import build, case, hip_pass

    rc, sd, flux, labels, _, _ = case("ms")
    B, rate = flux.shape[0], 0.2
    m = path_multiplier(path_rates(rate, 2)[1], dm.step_seed(BASE_SEED, STEP), dm.site_of(1, 3), B) != 0
    assert (B, m[:, 0].sum(), m[:, 1].sum()) == (256, 208, 203)
    model = build(rc, sd, dev, "bf16-mixed")
    model.engine.cfg.drop_path_rate = rate
    x, y = flux.to(dev), labels.to(dev)
    full = hip_pass(model, x, y, True, tail=False)
    tail = hip_pass(model, x, y, True, tail=True)
    assert full["tail"] is False and tail["tail"] is True and model.engine._last["pd"][1] > 0
    assert tail["loss"] == full["loss"] and torch.equal(tail["logits"], full["logits"])
    for n in full["grads"]:
        assert torch.equal(tail["grads"][n], full["grads"][n]), n
    model.engine.cfg.drop_path_rate = 0.0  # and the gate is not a no-op at this geometry
    assert hip_pass(model, x, y, True, tail=True)["loss"] != tail["loss"]


# ------------------------------------------------------------------ 6. rate 0 is today
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_rate_zero_and_eval_mode_are_the_plain_model(dev, precision):
    from test_cls_tail_gpu import build, case, hip_pass
    from vit_amd.config import ViTConfig

    rc, sd, flux, labels, _, _ = case("l3")
    x, y = flux.to(dev), labels.to(dev)
    plain = build(rc, sd, dev, precision)  # built without the field
    assert plain.engine.cfg.drop_path_rate == 0.0 and "drop_path_rate" in ViTConfig.__dataclass_fields__
    ref = {train: hip_pass(plain, x, y, train, tail=True) for train in (True, False)}
    assert plain.engine._last["pd"] is None
    model = build(rc, sd, dev, precision)
    for rate, train in ((0.0, True), (0.5, False)):
        model.engine.cfg.drop_path_rate = rate
        got = hip_pass(model, x, y, train, tail=True)
        assert model.engine._last["pd"] is None
        assert got["loss"] == ref[train]["loss"] and torch.equal(got["logits"], ref[train]["logits"])
        for n in got["grads"]:
            assert torch.equal(got["grads"][n], ref[train]["grads"][n]), n
    model.engine.cfg.drop_path_rate = 0.5
    assert hip_pass(model, x, y, True, tail=True)["loss"] != ref[True]["loss"]


# ------------------------------------------------------------------ 7. captured step
def test_hip_graph_replays_draw_the_restated_path_masks(dev):
    """C1, bf16-mixed, rate 0.5, lr = 0, at the gates of tests/test_parity_gpu.py::test_hip_graph_replays_draw_the_restated_masks:
    the frozen launch carries p_i, the bound record's keys vary the draw."""
    from test_parity_gpu import oracle_pass, setup
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedAdamW

    rc, g, sd, model, x, labels = setup("c1", dev)
    eng = model.engine
    eng.cfg.drop_path_rate = RATE
    eng.base_seed, eng.step_counter = BASE_SEED, 0
    opt = FusedAdamW(model, lr=0.0)
    opt.set_grad_clip(0.5)
    module = types.SimpleNamespace(model=model, noise_level=0, train=model.train)
    warmup = 2
    gs = GraphedTrainStep(module, opt, (x, None, labels), warmup=warmup)
    seed_cap = dm.step_seed(BASE_SEED, warmup + 1)
    B, L = x.shape[0], rc.num_hidden_layers
    draws, losses = [], []
    for r in range(3):
        loss = float(gs.step((x, None, labels)))
        torch.cuda.synchronize(dev)
        kx = dm.step_keys(BASE_SEED, r + 1)
        draws.append(np.stack([path_multiplier(p, seed_cap, dm.site_of(i, 3), B, kx) for i, p in enumerate(path_rates(RATE, L))]))
        o = oracle_pass(rc, sd, x, labels, masks=path_masks(RATE, L, 0.1, 0.1, seed_cap, keys_xor=kx))
        no_xor = oracle_pass(rc, sd, x, labels, masks=path_masks(RATE, L, 0.1, 0.1, seed_cap), grads=False)
        errs = {}
        for name, ref in o["grads"].items():
            if float(ref.norm()) < 1e-6:
                continue
            mine = eng.layout.view(eng.grads, name).detach().cpu().double().flatten()
            r_ = ref.double().flatten()
            errs[name] = (rel(mine, r_), float(torch.dot(mine, r_) / (mine.norm() * r_.norm())))
        print(f"replay {r}: loss {loss:.6f}, oracle {o['loss']:.6f} (without the step keys {no_xor['loss']:.6f}); "
              f"worst gradient {max(v[0] for v in errs.values()):.2e}")
        assert abs(loss - o["loss"]) / o["loss"] <= 3e-2, (loss, o["loss"])
        assert abs(loss - no_xor["loss"]) >= 10 * abs(loss - o["loss"]), (loss, o["loss"], no_xor["loss"])
        for name, (e, c) in errs.items():
            assert e < 4e-2 and c > 0.999, (r, name, e, c)
        losses.append(loss)
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2]) and len(set(losses)) == 3


# ------------------------------------------------------------------ 8. trainer
def test_yaml_with_drop_path_rate_trains(dev, tmp_path):
    import yaml

    from scripts import run as run_script
    from test_trainer_gpu import c1_config
    from vit_amd.trainer import Trainer

    cfg = c1_config(ep=1, precision="bf16-mixed")
    cfg["project"] = "t"
    cfg["model"]["drop_path_rate"] = 0.3
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump(cfg))
    args = types.SimpleNamespace(config=str(path), gpu=1, debug=0, seed=42, synthetic=48, save=False, ckpt=None)
    config, module, data = run_script.build(args)
    eng = module.model.engine
    assert eng.cfg.drop_path_rate == 0.3
    trainer = Trainer(config["train"], device=dev, verbose=False)
    train_loader, val_loader = data.fit_loaders(args.debug)
    before = None
    seen = []
    fwd = eng.forward

    def spy(*a, **kw):  # the path rates of every training forward, and the parameters ahead of the first one
        nonlocal before
        if before is None:
            before = eng.flat.detach().clone()
        out = fwd(*a, **kw)
        if eng._last["pd"] is not None:
            seen.append(eng._last["pd"])
        return out

    eng.forward = spy
    hist = trainer.fit(module, train_loader, val_loader)
    assert trainer.global_step == 3 and len(seen) == 3 and seen[0] == path_rates(0.3, 3)
    logged = {k: float(v) for k, v in hist[-1].items() if "loss" in k}
    assert logged and all(np.isfinite(v) for v in logged.values()), logged
    n = eng.layout.n_trainable
    assert bool(torch.isfinite(eng.flat).all()) and float((eng.flat[:n] - before[:n]).abs().max()) > 0
