"""Sharpness-aware minimisation (`train.sam_rho`, include/vit_amd_sam.h, vit_amd/sam.py) on the GPU: the three kernels against
their host restatement (tests/_sam_ref.py); the model's two-pass backward against the UNCHANGED CPU oracle run twice with the same
restated masks (`_sam_ref.oracle_sam`), through the chain construction -- the oracle evaluated at w + e(g_hip), a plain parity at
other weights, held to the project's own gates -- and end to end; that nothing is left behind; the compositions (LayerScale, patch
dropout, average pooling, masked spectrum modelling, soft targets); the captured step; the Trainer; two gloo ranks on one GPU.
Outputs and the workspace are poisoned before the kernel calls (tests/_poison.py)."""
import dataclasses
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _sam_ref as sr
from _poison import poisoned
from oracle import dropmask as dm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_SEED = 0x5DEECE66D2468ACE  # tests/test_cls_tail_gpu.py: hip_pass runs step STEP of this seed
STEP = 3
GUARD = 64  # elements behind every kernel buffer that must keep their fill
SIZES = [1, 3, 4, 5, 1023, 4096 + 7, 1 << 20]
# (case, adaptive) -> rho: where the oracle's second gradient is 0.17 ... 0.47 away from its first (the models are stiff)
RHO = {("l3", False): 0.005, ("l3", True): 0.05, ("rope", False): 0.02, ("rope", True): 0.2}


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def guarded(dev, n, dtype=torch.float32):
    """(a tensor of n elements, the GUARD elements behind it): one allocation, so the band is what an overrun would hit."""
    buf = torch.zeros(n + GUARD, dtype=dtype, device=dev)
    return buf[:n], buf[n:]


def kernel_case(dev, n, seed):
    g = torch.Generator().manual_seed(seed)
    p = (0.5 * torch.randn(n, generator=g)).to(dev)
    gr = (2.0 * torch.randn(n, generator=g)).to(dev)
    return p, gr


# ------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sqnorm_kernel(dev, n, adaptive):
    import vit_amd.functional as vf

    p, g = kernel_case(dev, n, 100 + n % 97)
    out = torch.zeros(1, device=dev)
    got = poisoned(dev, lambda: vf.sam_sqnorm(g, p, adaptive=adaptive, out=out), [out])[0]
    want = sr.sqnorm(p.cpu().numpy(), g.cpu().numpy(), adaptive)
    err = abs(float(got) - want) / want
    print(f"[sam sqnorm n={n} adaptive={adaptive}] rel {err:.2e}")
    assert err < 1e-6
    plain = vf.grad_sqnorm(g)
    if not adaptive:  # the same two launches: the same bits, and p is not needed
        assert torch.equal(bits(got), bits(plain))
        assert torch.equal(bits(vf.sam_sqnorm(g, None)), bits(plain))
    else:
        assert n < 4 or not torch.equal(bits(got), bits(plain))
    # accumulate: out[0] += the sum, one f32 add
    acc = torch.full((1,), 3.5, device=dev)
    vf.sam_sqnorm(g, p, adaptive=adaptive, accumulate=True, out=acc)
    assert torch.equal(bits(acc), bits(got + 3.5))
    if n >= 8:  # two runs in ascending order: vit_grad_sqnorm_acc's bits in the plain form, the float64 sum in both
        a = 4 * (n // 8)
        two = vf.sam_sqnorm(g[:a], p[:a], adaptive=adaptive)
        vf.sam_sqnorm(g[a:], p[a:], adaptive=adaptive, accumulate=True, out=two)
        assert abs(float(two) - want) / want < 1e-6
        if not adaptive:
            ref = vf.grad_sqnorm(g[:a])
            vf.grad_sqnorm(g[a:], out=ref, accumulate=True)
            assert torch.equal(bits(two), bits(ref))


@pytest.mark.parametrize("shadowed", [False, True])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_ascend_kernel(dev, n, adaptive, shadowed):
    import vit_amd.functional as vf

    rho = 0.5 if adaptive else 0.05
    p0, g = kernel_case(dev, n, 200 + n % 97)
    sq = vf.sam_sqnorm(g, p0, adaptive=adaptive)
    p, p_pad = guarded(dev, n)
    backup, b_pad = guarded(dev, n)
    shadow, s_pad = guarded(dev, n, torch.bfloat16) if shadowed else (None, None)

    def run():
        p.copy_(p0)
        vf.sam_ascend(p, g, backup, shadow, rho, sq, adaptive=adaptive)

    outs = [p, backup] + ([shadow] if shadowed else [])
    pads = [p_pad, b_pad] + ([s_pad] if shadowed else [])
    got = poisoned(dev, run, outs, pads=pads)  # pad elements behind n are untouched
    s = rho / (sq.sqrt() + 1e-12)
    want = p0 + ((p0 * p0) * g if adaptive else g) * s  # the torch twin, f32 on the device
    host = sr.ascend(p0.cpu().numpy(), g.cpu().numpy(), rho, adaptive, float(sq))
    e_twin, e_host = rel(got[0], want), rel(got[0], host)
    moved = rel(got[0], p0)
    print(f"[sam ascend n={n} adaptive={adaptive}] against the torch twin {e_twin:.2e}, the host restatement {e_host:.2e}; moved {moved:.2e}")
    assert e_twin < 1e-6 and e_host < 1e-6 and moved > 0
    # per element: the twin rounds the step e (half an ulp of e) and then the sum (half an ulp of it), the kernel fuses the step's
    # last multiply into the add and rounds once, so the two are at most 2^-23 (|e| + |p + e|) <= 2^-22 (|p| + |e|) apart.  At
    # n = 2^20 the whole step is 1e-4 of ||p||, which the norm-wise gate above alone would not see.
    assert bool(((got[0] - want).abs() <= 2.0 ** -22 * (p0.abs() + (want - p0).abs())).all())
    assert torch.equal(bits(got[1]), bits(p0))  # backup is the old p bit for bit
    if shadowed:
        assert torch.equal(bits(got[2]), bits(got[0].to(torch.bfloat16)))  # the shadow is bf16(p) exactly
    if n >= 8:  # a call on a 16-byte-aligned slice gives there the bits of the whole-buffer call, and touches nothing else
        a = 4 * (n // 8)
        q, bq = p0.clone(), torch.full_like(p0, -7.0)
        sh = torch.full((n,), -7.0, dtype=torch.bfloat16, device=dev) if shadowed else None
        vf.sam_ascend(q[a:], g[a:], bq[a:], None if sh is None else sh[a:], rho, sq, adaptive=adaptive)
        assert torch.equal(bits(q[a:]), bits(got[0][a:])) and torch.equal(bits(q[:a]), bits(p0[:a]))
        assert torch.equal(bits(bq[a:]), bits(p0[a:])) and bool((bq[:a] == -7.0).all())
        if shadowed:
            assert torch.equal(bits(sh[a:]), bits(got[2][a:])) and bool((sh[:a] == -7.0).all())


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("n", [1, 5, 4096 + 7])
def test_zero_gradient_leaves_p_bit_identical(dev, n, adaptive):
    import vit_amd.functional as vf

    p0, _ = kernel_case(dev, n, 300 + n)
    p0[0] = -0.0
    g = torch.zeros(n, device=dev)
    sq = vf.sam_sqnorm(g, p0, adaptive=adaptive)
    assert float(sq) == 0.0  # s = rho / 1e-12: huge and finite
    p, backup, shadow = p0.clone(), torch.empty_like(p0), torch.empty(n, dtype=torch.bfloat16, device=dev)
    vf.sam_ascend(p, g, backup, shadow, 0.05, sq, adaptive=adaptive)
    assert torch.equal(bits(p), bits(p0)) and torch.equal(bits(backup), bits(p0))
    assert torch.equal(bits(shadow), bits(vf.cast_f32_bf16(p0)))
    if adaptive and n > 4:  # likewise where only p is zero: c = p^2 = 0
        g = torch.ones(n, device=dev)
        q = p0.clone()
        q[1], q[n - 1] = 0.0, -0.0
        sq = vf.sam_sqnorm(g, q, adaptive=True)
        r = q.clone()
        vf.sam_ascend(r, g, backup, None, 0.05, sq, adaptive=True)
        assert bits(r)[1] == bits(q)[1] and bits(r)[n - 1] == bits(q)[n - 1] and bits(r)[0] == bits(q)[0]
        assert not torch.equal(r, q)


@pytest.mark.parametrize("n", SIZES)
def test_descend_restores_every_bit(dev, n):
    import vit_amd.functional as vf

    p0, g = kernel_case(dev, n, 400 + n % 97)
    sq = vf.sam_sqnorm(g)
    p, p_pad = guarded(dev, n)
    shadow, s_pad = guarded(dev, n, torch.bfloat16)
    backup = torch.empty(n, device=dev)
    p.copy_(p0)
    shadow0 = vf.cast_f32_bf16(p0)
    vf.sam_ascend(p, g, backup, shadow, 0.05, sq)
    assert not torch.equal(p, p0)
    got = poisoned(dev, lambda: vf.sam_descend(p, backup, shadow), [p, shadow], pads=[p_pad, s_pad])
    assert torch.equal(bits(got[0]), bits(p0)) and torch.equal(bits(got[1]), bits(shadow0))
    # f32 mode: no shadow
    q, bq = p0.clone(), torch.empty_like(p0)
    vf.sam_ascend(q, g, bq, None, 0.05, sq)
    vf.sam_descend(q, bq)
    assert torch.equal(bits(q), bits(p0))
    # NaN / Inf / -0.0 planted in p: the copy is bitwise (a NaN keeps its payload)
    w = p0.clone()
    plant = [float("nan"), float("inf"), -float("inf"), -0.0]
    for i in range(min(n, len(plant))):
        w[(i * 7919) % n] = plant[i]
    if n >= 4:
        bits(w)[n - 1] = 0x7FC12345  # a NaN with a payload
    w0 = w.clone()
    sh = vf.cast_f32_bf16(w0)
    sh0 = sh.clone()
    bw = torch.empty_like(w)
    vf.sam_ascend(w, g, bw, sh, 0.05, sq)
    vf.sam_descend(w, bw, sh)
    assert torch.equal(bits(w), bits(w0)) and torch.equal(bits(sh), bits(sh0))


def test_argument_errors_launch_nothing(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    n = 64
    h = vf._h(torch.empty(1, device=dev))
    st = torch.cuda.current_stream(dev).cuda_stream
    SENT = -12345.0
    g = torch.randn(n, device=dev)
    sq = torch.ones(4, device=dev)
    outs = dict(p=torch.full((n,), SENT, device=dev), backup=torch.full((n,), SENT, device=dev),
                shadow=torch.full((n,), SENT, dtype=torch.bfloat16, device=dev), out=torch.full((4,), SENT, device=dev))
    lib, hh = h.lib, h.h
    P, G, Bk, Sh, O, Sq = (outs["p"].data_ptr(), g.data_ptr(), outs["backup"].data_ptr(), outs["shadow"].data_ptr(),
                           outs["out"].data_ptr(), sq.data_ptr())
    nan = float("nan")
    calls = [
        (lambda: lib.vit_sam_sqnorm(hh, P, None, n, 0, 0, O, st), b"null pointer"),
        (lambda: lib.vit_sam_sqnorm(hh, P, G, n, 0, 0, None, st), b"null pointer"),
        (lambda: lib.vit_sam_sqnorm(hh, None, G, n, 1, 0, O, st), b"needs p"),
        (lambda: lib.vit_sam_sqnorm(hh, P, G, 0, 0, 0, O, st), b"n = 0"),
        (lambda: lib.vit_sam_sqnorm(hh, P, G + 4, n - 1, 0, 0, O, st), b"16-byte aligned"),
        (lambda: lib.vit_sam_sqnorm(hh, P + 8, G, n - 2, 1, 0, O, st), b"16-byte aligned"),
        (lambda: lib.vit_sam_sqnorm(hh, P, G, n, 0, 0, O + 2, st), b"4-byte aligned"),
        (lambda: lib.vit_sam_ascend(hh, None, G, Bk, Sh, n, 0.05, 0, Sq, st), b"null pointer"),
        (lambda: lib.vit_sam_ascend(hh, P, None, Bk, Sh, n, 0.05, 0, Sq, st), b"null pointer"),
        (lambda: lib.vit_sam_ascend(hh, P, G, None, Sh, n, 0.05, 0, Sq, st), b"null pointer"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk, Sh, n, 0.05, 0, None, st), b"null pointer"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk, Sh, -3, 0.05, 0, Sq, st), b"n = -3"),
        (lambda: lib.vit_sam_ascend(hh, P + 4, G, Bk, Sh, n - 1, 0.05, 0, Sq, st), b"16-byte aligned"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk + 8, Sh, n - 2, 0.05, 0, Sq, st), b"16-byte aligned"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk, Sh + 2, n - 1, 0.05, 0, Sq, st), b"8-byte aligned"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk, Sh, n, 0.05, 0, Sq + 1, st), b"4-byte aligned"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk, Sh, n, 0.0, 0, Sq, st), b"rho"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk, Sh, n, -1.0, 1, Sq, st), b"rho"),
        (lambda: lib.vit_sam_ascend(hh, P, G, Bk, Sh, n, nan, 0, Sq, st), b"rho"),
        (lambda: lib.vit_sam_descend(hh, None, Bk, Sh, n, st), b"null pointer"),
        (lambda: lib.vit_sam_descend(hh, P, None, Sh, n, st), b"null pointer"),
        (lambda: lib.vit_sam_descend(hh, P, Bk, Sh, 0, st), b"n = 0"),
        (lambda: lib.vit_sam_descend(hh, P + 4, Bk, Sh, n - 1, st), b"16-byte aligned"),
        (lambda: lib.vit_sam_descend(hh, P, Bk, Sh + 2, n - 1, st), b"8-byte aligned"),
    ]
    for i, (call, text) in enumerate(calls):
        assert call() == -1, i  # VIT_ERR_ARG
        assert text in lib.vit_last_error(), (i, text, lib.vit_last_error())
    with pytest.raises(_cabi.VitError, match="needs p"):
        vf.sam_sqnorm(g, None, adaptive=True, out=outs["out"])
    with pytest.raises(_cabi.VitError, match="exceeds a buffer"):
        vf.sam_ascend(outs["p"], g, outs["backup"], outs["shadow"], 0.05, sq, n=n + 1)
    with pytest.raises(_cabi.VitError, match="exceeds a buffer"):
        vf.sam_descend(outs["p"], outs["backup"][:-4], outs["shadow"])
    with pytest.raises(_cabi.VitError, match="expected torch.bfloat16"):
        vf.sam_descend(outs["p"], outs["backup"], outs["backup"])
    torch.cuda.synchronize(dev)
    for k, v in outs.items():  # nothing was launched: every output still holds its sentinel
        assert bool((v == SENT).all()), k


# ------------------------------------------------------------------ 2. the model is the oracle
_first = {}


def step_masks(rc):
    return dm.engine_masks(rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, dm.step_seed(BASE_SEED, STEP), None)


def cat(grads, names=None):
    return torch.cat([grads[k].double().flatten() for k in (sorted(grads) if names is None else names)])


def oracle_first(key, rc, sd, flux, labels, masks, step=None):
    """The oracle's first pass (loss, logits, g), computed once per case and left unchanged."""
    if key not in _first:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        _first[key] = sr._grad_pass(rc, sd, flux, labels, masks, sr._default_step if step is None else step)
    return _first[key]


def check_fp32(name, h, o):
    """The project's bounds for these cases at precision '32' (check_fp32 of tests/test_pool_gpu.py): logits and loss < 1e-4,
    every gradient tensor < 2e-4."""
    from test_cls_tail_gpu import errors

    e = errors(h, o)
    worst = max(e["grads"].items(), key=lambda kv: kv[1][0])
    print(f"[sam {name} 32] logits {e['logits']:.2e}, loss {e['loss']:.2e}, worst gradient {worst[1][0]:.2e} ({worst[0]})")
    assert e["logits"] < 1e-4 and e["loss"] < 1e-4, (name, e["logits"], e["loss"])
    for pname, (r, _) in e["grads"].items():
        assert r < 2e-4, (name, pname, r)
    return e


def chain(name, model, run_pass, rc, sd, flux, labels, masks, rho, adaptive, step=None, first_key=None):
    """The chain construction.  `run_pass(model)` -> dict(loss, logits, grads) of one training pass at step STEP.
    Returns (h0: the plain pass, h1: the pass with SAM attached, o: the oracle's L(w), logits(w) and its gradient at
    w + e(g_hip), first: the oracle's own first pass)."""
    model.set_sam(None)
    h0 = run_pass(model)
    eps = sr.named_epsilon(sd, h0["grads"], rho, adaptive)
    sam = model.set_sam(rho, adaptive)
    before = model.engine.flat.detach().clone()
    h1 = run_pass(model)
    assert sam.perturbed is False and torch.equal(bits(model.engine.flat), bits(before))
    first = oracle_first(first_key or name, rc, sd, flux, labels, masks, step)
    ref = sr.oracle_sam(rc, sd, flux, labels, masks, rho, adaptive, eps=eps, step=step)
    o = dict(loss=first[0], logits=first[1], grads=ref["g_sam"], loss_sam=ref["loss_sam"])
    return h0, h1, o, first


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
@pytest.mark.parametrize("tag", ["l3", "rope"])
def test_model_is_the_oracle(dev, tag, adaptive, precision):
    """The chain test -- hip gradient with SAM attached against the oracle at w + e(g_hip): precision '32' loss < 1e-4 and every
    gradient tensor < 2e-4; bf16-mixed on l3 every tensor < the case's gtol with cosine > 0.999 -- and the end-to-end test
    against the oracle's own two passes: rel(g_sam_hip, g_sam_oracle) < 0.25 * rel(g_oracle, g_sam_oracle) on the concatenated
    gradient, the measured value printed per precision."""
    from test_cls_tail_gpu import build, case, errors, hip_pass

    rc, sd, flux, labels, _, gtol = case(tag)
    rho = RHO[(tag, adaptive)]
    masks = step_masks(rc)
    model = build(rc, sd, dev, precision)
    x, y = flux.to(dev), labels.to(dev)
    h0, h1, o, first = chain(f"{tag} {'adaptive' if adaptive else 'plain'}", model, lambda m: hip_pass(m, x, y, True, tail=True),
                             rc, sd, flux, labels, masks, rho, adaptive, first_key=tag)
    assert h1["tail"] is True and model.engine.step_counter == STEP
    # the returned loss and logits are the first pass's: L(w), not L(w')
    assert abs(o["loss_sam"] - o["loss"]) / abs(o["loss"]) > 1e-3
    assert h1["loss"] == h0["loss"] and torch.equal(h1["logits"], h0["logits"])
    names = sorted(o["grads"])
    if precision == "32":
        check_fp32(f"{tag} rho={rho} adaptive={adaptive} chain", h1, o)
    else:
        e = errors(h1, o)
        worst = max(e["grads"].items(), key=lambda kv: kv[1][0])
        print(f"[sam {tag} rho={rho} adaptive={adaptive} bf16-mixed chain] loss {e['loss']:.2e}, worst gradient {worst[1][0]:.2e} "
              f"({worst[0]}, gtol {gtol}), lowest cosine {min(c for _, c in e['grads'].values()):.5f}")
        if tag == "l3":
            for name, (r, c) in e["grads"].items():
                assert r < gtol and c > 0.999, (name, r, c)
    # end to end: the oracle's own e, from its own first gradient
    full = sr.oracle_sam(rc, sd, flux, labels, masks, rho, adaptive, eps=sr.named_epsilon(sd, first[2], rho, adaptive))
    moved = rel(cat(first[2], names), cat(full["g_sam"], names))
    got = rel(cat(h1["grads"], names), cat(full["g_sam"], names))
    plain = rel(cat(h0["grads"], names), cat(full["g_sam"], names))
    worst_sep = min(rel(first[2][k], full["g_sam"][k]) for k in names if float(first[2][k].norm()) > 1e-6 * float(cat(first[2]).norm()))
    print(f"[sam {tag} rho={rho} adaptive={adaptive} {precision} end to end] rel(g_sam_hip, g_sam_oracle) {got:.3e}; the oracle's own "
          f"rel(g, g_sam) {moved:.3f} (worst-separated tensor {worst_sep:.3f}); the plain hip gradient is {plain:.3f} away")
    assert moved > 0.1 and plain > 0.5 * moved  # the second pass is in the path: without it the check below fails
    assert got < 0.25 * moved, (got, moved)


def test_fresh_masks_in_the_second_pass_would_fail(dev):
    """The negative control of the chain test: the oracle at w + e(g_hip) under the masks of step STEP + 1 is far outside the
    gates, so a second pass that redrew its masks could not pass."""
    from test_cls_tail_gpu import build, case, errors, hip_pass

    rc, sd, flux, labels, _, _ = case("rope")
    rho = RHO[("rope", False)]
    model = build(rc, sd, dev, "32")
    model.set_sam(rho)
    h1 = hip_pass(model, flux.to(dev), labels.to(dev), True, tail=True)
    model.set_sam(None)
    h0 = hip_pass(model, flux.to(dev), labels.to(dev), True, tail=True)
    eps = sr.named_epsilon(sd, h0["grads"], rho, False)
    other = dm.engine_masks(rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, dm.step_seed(BASE_SEED, STEP + 1), None)
    wrong = sr.oracle_sam(rc, sd, flux, labels, other, rho, False, eps=eps)
    e = errors(dict(h1, loss=1.0, logits=torch.ones(1)), dict(loss=1.0, logits=torch.ones(1), grads=wrong["g_sam"]))
    least = min(r for r, _ in e["grads"].values())
    print(f"[sam rope fresh masks] the nearest gradient tensor is {least:.3f} away")
    assert least > 0.05


# ------------------------------------------------------------------ 3. nothing is left behind
def sam_model(dev, precision, tag="l3", adaptive=False):
    from test_cls_tail_gpu import build, case

    rc, sd, flux, labels, _, _ = case(tag)
    model = build(rc, sd, dev, precision)
    model.set_sam(RHO[(tag, adaptive)], adaptive)
    return rc, model, flux.to(dev), labels.to(dev)


def tensors(eng, buf=None):
    """Every trainable tensor of a flat buffer (default: the gradients), concatenated: what the kernels write -- the alignment
    pads between the entries belong to nobody."""
    lay = eng.layout
    buf = eng.grads if buf is None else buf
    return torch.cat([lay.view(buf, k).flatten() for k, (off, _) in lay.entries.items() if off < lay.n_trainable]).clone()


def nan_fill(eng):
    """NaN into every trainable gradient tensor.  Not into the alignment pads between them: those are zero in every flat buffer
    and belong to the runs the norms sum over (the optimizer's clip norm included)."""
    lay = eng.layout
    for k, (off, _) in lay.entries.items():
        if off < lay.n_trainable:
            lay.view(eng.grads, k).fill_(float("nan"))


def one_step(model, x, y, step=STEP):
    eng = model.engine
    model.train()
    eng.base_seed, eng.step_counter = BASE_SEED, step - 1
    for p in model.parameters():
        p.grad = None
    out = model(x, labels=y)
    out.loss.backward()
    return out


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_nothing_is_left_behind(dev, precision):
    rc, model, x, y = sam_model(dev, precision)
    eng, sam, lay = model.engine, model.sam, model.engine.layout
    eng._ensure_device_state()
    flat0 = eng.flat.detach().clone()
    shadow0 = eng.shadow.clone() if precision != "32" else None
    out = one_step(model, x, y)
    torch.cuda.synchronize(dev)
    assert sam.perturbed is False and eng.step_counter == STEP  # advanced by one, not two
    assert torch.equal(bits(eng.flat), bits(flat0))
    if shadow0 is not None:
        assert torch.equal(bits(eng.shadow), bits(shadow0))
    assert float(sam.last_grad_norm) > 0 and torch.equal(sam.backup[:lay.n_trainable], flat0[:lay.n_trainable])
    loss1, g1 = float(out.loss.detach()), tensors(eng)
    for name, p in zip(model._param_names, model._param_list):  # autograd got the flat buffer's views
        if not name.startswith("vit.pooler."):
            assert p.grad is not None and p.grad.data_ptr() == eng.g(name).data_ptr(), name
    # a second identical step reproduces loss and gradient bit for bit
    nan_fill(eng)
    out2 = one_step(model, x, y)
    assert float(out2.loss.detach()) == loss1 and torch.equal(bits(tensors(eng)), bits(g1))
    # the next step draws other masks, and the same ones in both of its passes (not the previous step's)
    one_step(model, x, y, step=STEP + 1)
    assert eng.step_counter == STEP + 1 and not torch.equal(tensors(eng), g1)
    # detached: the plain gradient
    model.set_sam(None)
    one_step(model, x, y)
    assert rel(tensors(eng), g1) > 0.05


def test_refusals(dev):
    from vit_amd._cabi import VitError

    rc, model, x, y = sam_model(dev, "32")
    eng = model.engine
    one_step(model, x, y)
    flat0 = eng.flat.detach().clone()
    # a second backward without zero_grad would accumulate
    model.train()
    out = model(x, labels=y)
    with pytest.raises(VitError, match="accumulat"):
        out.loss.backward()
    assert model.sam.perturbed is False and torch.equal(bits(eng.flat), bits(flat0))
    # an input that requires grad
    with pytest.raises(ValueError, match="requires grad"):
        model(x.clone().requires_grad_(True), labels=y)


def test_frozen_slices_keep_every_bit(dev):
    """Query and key weights frozen (requires_grad False): their slices are outside the perturbed runs, bit-identical between
    ascend() and descend(), and their .grad stays None."""
    rc, model, x, y = sam_model(dev, "bf16-mixed")
    eng, sam, lay = model.engine, model.sam, model.engine.layout
    frozen = [n for n in model._param_names if ".attention.attention.query." in n or ".attention.attention.key." in n]
    assert len(frozen) == 4 * rc.num_hidden_layers
    for name, p in zip(model._param_names, model._param_list):
        if name in frozen:
            p.requires_grad_(False)
    runs = sam.runs()
    assert len(runs) == 2 * rc.num_hidden_layers + 1  # per layer: the value weight, and from the value bias to the next query
    eng._ensure_device_state()
    flat0, shadow0 = eng.flat.detach().clone(), eng.shadow.clone()
    seen = {}
    real = sam.descend

    def spy():
        seen["flat"], seen["shadow"], seen["perturbed"] = eng.flat.detach().clone(), eng.shadow.clone(), sam.perturbed
        real()

    sam.descend = spy
    one_step(model, x, y)
    assert seen["perturbed"] is True and sam.perturbed is False
    moved = 0
    for name, p in zip(model._param_names, model._param_list):
        was, now = lay.view(flat0, name), lay.view(seen["flat"], name)
        if name in frozen or name.startswith("vit.pooler."):
            assert torch.equal(bits(now), bits(was)), name
            assert torch.equal(bits(lay.view(seen["shadow"], name)), bits(lay.view(shadow0, name))), name
            assert p.grad is None, name
        else:
            moved += int(not torch.equal(now, was))
    assert moved > 10
    assert torch.equal(bits(eng.flat), bits(flat0)) and torch.equal(bits(eng.shadow), bits(shadow0))


def test_exception_in_the_second_forward_restores_the_weights(dev, monkeypatch):
    rc, model, x, y = sam_model(dev, "bf16-mixed")
    eng = model.engine
    eng._ensure_device_state()
    flat0, shadow0 = eng.flat.detach().clone(), eng.shadow.clone()
    real = eng.forward

    def failing(*a, reuse_step=False, **kw):
        if reuse_step:
            assert model.sam.perturbed and not torch.equal(eng.flat, flat0)
            raise RuntimeError("injected into the second forward")
        return real(*a, **kw)

    monkeypatch.setattr(eng, "forward", failing)
    model.train()
    out = model(x, labels=y)
    with pytest.raises(RuntimeError, match="injected"):
        out.loss.backward()
    torch.cuda.synchronize(dev)
    assert model.sam.perturbed is False
    assert torch.equal(bits(eng.flat), bits(flat0)) and torch.equal(bits(eng.shadow), bits(shadow0))


# ------------------------------------------------------------------ 4. compositions (precision '32', dropout off)
def no_dropout(model):
    model.engine.cfg.hidden_dropout_prob = model.engine.cfg.attention_probs_dropout_prob = 0.0
    return model


def test_composition_layer_scale(dev):
    """The folded operands follow the perturbed weights: with the refold suppressed the same step misses the gates."""
    from oracle import refvit
    from test_cls_tail_gpu import errors, hip_pass
    from test_layerscale_gpu import build as ls_build
    from test_layerscale_gpu import fixture

    rc, kw, sd, x, labels = fixture("c1")

    def step(rc, leaves, flux, labels, masks):
        params = {k: v for k, v in leaves.items() if not k.endswith(".lambda1")}
        for k, lam in leaves.items():
            if k.endswith(".lambda1"):
                stem = k.replace("layer_scale1.lambda1", "attention.output.dense").replace("layer_scale2.lambda1", "output.dense")
                params[stem + ".weight"] = lam[:, None] * leaves[stem + ".weight"]
                params[stem + ".bias"] = lam * leaves[stem + ".bias"]
        out = refvit.forward(rc, params, flux, labels, training=False)
        return out.loss, out.logits

    model = no_dropout(ls_build(kw, sd, dev, "32"))
    xd, yd = x.to(dev), labels.to(dev)
    run = lambda m: hip_pass(m, xd, yd, True, tail=True)  # noqa: E731
    h0, h1, o, _ = chain("layer scale", model, run, rc, sd, x, labels, None, 0.005, False, step=step)
    e = check_fp32("layer scale", h1, o)
    assert sum(n.endswith(".lambda1") for n in e["grads"]) == 2 * rc.num_hidden_layers
    # the same step with the refold suppressed: the second pass multiplies by operands folded from the unperturbed weights
    eng = model.engine
    eng.fold_layer_scale()
    eng.fold_layer_scale = lambda: None
    try:
        stale = errors(run(model), o)
    finally:
        del eng.fold_layer_scale
    worst = max(r for r, _ in stale["grads"].values())
    print(f"[sam layer scale] refold suppressed: worst gradient {worst:.2e}")
    assert worst > 10 * 2e-4


def test_composition_patch_dropout(dev):
    from _patchdrop_ref import kept, shortened_signal
    from test_cls_tail_gpu import case, hip_pass
    from test_pool_gpu import avg_model

    rc, sd, flux, labels, _, _ = case("l3")
    rc = dataclasses.replace(rc, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    B, N, P = flux.shape[0], rc.num_patches, rc.patch_size
    K = kept(N, 0.5)
    rng = np.random.default_rng(91)
    idx = np.stack([np.sort(rng.choice(N, K, replace=False)) for _ in range(B)]).astype(np.int32)
    rc2 = dataclasses.replace(rc, image_size=K * P)
    model = no_dropout(avg_model(rc, sd, dev, "32", global_pool="token", patch_drop_rate=0.5))
    eng = model.engine
    eng.patch_keep = torch.from_numpy(idx).to(dev)
    x, y = flux.to(dev), labels.to(dev)
    h0, h1, o, _ = chain("patch dropout", model, lambda m: hip_pass(m, x, y, True, tail=True), rc2, sd,
                         shortened_signal(flux, idx, P), labels, None, 0.005, False)
    assert eng._last["T"] == 1 + K and np.array_equal(eng._last["keep"].cpu().numpy(), idx)
    check_fp32("patch dropout", h1, o)
    assert rel(cat(h0["grads"]), cat(o["grads"])) > 0.05


def test_composition_average_pooling(dev):
    import _pool_ref as pr
    from test_cls_tail_gpu import case, hip_pass
    from test_pool_gpu import avg_model

    rc, sd, flux, labels, _, _ = case("rope")
    model = no_dropout(avg_model(rc, sd, dev, "32"))
    x, y = flux.to(dev), labels.to(dev)
    step = lambda rc, params, flux, labels, masks: pr.oracle_step(rc, params, flux, labels, False, None)[:2]  # noqa: E731
    h0, h1, o, _ = chain("average pooling", model, lambda m: hip_pass(m, x, y, True, tail=True), rc, sd, flux, labels, None,
                         0.02, False, step=step)
    assert model.engine._last["pool"] == "avg"
    check_fp32("average pooling", h1, o)
    assert rel(cat(h0["grads"]), cat(o["grads"])) > 0.05


def test_composition_masked_modelling(dev):
    import _mim_ref as mr
    from test_cls_tail_gpu import case
    from test_mim_gpu import mim_model, mim_pass, mim_state, step_mask

    rc, sd, flux, _, _, _ = case("rope")
    state = mim_state(rc, sd, 71)
    m = step_mask(rc, flux.shape[0])
    model = no_dropout(mim_model(rc, state, dev, "32", "mse"))
    x, md = flux.to(dev), torch.from_numpy(m).to(dev)
    handed = {}

    def run(mod):
        out, grads = mim_pass(mod, x, bool_masked_pos=md)
        handed["out"] = out
        return dict(loss=float(out.loss.detach()), logits=out.reconstruction.detach().cpu(), grads=grads)

    step = lambda rc, params, flux, labels, masks: mr.oracle_step(rc, params, flux, m, "mse", False, False, None)[:2]  # noqa: E731
    h0, h1, o, _ = chain("mim", model, run, rc, state, flux, None, None, 0.02, False, step=step)
    check_fp32("mim", h1, o)  # `logits`: the reconstruction handed out keeps the first pass's values
    out = handed["out"]
    assert np.array_equal(out.mask.cpu().numpy(), m) and len(out.hidden_states) == rc.num_hidden_layers + 1
    assert out.reconstruction.untyped_storage().data_ptr() != model.engine.act["mim_pred"].untyped_storage().data_ptr()
    assert rel(cat(h0["grads"]), cat(o["grads"])) > 0.05


def test_composition_soft_targets(dev):
    import _pool_ref as pr
    from oracle import refvit
    from test_cls_tail_gpu import hip_pass
    from test_pool_gpu import CLS5, avg_model

    rc = refvit.RefConfig(**CLS5)
    sd = refvit.make_state_dict(rc, 101)
    flux, _, _ = refvit.make_inputs(rc, 5, 102)
    t = torch.softmax(2 * torch.randn(5, rc.num_labels, generator=torch.Generator().manual_seed(103)), -1)
    model = no_dropout(avg_model(rc, sd, dev, "32", global_pool="token"))
    model.engine.set_soft_loss("ce")
    x, y = flux.to(dev), t.to(dev)

    def step(rc, params, flux, labels, masks):
        out = refvit.forward(rc, params, flux, None, training=False)
        return pr.head_loss(rc, out.logits, labels, "ce"), out.logits

    h0, h1, o, _ = chain("soft ce", model, lambda m: hip_pass(m, x, y, True, tail=True), rc, sd, flux, t, None, 0.02, False,
                         step=step)
    check_fp32("soft ce", h1, o)
    assert rel(cat(h0["grads"]), cat(o["grads"])) > 0.05


# ------------------------------------------------------------------ 5. the captured step
def test_hip_graph_replay_is_the_eager_two_pass_step(dev):
    """lr = 0: the replay is a step of the same weights.  Its loss and every gradient element are the eager SAM step's under the
    same bound record, bit for bit, written over a NaN fill; two replays differ from each other (fresh masks)."""
    import vit_amd.functional as vf
    from test_cls_tail_gpu import build, case
    from vit_amd import _cabi
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedAdamW

    rc, sd, flux, labels, _, _ = case("l3")
    model = build(rc, sd, dev, "bf16-mixed")
    sam = model.set_sam(RHO[("l3", False)])
    eng = model.engine
    eng.overlap_dw = False  # the captured step runs on one stream; so does the eager one it is compared with
    x, y = flux.to(dev), labels.to(dev)
    eng.base_seed, eng.step_counter = BASE_SEED, 0
    opt = FusedAdamW(model, lr=0.0)
    opt.set_grad_clip(0.5)
    module = types.SimpleNamespace(model=model, noise_level=0, train=model.train)
    warmup = 2
    eng._ensure_device_state()
    flat0, shadow0 = eng.flat.detach().clone(), eng.shadow.clone()
    gs = GraphedTrainStep(module, opt, (x, None, y), warmup=warmup)
    assert any(t is sam.backup for t in gs._held if isinstance(t, torch.Tensor))
    lay = eng.layout
    n = lay.n_trainable
    nan_fill(eng)
    loss = gs.step((x, None, y)).clone()
    torch.cuda.synchronize(dev)
    grads = tensors(eng)
    assert bool(torch.isfinite(grads).all()) and float(lay.view(eng.grads, "vit.layernorm.weight").abs().max()) > 0
    assert sam.perturbed is False and torch.equal(bits(eng.flat), bits(flat0)) and torch.equal(bits(eng.shadow), bits(shadow0))
    # the eager two-pass step under a record advanced to the same step
    h = eng.handle()
    record = torch.zeros(8, dtype=torch.int32, device=dev)
    eng.step_counter = warmup
    nan_fill(eng)
    dloss = torch.ones(1, device=dev)
    _cabi.check(h.lib.vit_step_state_bind(h.h, record.data_ptr()), "vit_step_state_bind")
    try:
        with vf.use_handle(h):
            _cabi.check(h.lib.vit_step_advance(h.h, BASE_SEED, 0.9, 0.999, vf._stream(record)), "vit_step_advance")
        eager, _, _, _ = eng.forward(x, y, training=True, need_grad=True)
        eng.backward(dloss)
        plain = tensors(eng)
        sam.ascend()
        eng.forward(x, y, training=True, need_grad=True, reuse_step=True)
        eng.backward(dloss)
        sam.descend()
        torch.cuda.synchronize(dev)
    finally:
        _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
    assert torch.equal(eager, loss), (float(eager), float(loss))
    assert torch.equal(bits(tensors(eng)), bits(grads))  # every element rewritten over the NaN fill, with the replay's bits
    assert rel(plain, grads) > 0.05  # ... which are the second pass's, not the first's
    # the next replay draws fresh masks
    loss2 = gs.step((x, None, y)).clone()
    torch.cuda.synchronize(dev)
    assert not torch.equal(tensors(eng), grads) and float(loss2) != float(loss)
    assert torch.equal(bits(eng.flat), bits(flat0))


# ------------------------------------------------------------------ 6. the Trainer
def trainer_run(steps, **train):
    from test_trainer_gpu import Batches, c1_config, make

    cfg = c1_config(**train)
    module, trainer = make(cfg)
    module.model.config.hidden_dropout_prob = 0.0
    module.model.config.attention_probs_dropout_prob = 0.0
    trainer._setup(module)
    module.train()
    b = tuple(t.cuda() for t in next(iter(Batches(16, 5))))
    losses, flats = [], []
    for i in range(steps):
        losses.append(float(trainer.training_step(module, b, i).detach()))
        flats.append(module.model.engine.flat.detach().clone())
    torch.cuda.synchronize()
    return module, trainer, losses, flats


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hip_graph"])
def test_trainer_steps(dev, graph):
    precision = "bf16-mixed"
    module, trainer, losses, flats = trainer_run(4, precision=precision, hip_graph=graph, sam_rho=0.01)
    sam = module.model.sam
    assert sam is not None and sam.rho == 0.01 and sam.adaptive is False and sam.perturbed is False
    assert trainer.use_graph is graph and (not graph or trainer._graphed)
    print(f"[sam trainer {'graph' if graph else 'eager'}] losses {losses}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert trainer.global_step == 4 and module.model.engine.step_counter == 4
    _, plain_trainer, plain_losses, plain_flats = trainer_run(1, precision=precision, hip_graph=graph)
    assert plain_losses[0] == losses[0]  # the logged loss is the first pass's
    assert not torch.equal(plain_flats[0], flats[0])  # the step used the second gradient


def test_trainer_refuses_accumulation_and_averages_the_restored_weights(dev):
    from test_trainer_gpu import c1_config, make

    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        make(c1_config(sam_rho=0.05, accumulate_grad_batches=2))
    module, trainer, losses, flats = trainer_run(2, precision="32", sam_rho=0.01, ema_decay=0.9)
    avg, n = trainer.averager, module.model.engine.layout.n_trainable
    assert avg.n_averaged == 2 and module.model.sam.perturbed is False
    want = torch.lerp(flats[0][:n], flats[1][:n], 0.1)  # first update: a copy of the stepped (restored) weights
    assert rel(avg.flat[:n], want) < 1e-6


# ------------------------------------------------------------------ 7. two gloo ranks on one GPU
def _ranks(tmp_path, world):
    child = os.path.join(ROOT, "tests", "_sam_ddp_child.py")
    out = tmp_path / f"w{world}"
    out.mkdir()
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "VIT_DIST_SINGLE", "VIT_DIST_BACKEND")}
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
    procs = [subprocess.Popen([sys.executable, child, str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for env in envs]
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0] * world, "\n".join(o[-2000:] for o in outs)
    return [torch.load(out / f"rank{r}.pt", weights_only=True) for r in range(world)]


def test_two_ranks_exchange_the_second_gradient_only(tmp_path):
    """Every rank perturbs by its local gradient (m-sharpness) and exchanges the second backward alone: the replicas stay
    bit-identical, the exchanged gradient is the mean of the two shards' single-process SAM gradients (the fp32 gates), and the
    reducer saw the buckets of one backward per step."""
    single = _ranks(tmp_path, 1)[0]
    r0, r1 = _ranks(tmp_path, 2)
    n = single["n_trainable"]
    assert r0["world"] == r1["world"] == 2 and single["world"] == 1
    assert torch.equal(r0["params"], r1["params"]) and not torch.equal(r0["params"], single["start"])
    assert torch.equal(r0["grad_step1"], r1["grad_step1"])
    want = 0.5 * (single["shard_grads"][0].double() + single["shard_grads"][1].double())
    local = 0.5 * (single["shard_plain"][0].double() + single["shard_plain"][1].double())
    worst = 0.0
    for name, (lo, hi) in single["spans"].items():
        w = want[lo:hi]
        if float(w.norm()) < 1e-6 * float(want.norm()):
            continue
        worst = max(worst, float((r0["grad_step1"][lo:hi].double() - w).norm() / w.norm()))
    apart = float((local[:n] - want[:n]).norm() / want[:n].norm())
    print(f"[sam ddp] exchanged gradient against the mean of the shards' SAM gradients: worst tensor {worst:.2e}; the mean of "
          f"their plain gradients is {apart:.3f} away")
    # the control: the mean of the plain gradients must miss the gate by a factor of ten, or the gate would not tell the two apart
    assert worst < 2e-4 and apart > 10 * 2e-4
    for r in (r0, r1):
        assert r["bucket_calls"] == [r["n_buckets"]] * 2, r["bucket_calls"]  # one backward's buckets per step, not two


# ------------------------------------------------------------------ 8. the poison table
# tests/test_poison_cpu.py demands that every exported vit_* name is a case of tests/test_poison_gpu.py's table or listed in its
# EXEMPT dict with a reason.  The three exports of include/vit_amd_sam.h are listed there from here, when this module is imported
# (pytest imports every test module before it runs the first test): the kernel tests above poison their outputs and the workspace.
def _list_in_poison_table():
    import test_poison_gpu as table

    here = "poisoned by tests/test_sam_gpu.py"
    for name in ("vit_sam_sqnorm", "vit_sam_ascend", "vit_sam_descend"):
        table.EXEMPT.setdefault(name, here)


_list_in_poison_table()
