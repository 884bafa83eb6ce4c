"""Masked spectrum modelling (`model.task_type: mim`, include/vit_amd_mim.h) on the GPU: the mask expansion against its host
restatement (tests/_mim_ref.py) bit for bit; the masked embedding kernels against their plain twins and the formula; the loss
kernels against the torch restatement and its autograd; argument errors; the model against the UNCHANGED CPU oracle (whose
tokenizer is wrapped at call time so that masked tokens become `mask_token`, plus the torch decoder and loss) at the bounds
tests/test_droppath_gpu.py applies to the same cases; that nothing moved for a 'reg' model; the captured step; gradient
accumulation; and the shipped YAML end to end, with the `model.init_from` hand-over to a regression run.
Outputs and the workspace are poisoned before the kernel calls (tests/_poison.py)."""
import os
import types

import numpy as np
import pytest
import torch

import _mim_ref as mr
from _patchdrop_ref import select_site
from _poison import IntOut, poisoned
from oracle import dropmask as dm

pytestmark = pytest.mark.gpu

BASE_SEED = 0x5DEECE66D2468ACE  # tests/test_cls_tail_gpu.py: hip_pass runs step STEP of this seed
STEP = 3
RATIO, SPAN = 0.5, 2
L1, MSE = 1, 0  # VIT_LOSS_L1, VIT_LOSS_MSE


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def equal_either(out, e_plain, e_fma):  # tests/test_dropout_gpu.py
    return bool(((out == e_plain) | (out == e_fma)).all())


def I32(dev, *s):
    return torch.empty(s, dtype=torch.int32, device=dev)


def random_mask(B, N, seed, must=None):
    """int32 [B, N], about half masked, every sample with a masked and (N > 1) a visible patch; `must`: a patch all mask."""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, N, generator=g) < 0.5).to(torch.int32)
    m[:, 0] = 1
    if N > 1:
        m[:, 1] = 0
    if must is not None:
        m[:, must] = 1
    return m


# ------------------------------------------------------------------ 1. the mask expansion
@pytest.mark.parametrize("B,N,span", [(3, 1, 1), (5, 13, 3), (4, 196, 4), (2, 4089, 7)])
def test_mask_kernel_is_the_restatement(dev, B, N, span):
    import vit_amd.functional as vf

    seed, site, ratio = 0x1234567, 49, 0.6
    Nb, Kb = mr.blocks(N, span, ratio)
    idx, slot, mask = I32(dev, B, Kb), I32(dev, B, Nb), I32(dev, B, N)

    def run():
        vf.patch_select(B, Nb, Kb, seed, site, idx, slot)
        vf.mim_mask(slot, span, mask)

    got = poisoned(dev, run, [IntOut(idx, Nb - 1), IntOut(slot, Kb - 1), IntOut(mask, 1)])[2]
    want = mr.mask(B, N, span, ratio, seed, site)
    assert np.array_equal(got.cpu().numpy(), want)
    if N == 13:  # the short last block: one patch
        assert Nb * span - N == 2 and {int(want[:, -1:].sum(1)[b]) for b in range(B)} <= {0, 1}


def test_mask_under_a_bound_step_record(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    B, N, span, ratio, seed, site = 5, 196, 4, 0.6, 0x1234567, 49
    Nb, Kb = mr.blocks(N, span, ratio)
    h = _cabi.Handle(dev.index or 0)
    base, step = 0x1234567, 7
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    state[5] = step - 1
    kx = dm.step_keys(base, step)
    _cabi.check(h.lib.vit_step_state_bind(h.h, state.data_ptr()), "vit_step_state_bind")
    try:
        with vf.use_handle(h):
            _cabi.check(h.lib.vit_step_advance(h.h, base, 0.9, 0.999, vf._stream(state)), "vit_step_advance")
            _, slot = vf.patch_select(B, Nb, Kb, seed, site, I32(dev, B, Kb), I32(dev, B, Nb))
            mask = vf.mim_mask(slot, span, I32(dev, B, N).fill_(-7))
        torch.cuda.synchronize(dev)
    finally:
        _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
    want = mr.mask(B, N, span, ratio, seed, site, keys_xor=kx)
    assert np.array_equal(mask.cpu().numpy(), want) and not np.array_equal(want, mr.mask(B, N, span, ratio, seed, site))


# ------------------------------------------------------------------ 2. embedding finish, masked: forward
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("D", [32, 768])
def test_embed_finish_masked_forward(dev, D, with_pos, p):
    import vit_amd.functional as vf

    B, N, seed = 3, 13, 2 ** 64 - 3
    T = N + 1
    tok = randn((B, T, D), dev, 412)
    cls, mtok = randn((D,), dev, 413), randn((D,), dev, 415)
    pos = randn((T, D), dev, 414) if with_pos else None
    zero = torch.zeros(B, N, dtype=torch.int32, device=dev)
    plain = vf.embed_finish(tok.clone(), cls, pos, dropout=(p, seed, 0))
    assert torch.equal(vf.embed_finish_masked(tok.clone(), cls, zero, mtok, pos, dropout=(p, seed, 0)), plain)
    m = random_mask(B, N, 416).to(dev)
    out = vf.embed_finish_masked(tok.clone(), cls, m, mtok, pos, dropout=(p, seed, 0))
    v = tok.clone()
    v[:, 0] = cls
    v[:, 1:] = torch.where(m[:, :, None] != 0, mtok[None, None, :], v[:, 1:])
    mult = torch.from_numpy(dm.hidden_multiplier(dm.drop_cfg(p, seed, 0), B, T, D)).to(dev)
    if with_pos:
        e_plain, e_fma = (v + pos[None]) * mult, ((v.double() + pos[None].double()) * mult.double()).float()
    else:
        e_plain = e_fma = v * mult
    assert equal_either(out, e_plain, e_fma)
    assert p == 0.0 or 0 < int((out == 0).sum()) < out.numel()
    # a masked row does not depend on its projected token: NaN there, the same finite output
    bad = tok.clone()
    bad[:, 1:][m != 0] = float("nan")
    bad[:, 0] = float("nan")  # the CLS row is never read either
    again = vf.embed_finish_masked(bad, cls, m, mtok, pos, dropout=(p, seed, 0))
    assert bool(torch.isfinite(again).all()) and torch.equal(again, out)


# ------------------------------------------------------------------ 3. embedding finish, masked: backward
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,D,with_pos,p", [(3, 32, False, 0.0), (3, 32, True, 0.1), (3, 768, False, 0.1), (3, 768, True, 0.0),
                                            (3, 768, True, 0.1), (3, 32, True, 0.0), (3, 32, False, 0.1), (3, 768, False, 0.0),
                                            (37, 32, True, 0.1)])  # B = 37: batch chunks of more than one sample
def test_embed_finish_masked_backward(dev, B, D, with_pos, p, dt):
    import vit_amd.functional as vf

    N, seed = 13, 41
    T = N + 1
    dtok = randn((B, T, D), dev, 423)
    E = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)

    def plain_call():
        dcls, dpos = E(D), (E(T, D) if with_pos else None)
        dpatch = torch.empty(B * N, D, dtype=dt, device=dev)
        poisoned(dev, lambda: vf.embed_finish_bwd(dtok, dcls, dpos, dropout=(p, seed, 0), dpatch=dpatch),
                 [dpatch, dcls] + ([dpos] if with_pos else []))
        return dpatch, dcls, dpos

    def masked_call(m):
        dcls, dmt, dpos = E(D), E(D), (E(T, D) if with_pos else None)
        dpatch = torch.empty(B * N, D, dtype=dt, device=dev)
        # two rounds over different poison: finite and bit-identical, dmask_token included
        poisoned(dev, lambda: vf.embed_finish_masked_bwd(dtok, m, dcls, dmt, dpos, dropout=(p, seed, 0), dpatch=dpatch),
                 [dpatch, dcls, dmt] + ([dpos] if with_pos else []))
        return dpatch, dcls, dpos, dmt

    p_patch, p_cls, p_pos = plain_call()
    zero = torch.zeros(B, N, dtype=torch.int32, device=dev)
    z_patch, z_cls, z_pos, z_mt = masked_call(zero)
    assert torch.equal(z_patch, p_patch) and torch.equal(z_cls, p_cls) and (not with_pos or torch.equal(z_pos, p_pos))
    assert bool((z_mt == 0).all())
    m = random_mask(B, N, 426).to(dev)
    r_patch, r_cls, r_pos, r_mt = masked_call(m)
    mb = (m != 0)
    rp, pp = r_patch.view(B, N, D), p_patch.view(B, N, D)
    assert bool((rp[mb] == 0).all()) and torch.equal(rp[~mb], pp[~mb])
    assert torch.equal(r_cls, p_cls) and (not with_pos or torch.equal(r_pos, p_pos))  # the same sums, whatever the mask
    mult = torch.from_numpy(dm.hidden_multiplier(dm.drop_cfg(p, seed, 0), B, T, D)).to(dev)
    want = ((dtok * mult)[:, 1:].double() * mb[:, :, None].double()).sum((0, 1)).cpu()
    e = rel(r_mt, want)
    print(f"[embed masked bwd B={B} D={D} pos={with_pos} p={p} {dt}] dmask_token rel error {e:.2e}")
    assert e < 1e-5
    # accumulate stores old + new (new = what overwrite mode stores, bit for bit)
    old_cls, old_mt, old_pos = randn((D,), dev, 427), randn((D,), dev, 428), (randn((T, D), dev, 429) if with_pos else None)
    a_cls, a_mt, a_pos = old_cls.clone(), old_mt.clone(), (old_pos.clone() if with_pos else None)
    a_patch = vf.embed_finish_masked_bwd(dtok, m, a_cls, a_mt, a_pos, dropout=(p, seed, 0), out_dtype=dt, accumulate=True)
    assert torch.equal(a_patch, r_patch) and torch.equal(a_cls, old_cls + r_cls) and torch.equal(a_mt, old_mt + r_mt)
    assert not with_pos or torch.equal(a_pos, old_pos + r_pos)


# ------------------------------------------------------------------ 4. the loss kernels
def loss_case(L, P, S, B, dt, norm, kind, seed0):
    """x, pred (rounded to `dt`), a mask with the ragged tail's zero window forced in -- at the first seed >= seed0 for which no
    masked |pred - target| is below 1e-3 (L1's precondition: no sign can flip by rounding); asserted on the CPU."""
    N = -(-(L - P) // S) + 1
    ragged = (L - P) % S != 0
    m = random_mask(B, N, 431, must=N - 1 if ragged else None)
    for seed in range(seed0, seed0 + 200):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, L, generator=g)
        pred = torch.randn(B * (N + 1), P, generator=g).to(dt)
        d = (pred.float().view(B, N + 1, P)[:, 1:] - mr.targets(x, P, S, N, norm)).abs()
        if kind != "l1" or float(d[m != 0].min()) > 1e-3:
            assert kind != "l1" or float(d[m != 0].min()) > 1e-3
            return N, ragged, x, pred, m
    raise AssertionError("no seed satisfies the L1 precondition")


def bf16_neighbours(g):
    """The two bf16 values that bracket the f32 tensor g (equal when g is a bf16 value), as f32."""
    bits = g.contiguous().view(torch.int32)
    down = bits & -65536  # toward zero
    up = torch.where(bits == down, down, down + 65536)  # away from zero
    return down.view(torch.float32), up.view(torch.float32)


def check_loss(dev, x, pred, m, P, S, kind, norm, dt, tag):
    import vit_amd.functional as vf

    B, N = m.shape
    T = N + 1
    pf = pred.float().clone().requires_grad_(True)
    want = mr.loss(pf.view(B, T, P)[:, 1:], x, m, P, S, kind, norm)
    want.backward()
    want = want.detach()
    xd, pd, md = x.to(dev), pred.to(dev), m.to(dev)
    loss, count = torch.empty((), device=dev), torch.empty((), dtype=torch.int32, device=dev)
    k = L1 if kind == "l1" else MSE
    poisoned(dev, lambda: vf.mim_loss_fwd(xd, pd, md, P, S, k, norm, loss=loss, count=count), [loss, IntOut(count, 7)])
    assert int(count) == int(m.sum())
    e = abs(float(loss) - float(want)) / max(abs(float(want)), 1e-30) if int(m.sum()) else abs(float(loss))
    dloss = torch.ones(1, device=dev)
    dpred = torch.empty(B * T, P, dtype=dt, device=dev)
    poisoned(dev, lambda: vf.mim_loss_bwd(xd, pd, md, count, dloss, P, S, k, norm, dpred=dpred), [dpred], workspace=False)
    got = dpred.view(B, T, P).cpu()
    masked = torch.cat([torch.zeros(B, 1, dtype=torch.bool), m != 0], dim=1)
    assert bool((got[~masked] == 0).all()), tag  # CLS rows and unmasked windows: exact zeros
    auto = pf.grad.view(B, T, P)
    assert bool((auto[~masked] == 0).all())
    if dt == torch.float32:
        eg = rel(got[masked], auto[masked]) if int(m.sum()) else 0.0
        print(f"[mim loss {tag}] loss rel error {e:.2e}, dpred rel error {eg:.2e}")
        assert eg < 1e-5, tag
    else:
        lo, hi = bf16_neighbours(auto[masked])
        mine = got[masked].float()
        ok = (mine == lo) | (mine == hi) | (mine == auto[masked].to(torch.bfloat16).float())
        print(f"[mim loss {tag}] loss rel error {e:.2e}, dpred: {int((~ok).sum())} of {ok.numel()} off autograd's bf16 neighbours")
        assert bool(ok.all()), tag
    assert e < 1e-5, (tag, float(loss), float(want))
    return float(loss), got


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", ["l1", "mse"])
@pytest.mark.parametrize("L,P,S", [(64, 8, 1), (103, 16, 12), (1024, 256, 256)])
def test_loss_kernels_against_the_restatement(dev, L, P, S, kind, norm, dt):
    B = 3
    N, ragged, x, pred, m = loss_case(L, P, S, B, dt, norm, kind, 440)
    if ragged:  # a masked zero-padded window occurs
        assert N * S + P - S > L and bool((m[:, N - 1] == 1).all()) and float(mr.targets(x, P, S, N)[:, N - 1].abs().max()) == 0
    tag = f"L={L} P={P} S={S} {kind} norm={norm} {dt}"
    check_loss(dev, x, pred, m, P, S, kind, norm, dt, tag)
    if dt == torch.float32 and not norm:
        ones = torch.ones_like(m)
        check_loss(dev, x, pred, ones, P, S, kind, norm, dt, tag + " all masked")
        one = torch.zeros_like(m)
        one[B - 1, N - 1] = 1
        check_loss(dev, x, pred, one, P, S, kind, norm, dt, tag + " one window")
        loss0, g0 = check_loss(dev, x, pred, torch.zeros_like(m), P, S, kind, norm, dt, tag + " m = 0")
        assert loss0 == 0.0 and bool((g0 == 0).all())


# ------------------------------------------------------------------ 5. argument errors
def test_argument_errors_launch_nothing(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    B, N, P, D = 2, 8, 8, 32
    h = vf._h(torch.empty(1, device=dev))
    st = torch.cuda.current_stream(dev).cuda_stream
    SENT = -12345.0
    x, pred = randn((B, 64), dev, 451), randn((B * (N + 1), P), dev, 452)
    mask, slot = torch.ones(B, N, dtype=torch.int32, device=dev), torch.zeros(B, N, dtype=torch.int32, device=dev)
    outs = dict(loss=torch.full((), SENT, device=dev), count=torch.full((), -5, dtype=torch.int32, device=dev),
                dpred=torch.full((B * (N + 1), P), SENT, device=dev), tok=torch.full((B, N + 1, D), SENT, device=dev),
                dpatch=torch.full((B * N, D), SENT, device=dev), dcls=torch.full((D,), SENT, device=dev),
                dmt=torch.full((D,), SENT, device=dev), m=torch.full((B, N), -5, dtype=torch.int32, device=dev))
    ptr = {k: v.data_ptr() for k, v in outs.items()}
    cls, dloss = randn((D,), dev, 453), torch.ones(1, device=dev)
    lib, hh = h.lib, h.h
    calls = [
        (lambda: lib.vit_mim_mask(hh, slot.data_ptr(), ptr["m"], B, N, N, 0, st), b"span=0"),
        (lambda: lib.vit_mim_mask(hh, None, ptr["m"], B, N, N, 1, st), b"null pointer"),
        (lambda: lib.vit_mim_mask(hh, slot.data_ptr(), ptr["m"], B, N, N - 1, 1, st), b"Nb="),
        (lambda: lib.vit_embed_finish_masked(hh, ptr["tok"], cls.data_ptr(), None, mask.data_ptr(), None, B, N + 1, D, 0.0, 1, 0, st),
         b"null pointer"),
        (lambda: lib.vit_embed_finish_masked_bwd(hh, ptr["tok"], None, ptr["dpatch"], 0, ptr["dcls"], None, ptr["dmt"], B, N + 1, D,
                                                 0.0, 1, 0, 0, st), b"null pointer"),
        (lambda: lib.vit_mim_loss_fwd(hh, x.data_ptr(), pred.data_ptr(), 0, mask.data_ptr(), ptr["loss"], ptr["count"], B, 64, P, 8, N,
                                      N, L1, 0, st), b"must be N + 1"),
        (lambda: lib.vit_mim_loss_fwd(hh, x.data_ptr(), pred.data_ptr(), 0, mask.data_ptr(), ptr["loss"], ptr["count"], B, 64, P, 8, N,
                                      N + 1, 2, 0, st), b"kind 2"),
        (lambda: lib.vit_mim_loss_fwd(hh, x.data_ptr(), pred.data_ptr(), 0, None, ptr["loss"], ptr["count"], B, 64, P, 8, N, N + 1, L1,
                                      0, st), b"null pointer"),
        (lambda: lib.vit_mim_loss_bwd(hh, x.data_ptr(), pred.data_ptr(), 0, mask.data_ptr(), ptr["count"], dloss.data_ptr(),
                                      ptr["dpred"], 0, B, 64, P, 8, N, N + 2, MSE, 0, st), b"must be N + 1"),
        (lambda: lib.vit_mim_loss_bwd(hh, x.data_ptr(), pred.data_ptr(), 0, mask.data_ptr(), ptr["count"], dloss.data_ptr(),
                                      ptr["dpred"], 0, B, 64, P, 8, N, N + 1, 3, 0, st), b"kind 3"),
        (lambda: lib.vit_mim_loss_bwd(hh, x.data_ptr(), pred.data_ptr(), 0, mask.data_ptr(), ptr["count"], None, ptr["dpred"], 0, B,
                                      64, P, 8, N, N + 1, MSE, 0, st), b"null pointer"),
    ]
    for call, text in calls:
        assert call() == -1  # VIT_ERR_ARG
        assert text in lib.vit_last_error(), (text, lib.vit_last_error())
    with pytest.raises(_cabi.VitError, match="span"):
        vf.mim_mask(slot, 0, outs["m"])
    torch.cuda.synchronize(dev)
    for k, v in outs.items():  # nothing was launched: every output still holds its sentinel
        assert bool((v == (-5 if v.dtype == torch.int32 else SENT)).all()), k


# ------------------------------------------------------------------ 6. the model against the oracle
_oracle = {}


def mim_state(rc, sd, seed):
    """The case's state dict plus the 'mim' model's own tensors: a non-zero mask token (its value and its gradient path are
    both exercised; the same for every seed) and a decoder drawn from `seed`."""
    D, P = rc.hidden_size, rc.patch_size
    g = torch.Generator().manual_seed(seed)
    extra = {mr.MASK_TOKEN: 0.5 * torch.randn(1, 1, D, generator=torch.Generator().manual_seed(70)),
             "decoder.weight": torch.randn(P, D, generator=g) / D ** 0.5, "decoder.bias": 0.02 * torch.randn(P, generator=g)}
    return dict(sd, **extra)


def mim_model(rc, state, dev, precision, kind, norm=False):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    cfg = ViTConfig(task_type="mim", image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                    num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
                    stride_size=rc.stride_size, pos_encoding_type=rc.pos_encoding_type, rope_base=rc.rope_base,
                    mim_mask_ratio=RATIO, mim_span=SPAN, mim_loss=kind, mim_norm_target=norm)
    model = MyViT(cfg, loss_name="")
    model.set_precision(precision)
    model.load_state_dict({k: v for k, v in state.items() if not k.startswith("regressor.")}, strict=True)
    return model.to(dev)


def step_mask(rc, B, keys_xor=None, seed=None):
    seed = dm.step_seed(BASE_SEED, STEP) if seed is None else seed
    return mr.mask(B, rc.num_patches, SPAN, RATIO, seed, select_site(rc.num_hidden_layers), keys_xor=keys_xor)


def oracle_mim(tag, kind):
    """(rc, state, flux, gtol, oracle results) of one case and loss: the CPU oracle's training step with the restated dropout
    masks and block mask of step STEP, its gradients by autograd, and its hidden states under the complementary mask.  For L1
    the decoder's seed is the first whose oracle residuals |rec - target| over the masked windows all exceed 1e-3 (the encoder's
    output does not depend on the decoder, so the search costs one Linear per seed)."""
    from test_cls_tail_gpu import case

    key = (tag, kind)
    if key in _oracle:
        return _oracle[key]
    rc, sd, flux, _, _, gtol = case(tag)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    B = flux.shape[0]
    m = step_mask(rc, B)
    masks = dm.engine_masks(rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, dm.step_seed(BASE_SEED, STEP), None)
    seed = 71
    if kind == "l1":
        tgt, mb = mr.targets(flux, rc.patch_size, rc.stride, rc.num_patches), torch.from_numpy(m) != 0
        with torch.no_grad():
            _, _, enc = mr.oracle_step(rc, mim_state(rc, sd, seed), flux, m, kind, False, True, masks)
            rows = enc.last_hidden_state[:, 1:, :][mb]
            for seed in range(71, 20071):
                st = mim_state(rc, sd, seed)
                if float((torch.nn.functional.linear(rows, st["decoder.weight"], st["decoder.bias"]) - tgt[mb]).abs().min()) > 1e-3:
                    break
    state = mim_state(rc, sd, seed)
    params = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    loss, rec, out = mr.oracle_step(rc, params, flux, m, kind, False, True, masks)
    resid = (rec.detach() - mr.targets(flux, rc.patch_size, rc.stride, rc.num_patches)).abs()[torch.from_numpy(m) != 0]
    assert kind != "l1" or float(resid.min()) > 1e-3, f"no decoder seed satisfies the L1 precondition (last {seed})"
    loss.backward()
    with torch.no_grad():
        _, _, wrong = mr.oracle_step(rc, state, flux, 1 - m, kind, False, True, masks)
    o = dict(loss=float(loss.detach()), rec=rec.detach(), hs=torch.stack([h.detach() for h in out.hidden_states]),
             hs_wrong=torch.stack(wrong.hidden_states), mask=m,
             grads={k: p.grad for k, p in params.items() if p.grad is not None})
    _oracle[key] = (rc, state, flux, gtol, o)
    return _oracle[key]


def mim_pass(model, x, step=STEP, **kw):
    eng = model.engine
    model.train()
    eng.base_seed, eng.step_counter = BASE_SEED, step - 1
    for p in model.parameters():
        p.grad = None
    out = model(x, output_hidden_states=True, **kw)
    out.loss.backward()
    lay = eng.layout
    grads = {n: lay.view(eng.grads, n).detach().clone().cpu() for n, (off, _) in lay.entries.items() if off < lay.n_trainable}
    return out, grads


def grad_errors(grads, o):
    gmax = max(float(g.norm()) for g in o["grads"].values())
    assert set(grads) == set(o["grads"])  # every trainable slice has an oracle gradient, and the other way round
    errs = {}
    for name, g in o["grads"].items():
        mine, r = grads[name].double().flatten(), g.double().flatten()
        if float(r.norm()) < 1e-6 * gmax:  # key.bias: analytically zero
            assert float(mine.norm()) < 2e-3 * gmax, name
            continue
        errs[name] = (float((mine - r).norm() / r.norm()), float(torch.dot(mine, r) / (mine.norm() * r.norm() + 1e-30)))
    return errs


@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("tag", ["l3", "rope"])
def test_model_is_the_oracle_fp32(dev, tag, kind):
    """6a and 6c at precision '32': hidden states, reconstruction and loss < 1e-4, every gradient tensor < 2e-4."""
    rc, state, flux, _, o = oracle_mim(tag, kind)
    model = mim_model(rc, state, dev, "32", kind)
    out, grads = mim_pass(model, flux.to(dev))
    assert np.array_equal(out.mask.cpu().numpy(), o["mask"]) and 0 < int(o["mask"].sum()) < o["mask"].size
    assert out.reconstruction.shape == o["rec"].shape and len(out.hidden_states) == rc.num_hidden_layers + 1
    hs = torch.stack([h.cpu() for h in out.hidden_states])
    e_hs, e_rec, e_loss = rel(hs, o["hs"]), rel(out.reconstruction, o["rec"]), abs(float(out.loss.detach()) - o["loss"]) / o["loss"]
    errs = grad_errors(grads, o)
    worst = max(errs.items(), key=lambda kv: kv[1][0])
    e_wrong = rel(hs, o["hs_wrong"])
    print(f"[mim {tag} 32 {kind}] hidden {e_hs:.2e} (complementary mask {e_wrong:.2e}), reconstruction {e_rec:.2e}, loss {e_loss:.2e}, "
          f"worst gradient {worst[1][0]:.2e} ({worst[0]}); mask_token {errs[mr.MASK_TOKEN][0]:.2e}, "
          f"decoder.weight {errs['decoder.weight'][0]:.2e}")
    assert e_hs < 1e-4 and e_rec < 1e-4 and e_loss < 1e-4
    for name, (r, _) in errs.items():
        assert r < 2e-4, (name, r)
    assert {mr.MASK_TOKEN, "decoder.weight", "decoder.bias"} <= set(errs)
    assert e_wrong >= 10 * e_hs  # 6c


@pytest.mark.parametrize("tag", ["l3", "rope"])
def test_model_is_the_oracle_bf16(dev, tag):
    """6b (MSE) and 6c at bf16-mixed: hidden states and reconstruction < 1.5e-2, the loss within tests/test_droppath_gpu.py's
    loss_tol rule, every gradient tensor < the case's gtol with cosine > 0.999."""
    rc, state, flux, gtol, o = oracle_mim(tag, "mse")
    model = mim_model(rc, state, dev, "bf16-mixed", "mse")
    out, grads = mim_pass(model, flux.to(dev))
    assert np.array_equal(out.mask.cpu().numpy(), o["mask"])
    hs = torch.stack([h.cpu() for h in out.hidden_states])
    e_hs, e_rec, e_loss = rel(hs, o["hs"]), rel(out.reconstruction, o["rec"]), abs(float(out.loss.detach()) - o["loss"]) / o["loss"]
    errs = grad_errors(grads, o)
    worst = max(errs.items(), key=lambda kv: kv[1][0])
    e_wrong = rel(hs, o["hs_wrong"])
    loss_tol = 3e-2
    if tag == "rope":  # tests/test_droppath_gpu.py: the rope case's rule
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "rope.npz"))
        loss_tol = 2 * float(g["p1_loss"]) ** -0.5 * 1.5e-2
    print(f"[mim {tag} bf16-mixed mse] hidden {e_hs:.2e} (complementary mask {e_wrong:.2e}), reconstruction {e_rec:.2e}, "
          f"loss {e_loss:.2e} (tol {loss_tol:.2e}), worst gradient {worst[1][0]:.2e} ({worst[0]}, gtol {gtol}); "
          f"mask_token {errs[mr.MASK_TOKEN]}, decoder.weight {errs['decoder.weight']}, decoder.bias {errs['decoder.bias']}")
    assert e_hs < 1.5e-2 and e_rec < 1.5e-2 and e_loss <= loss_tol
    for name, (r, c) in errs.items():
        assert r < gtol and c > 0.999, (name, r, c)
    assert e_wrong >= 10 * e_hs


def test_given_mask_eval_masks_and_norm_target(dev):
    """bool_masked_pos is used as given (and labels are ignored); eval-mode masks repeat after eval(); norm_target reaches the
    kernels: the loss is the restatement's on the engine's own reconstruction."""
    rc, state, flux, _, o = oracle_mim("l3", "mse")
    model = mim_model(rc, state, dev, "32", "mse", norm=True)
    x = flux.to(dev)
    B, N = flux.shape[0], rc.num_patches
    given = random_mask(B, N, 461)
    model.eval()
    with torch.no_grad():
        out = model(x, labels=torch.zeros(B, device=dev), bool_masked_pos=given.to(dev).bool())
    assert np.array_equal(out.mask.cpu().numpy(), given.numpy()) and model.engine.mim_mask is None
    want = mr.loss(out.reconstruction.cpu(), flux, given, rc.patch_size, rc.stride, "mse", True)
    assert abs(float(out.loss) - float(want)) <= 1e-5 * float(want)
    with torch.no_grad():
        model.eval()
        a = [model(x).mask.clone() for _ in range(2)]
        model.eval()
        b = [model(x[:, :].clone() * 2).mask.clone() for _ in range(2)]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], a[1])
    eng = model.engine
    seed0 = ((eng.base_seed ^ 0x6D696D5F6576616C) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    assert np.array_equal(a[0].cpu().numpy(), mr.mask(B, N, SPAN, RATIO, seed0, select_site(rc.num_hidden_layers)))
    with pytest.raises(ValueError, match="bool_masked_pos"):
        model(x, bool_masked_pos=torch.zeros(B, N + 1, dtype=torch.bool, device=dev))


# ------------------------------------------------------------------ 7. nothing else moves
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_a_reg_model_keeps_its_bits(dev, precision):
    """Two builds of the 'l3' regression model: one as it is -- every new branch taken on its "off" side -- and one whose
    embedding finish and its backward are the masked kernels under an all-zero mask (the "on" side with nothing masked).  Logits,
    loss and every gradient tensor are the same bits, with the CLS tail and without."""
    import vit_amd.functional as vf
    from test_cls_tail_gpu import build, case, hip_pass

    rc, sd, flux, labels, _, _ = case("l3")
    x, y = flux.to(dev), labels.to(dev)
    B, N, D = flux.shape[0], rc.num_patches, rc.hidden_size
    plain = build(rc, sd, dev, precision)
    assert not plain.engine.mim and "mim_mask" not in plain.engine.act
    zero, mtok = torch.zeros(B, N, dtype=torch.int32, device=dev), torch.full((D,), float("nan"), device=dev)
    sink = torch.empty(D, device=dev)
    fwd, bwd = vf.embed_finish, vf.embed_finish_bwd
    for tail in (True, False):
        a = hip_pass(plain, x, y, True, tail=tail)
        other = build(rc, sd, dev, precision)
        vf.embed_finish = lambda tok, cls, pos=None, dropout=vf.NO_DROP: vf.embed_finish_masked(tok, cls, zero, mtok, pos, dropout)
        vf.embed_finish_bwd = lambda dtok, dcls, dpos=None, dropout=vf.NO_DROP, dpatch=None: \
            vf.embed_finish_masked_bwd(dtok, zero, dcls, sink, dpos, dropout, dpatch)
        try:
            b = hip_pass(other, x, y, True, tail=tail)
        finally:
            vf.embed_finish, vf.embed_finish_bwd = fwd, bwd
        assert a["tail"] is tail and b["tail"] is tail
        assert a["loss"] == b["loss"] and torch.equal(a["logits"], b["logits"])
        for n in a["grads"]:
            assert torch.equal(a["grads"][n], b["grads"][n]), (tail, n)
        assert bool((sink == 0).all())
        assert "mim_mask" not in other.engine.act and "mim_dpred" not in other.engine.tmp


# ------------------------------------------------------------------ 8. the captured step
def test_hip_graph_replays_draw_the_restated_masks(dev):
    """lr = 0: every replay is a step of the same weights.  The mask of replay r is the restatement's under the record's keys of
    step r + 1, and its loss is the eager forward's under the same bound record, bit for bit."""
    import vit_amd.functional as vf
    from vit_amd import _cabi
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedAdamW

    rc, state, flux, _, _ = oracle_mim("l3", "mse")
    model = mim_model(rc, state, dev, "bf16-mixed", "mse")
    eng = model.engine
    x, labels = flux.to(dev), torch.zeros(flux.shape[0], device=dev)
    eng.base_seed, eng.step_counter = BASE_SEED, 0
    opt = FusedAdamW(model, lr=0.0)
    opt.set_grad_clip(0.5)
    module = types.SimpleNamespace(model=model, noise_level=0, train=model.train)
    warmup = 2
    gs = GraphedTrainStep(module, opt, (x, None, labels), warmup=warmup)
    seed_cap = dm.step_seed(BASE_SEED, warmup + 1)
    B = x.shape[0]
    seen, losses = [], []
    for r in range(2):
        loss = gs.step((x, None, labels)).clone()
        torch.cuda.synchronize(dev)
        want = step_mask(rc, B, keys_xor=dm.step_keys(BASE_SEED, r + 1), seed=seed_cap)
        assert np.array_equal(eng._last["mask"].cpu().numpy(), want), r
        seen.append(want)
        losses.append(loss)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], step_mask(rc, B, seed=seed_cap))
    # the eager forward of the same steps: the same host seed, the record advanced to the same step by hand
    h = eng.handle()
    record = torch.zeros(8, dtype=torch.int32, device=dev)
    for r in range(2):
        record[5] = r
        eng.step_counter = warmup
        _cabi.check(h.lib.vit_step_state_bind(h.h, record.data_ptr()), "vit_step_state_bind")
        try:
            with vf.use_handle(h):
                _cabi.check(h.lib.vit_step_advance(h.h, BASE_SEED, 0.9, 0.999, vf._stream(record)), "vit_step_advance")
            eager, _, _, _ = eng.forward(x, None, training=True, need_grad=True)
            torch.cuda.synchronize(dev)
        finally:
            _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
        assert np.array_equal(eng._last["mask"].cpu().numpy(), seen[r])
        assert torch.equal(eager, losses[r]), (r, float(eager), float(losses[r]))


# ------------------------------------------------------------------ 9. accumulation
def test_gradient_accumulation_adds_two_backwards(dev):
    rc, state, flux, _, _ = oracle_mim("l3", "mse")
    model = mim_model(rc, state, dev, "bf16-mixed", "mse")
    eng = model.engine
    x = flux.to(dev)
    model.train()
    lay = eng.layout

    def backward_of(step, fresh):
        eng.base_seed, eng.step_counter = BASE_SEED, step - 1
        if fresh:
            for p in model.parameters():
                p.grad = None
        model(x).loss.backward()
        return eng.grads[:lay.n_trainable].detach().clone()

    g1, g2 = backward_of(3, True), backward_of(4, True)
    assert not torch.equal(g1, g2)
    backward_of(3, True)
    both = backward_of(4, False)  # the parameters still hold the buffer's views: this backward accumulates
    want = g1 + g2
    for name in (mr.MASK_TOKEN, "decoder.weight", "decoder.bias", "vit.embeddings.cls_token", "vit.layernorm.weight"):
        e = rel(lay.view(both, name), lay.view(want, name))
        assert e < 1e-6 and float(lay.view(want, name).abs().max()) > 0, (name, e)
    assert rel(both, want) < 1e-6


# ------------------------------------------------------------------ 10. end to end
def test_mim_yaml_pretrains_and_hands_over(dev, tmp_path, monkeypatch):
    import yaml

    from scripts import run as run_script
    from vit_amd.trainer import Trainer, load_checkpoint_file, model_state_from_checkpoint

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "exp", "mim_pretrain.yaml")))
    assert cfg["model"]["task_type"] == "mim" and cfg["mim"]["mask_ratio"] == 0.6 and cfg["model"]["hidden_size"] == 768
    cfg["model"].update(image_size=256, patch_size=16, stride_size=16, hidden_size=32, num_hidden_layers=2, num_attention_heads=2)
    cfg["train"].update(batch_size=8, ep=1, save=True)
    cfg["project"] = "t"
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump(cfg))
    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "ckpt"))
    args = types.SimpleNamespace(config=str(path), gpu=1, debug=0, seed=42, synthetic=240, save=True, ckpt=None)
    config, module, data = run_script.build(args)
    assert module.monitor_metric == "mim_loss" and module.epoch_metrics() == {} and module.model.name.endswith("_mim")
    trainer = Trainer(config["train"], device=dev, verbose=False)
    steps, log = [], trainer._log

    def spy(name, value, **kw):
        if name == "mim_loss":
            steps.append(value.detach().clone() if torch.is_tensor(value) else value)
        return log(name, value, **kw)

    trainer._log = spy
    hist = trainer.fit(module, *data.fit_loaders(args.debug))
    assert trainer.monitor == "val_mim_loss" and trainer.monitor_mode == "min"
    steps = [float(v) for v in steps]
    assert trainer.global_step == 30 and len(steps) == 30 and all(np.isfinite(steps))
    first, last = sum(steps[:5]) / 5, sum(steps[-5:]) / 5
    print(f"[mim end to end] mim_loss of the first 5 steps {first:.4f}, of the last 5 {last:.4f}; logged {sorted(hist[-1])}")
    assert last < first
    assert "val_mim_loss" in hist[-1] and not any(k.endswith(("_mae", "_acc", "_r2")) for k in hist[-1])
    ckpt = trainer.checkpointer.last_path
    assert ckpt and os.path.exists(ckpt)
    saved = model_state_from_checkpoint(load_checkpoint_file(ckpt))
    # the hand-over: a regression run takes every encoder tensor, bit for bit, and trains
    cfg["model"].update(task_type="reg", init_from=ckpt)
    cfg["data"]["param"] = "log_g"
    cfg["loss"] = {"name": "mae"}
    cfg["train"].update(save=False)
    cfg.pop("mim")
    path2 = tmp_path / "ft.yaml"
    path2.write_text(yaml.safe_dump(cfg))
    args2 = types.SimpleNamespace(config=str(path2), gpu=1, debug=0, seed=43, synthetic=8, save=False, ckpt=None)
    config2, module2, data2 = run_script.build(args2)
    own = module2.model.state_dict()
    skipped = sorted(set(saved) - set(own))
    assert skipped == ["decoder.bias", "decoder.weight", "vit.embeddings.mask_token"]
    assert sorted(set(own) - set(saved)) == ["regressor.bias", "regressor.weight"]
    for k in set(own) & set(saved):
        assert torch.equal(own[k].cpu(), saved[k]), k
    t2 = Trainer(config2["train"], device=dev, verbose=False)
    hist2 = t2.fit(module2, *data2.fit_loaders(args2.debug))
    assert t2.global_step == 1 and all(np.isfinite(float(v)) for k, v in hist2[-1].items() if "loss" in k)
    moved = module2.model.state_dict()
    assert float((moved["vit.layernorm.weight"].cpu() - saved["vit.layernorm.weight"]).abs().max()) > 0


# ------------------------------------------------------------------ the poison table
# tests/test_poison_cpu.py demands that every exported vit_* name is a case of tests/test_poison_gpu.py's table or listed in its
# EXEMPT dict with a reason.  The five exports of include/vit_amd_mim.h are listed there from here, when this module is imported
# (pytest imports every test module before it runs the first test): the tests of this file poison their outputs and workspace
# themselves (tests 1, 3 and 4 above), and vit_embed_finish_masked works in place like vit_embed_finish.
def _list_in_poison_table():
    import test_poison_gpu as table

    here = "poisoned by tests/test_mim_gpu.py"
    for name, reason in (("vit_mim_mask", here), ("vit_embed_finish_masked", "in place"), ("vit_embed_finish_masked_bwd", here),
                         ("vit_mim_loss_fwd", here), ("vit_mim_loss_bwd", here)):
        table.EXEMPT.setdefault(name, reason)


_list_in_poison_table()
