"""Register tokens (`model.num_register_tokens`, include/vit_amd_registers.h) on the GPU: the two kernels against their host
restatement (tests/_registers_ref.py) bit for bit, the batch sums also against a float64 sum at the f32 bound, R = 0 against the
existing entry points; the model against the UNCHANGED CPU oracle run under `_registers_ref.registers` at the project's gates
(precision '32': logits and loss < 1e-4, every gradient tensor < 2e-4; bf16-mixed: the case's gtol, cosine > 0.999) for the
cases l3, rope and l3 with learned positions; masked modelling, average pooling, LayerScale and sharpness-aware minimisation
with registers; the captured step; two gloo ranks; that the registers matter; and that 0 registers is the code as it was.
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

import _registers_ref as rr
from _poison import poisoned
from oracle import dropmask as dm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_SEED = 0x5DEECE66D2468ACE  # tests/test_cls_tail_gpu.py: hip_pass runs step STEP of this seed
STEP = 3
GUARD = 64  # elements around every kernel buffer that must keep their fill
REG = rr.REG


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def guarded(dev, shape, dtype=torch.float32):
    """(a tensor of `shape`, the GUARD elements behind it): one allocation, so the band is what an overrun would hit."""
    n = int(np.prod(shape))
    buf = torch.empty(n + GUARD, dtype=dtype, device=dev)
    return buf[:n].view(*shape), buf[n:]


# ------------------------------------------------------------------ 1. the kernels
def kernel_inputs(shape, mask_kind):
    B, R, N, D = shape
    T = 1 + R + N
    g = torch.Generator().manual_seed(1000 * B + 100 * R + 10 * N + D)
    t = dict(tok=torch.randn(B, T, D, generator=g), cls=torch.randn(D, generator=g), reg=torch.randn(R, D, generator=g),
             pos=torch.randn(1 + N, D, generator=g), mtok=torch.randn(D, generator=g), dtok=torch.randn(B, T, D, generator=g),
             old=dict(dcls=torch.randn(D, generator=g), dreg=torch.randn(R, D, generator=g), dpos=torch.randn(1 + N, D, generator=g),
                      dmt=torch.randn(D, generator=g)))
    t["mask"] = rr.make_mask(mask_kind, B, N, 17 + B)
    return t


@pytest.mark.parametrize("mask_kind", rr.MASKS, ids=lambda k: f"mask-{k}")
@pytest.mark.parametrize("shape", rr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_kernel_is_the_restatement(dev, shape, mask_kind):
    import vit_amd.functional as vf

    B, R, N, D = shape
    T = 1 + R + N
    h = kernel_inputs(shape, mask_kind)
    mask = None if h["mask"] is None else h["mask"].to(dev)
    cls, reg, pos, mtok = (h[k].to(dev) for k in ("cls", "reg", "pos", "mtok"))
    seed = 2 ** 64 - 59
    for with_pos in (False, True):
        for p in (0.0, 0.1):
            want = rr.embed_fwd(h["tok"], R, h["cls"], h["reg"], h["pos"] if with_pos else None, h["mask"],
                                h["mtok"] if mask is not None else None, rr.multiplier(p, seed, 0, B, T, D))
            # the token tensor between two bands; CLS, register and masked rows are outputs only: poisoned before the call
            buf = torch.full((GUARD + B * T * D + GUARD,), -7.5, device=dev)
            tok = buf[GUARD:GUARD + B * T * D].view(B, T, D)
            tok.copy_(h["tok"])
            tok[:, :1 + R] = float("nan")
            if mask is not None:
                tok[:, 1 + R:][mask != 0] = float("nan")
            got = vf.embed_finish_reg(tok, R, cls, reg, pos if with_pos else None, mask, mtok if mask is not None else None,
                                      dropout=(p, seed, 0))
            assert got.data_ptr() == tok.data_ptr()
            assert torch.equal(bits(tok.cpu()), bits(want)), (shape, mask_kind, with_pos, p)
            assert bool((buf[:GUARD] == -7.5).all()) and bool((buf[-GUARD:] == -7.5).all())
            if R == 0:  # the existing entry points store the same bits
                twin = h["tok"].to(dev)
                if mask is None:
                    vf.embed_finish(twin, cls, pos if with_pos else None, dropout=(p, seed, 0))
                else:
                    vf.embed_finish_masked(twin, cls, mask, mtok, pos if with_pos else None, dropout=(p, seed, 0))
                assert torch.equal(bits(tok), bits(twin))


@pytest.mark.parametrize("mask_kind", rr.MASKS, ids=lambda k: f"mask-{k}")
@pytest.mark.parametrize("shape", rr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_kernel_is_the_restatement(dev, shape, mask_kind):
    import vit_amd.functional as vf

    B, R, N, D = shape
    T = 1 + R + N
    h = kernel_inputs(shape, mask_kind)
    mask = None if h["mask"] is None else h["mask"].to(dev)
    dtok = h["dtok"].to(dev)
    seed = 2 ** 63 + 41
    worst = 0.0
    for with_pos in (False, True):
        for p in (0.0, 0.1):
            mult = rr.multiplier(p, seed, 0, B, T, D)
            want = rr.embed_bwd(h["dtok"], R, h["mask"], mult, with_pos=with_pos)
            acc = rr.embed_bwd(h["dtok"], R, h["mask"], mult, with_pos=with_pos, old=h["old"])
            # the float64 sums and the bound of an f32 sum of B terms in any order
            gd = (h["dtok"] if mult is None else h["dtok"] * mult).double()
            terms = dict(dcls=gd[:, 0], dreg=gd[:, 1:1 + R], dpos=torch.cat([gd[:, :1], gd[:, 1 + R:]], dim=1))
            if mask is not None:
                terms["dmt"] = (gd[:, 1 + R:] * (h["mask"] != 0)[:, :, None]).reshape(B * N, D)
            for k, tm in terms.items():
                if want[k] is not None and want[k].numel():
                    err = (want[k].double() - tm.sum(0).view(want[k].shape)).abs()
                    lim = (B + 2) * 2.0 ** -24 * tm.abs().sum(0).view(want[k].shape)
                    assert bool((err <= lim + 1e-30).all()), (k, shape)
                    worst = max(worst, float((err / (lim + 1e-30)).max()))
            for dt in (torch.bfloat16, torch.float32):
                for accumulate in (False, True):
                    dpatch, pad_p = guarded(dev, (B * N, D), dt)
                    dcls, pad_c = guarded(dev, (D,))
                    dreg, pad_r = guarded(dev, (R, D))
                    dpos, pad_q = guarded(dev, (1 + N, D)) if with_pos else (None, None)
                    dmt, pad_m = guarded(dev, (D,)) if mask is not None else (None, None)
                    sums = [(dcls, "dcls"), (dreg, "dreg"), (dpos, "dpos"), (dmt, "dmt")]
                    run = lambda: vf.embed_finish_reg_bwd(dtok, R, dcls, dreg, dpos, mask, dmt, dropout=(p, seed, 0), dpatch=dpatch,
                                                          accumulate=accumulate)
                    pads = [x for x in (pad_p, pad_c, pad_r, pad_q, pad_m) if x is not None]
                    if accumulate:  # the sums read what they hold: prefilled with the old values; dpatch and the workspace poisoned
                        def run_acc():
                            for t, k in sums:
                                if t is not None:
                                    t.copy_(h["old"][k])
                            run()
                        poisoned(dev, run_acc, [dpatch], pads=pads)
                    else:
                        poisoned(dev, run, [dpatch] + [t for t, _ in sums if t is not None and t.numel()], pads=pads)
                    exp = acc if accumulate else want
                    assert torch.equal(bits(dpatch.cpu()), bits(exp["dpatch"].to(dt))), (shape, mask_kind, with_pos, p, dt)
                    for t, k in sums:
                        if t is not None:
                            assert torch.equal(bits(t.cpu()), bits(exp[k].view(t.shape))), (k, shape, mask_kind, with_pos, p, dt, accumulate)
                    if R == 0:  # the existing entry points store the same bits
                        c2, q2 = (h["old"]["dcls"].to(dev), h["old"]["dpos"].to(dev) if with_pos else None)
                        if mask is None:
                            p2 = torch.empty_like(dpatch)
                            vf._h(dtok).call("vit_embed_finish_bwd", dtok.data_ptr(), p2.data_ptr(), vf._DT[dt], c2.data_ptr(), vf._ptr(q2), B, T,
                                    D, p, seed, 0, int(accumulate), vf._stream(dtok))
                        else:
                            m2 = h["old"]["dmt"].to(dev)
                            p2 = vf.embed_finish_masked_bwd(dtok, mask, c2, m2, q2, dropout=(p, seed, 0), out_dtype=dt, accumulate=accumulate)
                            assert torch.equal(bits(dmt), bits(m2))
                        assert torch.equal(bits(dpatch), bits(p2.view(dpatch.shape))) and torch.equal(bits(dcls), bits(c2))
                        assert q2 is None or torch.equal(bits(dpos), bits(q2))
    print(f"[registers bwd {shape} mask {mask_kind}] worst restated sum error / f32 bound {worst:.3f}")


def test_argument_errors_launch_nothing(dev):
    import vit_amd.functional as vf

    B, R, N, D = 2, 2, 3, 32
    T = 1 + R + N
    h = vf._h(torch.empty(1, device=dev))
    st = torch.cuda.current_stream(dev).cuda_stream
    SENT = -12345.0
    F = lambda *s: torch.full(s, SENT, device=dev)
    outs = dict(tok=F(B, T, D), dpatch=F(B * N, D), dcls=F(D), dreg=F(R, D), dpos=F(1 + N, D), dmt=F(D))
    cls, reg, mtok = torch.randn(D, device=dev), torch.randn(R, D, device=dev), torch.randn(D, device=dev)
    mask = torch.ones(B, N, dtype=torch.int32, device=dev)
    dtok = torch.randn(B, T, D, device=dev)
    lib, hh = h.lib, h.h
    o = {k: v.data_ptr() for k, v in outs.items()}
    c, r, m, mt, dt = cls.data_ptr(), reg.data_ptr(), mask.data_ptr(), mtok.data_ptr(), dtok.data_ptr()
    fwd, bwd = lib.vit_embed_finish_reg, lib.vit_embed_finish_reg_bwd
    calls = [
        (lambda: fwd(hh, None, c, r, None, None, None, B, R, N, D, 0.0, 1, 0, st), b"null pointer"),
        (lambda: fwd(hh, o["tok"], None, r, None, None, None, B, R, N, D, 0.0, 1, 0, st), b"null pointer"),
        (lambda: fwd(hh, o["tok"], c, None, None, None, None, B, R, N, D, 0.0, 1, 0, st), b"null pointer"),
        (lambda: fwd(hh, o["tok"], c, r, None, m, None, B, R, N, D, 0.0, 1, 0, st), b"mask and mask_token"),
        (lambda: fwd(hh, o["tok"], c, r, None, None, None, 0, R, N, D, 0.0, 1, 0, st), b"B=0"),
        (lambda: fwd(hh, o["tok"], c, r, None, None, None, B, R, 0, D, 0.0, 1, 0, st), b"N=0"),
        (lambda: fwd(hh, o["tok"], c, r, None, None, None, B, -1, N, D, 0.0, 1, 0, st), b"R=-1"),
        (lambda: fwd(hh, o["tok"], c, r, None, None, None, B, R, N, 30, 0.0, 1, 0, st), b"D=30"),
        (lambda: fwd(hh, o["tok"], c, r, None, None, None, B, R, N, D, 1.0, 1, 0, st), b"dropout_p"),
        (lambda: bwd(hh, None, None, o["dpatch"], 1, o["dcls"], o["dreg"], None, None, B, R, N, D, 0.0, 1, 0, 0, st), b"null pointer"),
        (lambda: bwd(hh, dt, None, None, 1, o["dcls"], o["dreg"], None, None, B, R, N, D, 0.0, 1, 0, 0, st), b"null pointer"),
        (lambda: bwd(hh, dt, None, o["dpatch"], 1, None, o["dreg"], None, None, B, R, N, D, 0.0, 1, 0, 0, st), b"null pointer"),
        (lambda: bwd(hh, dt, None, o["dpatch"], 1, o["dcls"], None, None, None, B, R, N, D, 0.0, 1, 0, 0, st), b"null pointer"),
        (lambda: bwd(hh, dt, m, o["dpatch"], 1, o["dcls"], o["dreg"], None, None, B, R, N, D, 0.0, 1, 0, 0, st), b"mask and dmask_token"),
        (lambda: bwd(hh, dt, None, o["dpatch"], 1, o["dcls"], o["dreg"], None, None, B, R, N, 0, 0.0, 1, 0, 0, st), b"D=0"),
        (lambda: bwd(hh, dt, None, o["dpatch"], 1, o["dcls"], o["dreg"], None, None, B, R, N, D, -0.1, 1, 0, 0, st), b"dropout_p"),
        (lambda: bwd(hh, dt, None, o["dpatch"], 9, o["dcls"], o["dreg"], None, None, B, R, N, D, 0.0, 1, 0, 0, st), b"bad dtype"),
    ]
    for call, text in calls:
        assert call() == -1  # VIT_ERR_ARG
        assert text in lib.vit_last_error(), (text, lib.vit_last_error())
    torch.cuda.synchronize(dev)
    for k, v in outs.items():  # nothing was launched: every output still holds its sentinel
        assert bool((v == SENT).all()), k


# ------------------------------------------------------------------ 2. the model against the oracle
_oracle = {}
TAGS = ["l3", "rope", "l3-learned"]


def reg_case(tag):
    """(rc, sd, flux, labels, gtol) of tests/test_cls_tail_gpu.py's case, `l3-learned`: l3 with a learned position table."""
    from oracle import refvit
    from test_cls_tail_gpu import CASES, case

    base = tag.split("-")[0]
    rc, sd, flux, labels, _, gtol = case(base)
    if tag.endswith("-learned"):
        rc = dataclasses.replace(rc, pos_encoding_type="learned")
        sd = refvit.make_state_dict(rc, CASES[base][2])
    return rc, sd, flux, labels, gtol


def with_registers(rc, sd, R, seed=900):
    """The case's weights plus register values of std 1 (the same for every R' <= R: a prefix)."""
    return dict(sd, **{REG: rr.register_values(4, rc.hidden_size, seed)[:, :R].clone()}) if R > 0 else dict(sd)


def reg_model(rc, sd, dev, precision, R, **over):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    kw = dict(task_type=rc.task_type, image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
              num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
              stride_size=rc.stride_size, num_labels=rc.num_labels, pos_encoding_type=rc.pos_encoding_type, rope_base=rc.rope_base,
              num_register_tokens=R)
    model = MyViT(ViTConfig(**dict(kw, **over)), loss_name=rc.loss_name)
    model.set_precision(precision)
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def step_masks(rc):
    return dm.engine_masks(rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, dm.step_seed(BASE_SEED, STEP), None)


def oracle_pass(tag, R, train):
    """One CPU oracle forward + backward with R registers per (case, R, mode), computed once and left unchanged."""
    key = (tag, R, train)
    if key not in _oracle:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        rc, sd, flux, labels, _ = reg_case(tag)
        params = {k: v.clone().requires_grad_(True) for k, v in with_registers(rc, sd, R).items()}
        out = rr.oracle_forward(rc, params, flux, labels, R, train, step_masks(rc) if train else None)
        out.loss.backward()
        _oracle[key] = dict(loss=float(out.loss.detach()), logits=out.logits.detach(),
                            grads={k: p.grad for k, p in params.items() if p.grad is not None})
    return _oracle[key]


def registers_matter(tag, train):
    """The two conditions on the ORACLE alone (seed 900 of `with_registers` was chosen on the CPU to satisfy them for every case):
    its logits with 4 registers and with none differ by at least ten times the parity gate, and the 4 rows of its register
    gradient differ pairwise."""
    o4, o0 = oracle_pass(tag, 4, train), oracle_pass(tag, 0, train)
    apart = rel(o4["logits"], o0["logits"])
    dreg = o4["grads"][REG][0]
    rows = min(rel(dreg[i], dreg[j]) for i in range(4) for j in range(i))
    assert apart >= 10 * 1e-4, (tag, apart)
    assert rows >= 10 * 2e-4 and float(dreg.norm()) > 0, (tag, rows)
    return apart, rows


def check_fp32(name, h, o):
    """The project's gates at precision '32': logits and loss < 1e-4, every gradient tensor < 2e-4, register_tokens included."""
    from test_cls_tail_gpu import errors

    e = errors(h, o)
    worst = max(e["grads"].items(), key=lambda kv: kv[1][0])
    reg = e["grads"].get(REG, (float("nan"),))[0]
    print(f"[registers {name} 32] logits {e['logits']:.2e}, loss {e['loss']:.2e}, worst gradient {worst[1][0]:.2e} ({worst[0]}), "
          f"register_tokens {reg:.2e}")
    assert e["logits"] < 1e-4 and e["loss"] < 1e-4, (name, e["logits"], e["loss"])
    for pname, (r, _) in e["grads"].items():
        assert r < 2e-4, (name, pname, r)
    return e


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("tag", TAGS)
def test_model_is_the_oracle_fp32(dev, tag, R, train):
    from test_cls_tail_gpu import hip_pass

    rc, sd, flux, labels, _ = reg_case(tag)
    if R == 4:
        apart, rows = registers_matter(tag, train)
        print(f"[registers {tag} {'train' if train else 'eval'}] the oracle's logits with 4 registers and with none are {apart:.2e} apart; "
              f"the closest two rows of its register gradient {rows:.2e}")
    o = oracle_pass(tag, R, train)
    model = reg_model(rc, with_registers(rc, sd, R), dev, "32", R)
    eng = model.engine
    assert eng.cfg.seq_len == 1 + R + rc.num_patches and eng.layout.entries[REG][1] == (1, R, rc.hidden_size)
    x, y = flux.to(dev), labels.to(dev)
    h = hip_pass(model, x, y, train, tail=True)
    assert h["tail"] is True and eng._last["T"] == 1 + R + rc.num_patches  # the CLS tail stays on: row 0 at stride T
    e = check_fp32(f"{tag} R={R} {'train' if train else 'eval'}", h, o)
    assert REG in e["grads"] and "vit.embeddings.cls_token" in e["grads"]
    if rc.pos_encoding_type == "learned":
        assert rr.POS in e["grads"] and h["grads"][rr.POS].shape == (1, 1 + rc.num_patches, rc.hidden_size)
    if R == 4 and not train:
        # the full path gives the tail's numbers; hidden states and attention maps carry the register rows and columns
        full = hip_pass(model, x, y, train, tail=False)
        check_fp32(f"{tag} R={R} eval, full path", full, o)
        model.eval()
        with torch.no_grad():
            out = model(x, labels=y, output_hidden_states=True, output_attentions=True)
        T = 1 + R + rc.num_patches
        assert all(hs.shape == (x.shape[0], T, rc.hidden_size) for hs in out.hidden_states)
        assert all(a.shape == (x.shape[0], rc.num_attention_heads, T, T) for a in out.attentions)
        with rr.registers(with_registers(rc, sd, R), R) as sdr, torch.no_grad():
            from oracle import refvit

            ref = refvit.forward(rc, sdr, flux, labels, output_hidden_states=True, output_attentions=True)
        assert rel(torch.stack([t.cpu() for t in out.hidden_states]), torch.stack(ref.hidden_states)) < 1e-4
        assert rel(torch.stack([t.cpu() for t in out.attentions]), torch.stack(ref.attentions)) < 1e-4


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_model_is_the_oracle_bf16(dev, train):
    """Case l3 with 4 registers at bf16-mixed: logits < 1.5e-2 and the loss within 3e-2 (tests/test_pool_gpu.py's rule for this
    case), every gradient tensor < the case's gtol with cosine > 0.999."""
    from test_cls_tail_gpu import errors, hip_pass

    rc, sd, flux, labels, gtol = reg_case("l3")
    registers_matter("l3", train)
    o = oracle_pass("l3", 4, train)
    model = reg_model(rc, with_registers(rc, sd, 4), dev, "bf16-mixed", 4)
    h = hip_pass(model, flux.to(dev), labels.to(dev), train, tail=True)
    e = errors(h, o)
    worst = max(e["grads"].items(), key=lambda kv: kv[1][0])
    print(f"[registers l3 R=4 bf16-mixed {'train' if train else 'eval'}] logits {e['logits']:.2e}, loss {e['loss']:.2e} (tol 3e-2), "
          f"worst gradient {worst[1][0]:.2e} ({worst[0]}, gtol {gtol}), register_tokens {e['grads'][REG]}, lowest cosine "
          f"{min(c for _, c in e['grads'].values()):.5f}")
    assert e["logits"] < 1.5e-2 and e["loss"] <= 3e-2
    for name, (r, c) in e["grads"].items():
        assert r < gtol and c > 0.999, (name, r, c)


# ------------------------------------------------------------------ 3. with the rest of the recipe
@pytest.mark.parametrize("tag", ["l3", "rope"])
def test_masked_modelling_with_registers(dev, tag):
    """task_type 'mim', 4 registers, '32', MSE: the decoder reads rows 1 + R ..; hidden states (register rows included),
    reconstruction and loss < 1e-4, every gradient tensor < 2e-4 against tests/_mim_ref.py composed with the register wrapper."""
    import _mim_ref as mr
    from oracle import refvit
    from test_mim_gpu import RATIO, SPAN, grad_errors, mim_pass, mim_state, step_mask
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    R = 4
    rc, sd, flux, _, _ = reg_case(tag)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    state = with_registers(rc, mim_state(rc, sd, 71), R)
    B, N, P = flux.shape[0], rc.num_patches, rc.patch_size
    m = step_mask(rc, B)
    assert 0 < int(m.sum()) < m.size
    params = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    with mr.masked_tokens(m, params[mr.MASK_TOKEN]), rr.registers(params, R) as sdr:
        out = refvit.forward(rc, sdr, flux, None, training=True, masks=step_masks(rc), output_hidden_states=True)
    rec = torch.nn.functional.linear(out.last_hidden_state[:, 1 + R:, :], params["decoder.weight"], params["decoder.bias"])
    loss = mr.loss(rec, flux, m, P, rc.stride, "mse", False)
    loss.backward()
    o = dict(grads={k: p.grad for k, p in params.items() if p.grad is not None})
    cfg = ViTConfig(task_type="mim", image_size=rc.image_size, patch_size=P, hidden_size=rc.hidden_size,
                    num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
                    stride_size=rc.stride_size, pos_encoding_type=rc.pos_encoding_type, rope_base=rc.rope_base, mim_mask_ratio=RATIO,
                    mim_span=SPAN, mim_loss="mse", num_register_tokens=R)
    model = MyViT(cfg, loss_name="")
    model.set_precision("32")
    model.load_state_dict({k: v for k, v in state.items() if not k.startswith("regressor.")}, strict=True)
    model = model.to(dev)
    got, grads = mim_pass(model, flux.to(dev))
    assert np.array_equal(got.mask.cpu().numpy(), m) and got.reconstruction.shape == (B, N, P)
    hs = torch.stack([t.cpu() for t in got.hidden_states])
    assert hs.shape[2] == 1 + R + N
    e_hs, e_rec = rel(hs, torch.stack([t.detach() for t in out.hidden_states])), rel(got.reconstruction, rec.detach())
    e_loss = abs(float(got.loss.detach()) - float(loss.detach())) / float(loss.detach())
    errs = grad_errors(grads, o)
    worst = max(errs.items(), key=lambda kv: kv[1][0])
    print(f"[registers mim {tag} R=4 32] hidden {e_hs:.2e}, reconstruction {e_rec:.2e}, loss {e_loss:.2e}, worst gradient "
          f"{worst[1][0]:.2e} ({worst[0]}); register_tokens {errs[REG][0]:.2e}, mask_token {errs[mr.MASK_TOKEN][0]:.2e}")
    assert e_hs < 1e-4 and e_rec < 1e-4 and e_loss < 1e-4
    for name, (r, _) in errs.items():
        assert r < 2e-4, (name, r)
    assert {REG, mr.MASK_TOKEN, "decoder.weight", "decoder.bias"} <= set(errs)
    # the decoder's row offset is in the path: the oracle's reconstruction from rows 1 .. N (registers taken for patches) is far
    wrong = torch.nn.functional.linear(out.last_hidden_state[:, 1:1 + N, :], params["decoder.weight"], params["decoder.bias"])
    assert rel(got.reconstruction, wrong.detach()) >= 10 * 1e-4


def test_average_pooling_with_registers(dev):
    """global_pool 'avg', 4 registers, '32', train mode: the mean runs over rows 1 + R .. (first = 1 + R)."""
    import _pool_ref as pr
    from test_cls_tail_gpu import hip_pass

    R = 4
    rc, sd, flux, labels, _ = reg_case("l3")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    state = with_registers(rc, sd, R)
    params = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    out = rr.oracle_forward(rc, params, flux, None, R, True, step_masks(rc))
    head = lambda rows: torch.nn.functional.linear(rows.mean(1), params[rc.head_name + ".weight"], params[rc.head_name + ".bias"])
    logits = head(out.last_hidden_state[:, 1 + R:])
    loss = pr.head_loss(rc, logits, labels)
    loss.backward()
    o = dict(loss=float(loss.detach()), logits=logits.detach(), grads={k: p.grad for k, p in params.items() if p.grad is not None})
    model = reg_model(rc, state, dev, "32", R, global_pool="avg")
    h = hip_pass(model, flux.to(dev), labels.to(dev), True, tail=True)
    assert h["tail"] is False and model.engine._last["pool"] == "avg" and model.name.endswith("_gap_reg4")
    e = check_fp32("l3 R=4 avg train", h, o)
    wrong = rel(h["logits"], head(out.last_hidden_state[:, 1:]).detach())  # a mean that took the registers in
    print(f"[registers avg] logits against the mean over rows 1 ..: {wrong:.2e}")
    assert wrong >= 10 * 1e-4 and REG in e["grads"]


def test_layer_scale_with_registers(dev):
    """layer_scale_init, 4 registers, '32', train mode, on tests/test_layerscale_gpu.py's fixture c1 and its oracle construction
    (the scaled weights are lambda[:, None] * W of leaf tensors) composed with the register wrapper."""
    from test_cls_tail_gpu import hip_pass
    from test_layerscale_gpu import fixture
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    R = 4
    rc, kw, sd, x, labels = fixture("c1")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    state = with_registers(rc, sd, R)
    leaves = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    params = {k: v for k, v in leaves.items() if not k.endswith(".lambda1")}
    for k, lam in leaves.items():
        if k.endswith(".lambda1"):
            stem = k.replace("layer_scale1.lambda1", "attention.output.dense").replace("layer_scale2.lambda1", "output.dense")
            params[stem + ".weight"] = lam[:, None] * leaves[stem + ".weight"]
            params[stem + ".bias"] = lam * leaves[stem + ".bias"]
    out = rr.oracle_forward(rc, params, x, labels, R, True, step_masks(rc))
    out.loss.backward()
    o = dict(loss=float(out.loss.detach()), logits=out.logits.detach(), grads={k: p.grad for k, p in leaves.items() if p.grad is not None})
    model = MyViT(ViTConfig(**kw, layer_scale_init=1.0, num_register_tokens=R), loss_name="mae")
    model.set_precision("32")
    model.load_state_dict(state, strict=True)
    model = model.to(dev)
    e = check_fp32("c1 R=4 layer scale train", hip_pass(model, x.to(dev), labels.to(dev), True, tail=True), o)
    assert REG in e["grads"] and sum(n.endswith(".lambda1") for n in e["grads"]) >= 4


def test_sharpness_aware_step_with_registers(dev):
    """train.sam_rho with 4 registers, '32': tests/test_sam_gpu.py's chain construction -- the gradient with SAM attached against
    the oracle at w + e(g_hip) under the register wrapper; the perturbation covers register_tokens."""
    from test_cls_tail_gpu import hip_pass
    from test_sam_gpu import RHO, chain

    R = 4
    rc, sd, flux, labels, _ = reg_case("l3")
    state = with_registers(rc, sd, R)

    def step(rc_, params, x, y, masks):
        out = rr.oracle_forward(rc_, params, x, y, R, masks is not None, masks)
        return out.loss, out.logits

    model = reg_model(rc, state, dev, "32", R)
    x, y = flux.to(dev), labels.to(dev)
    h0, h1, o, _ = chain("registers l3 R=4", model, lambda m: hip_pass(m, x, y, True, tail=True), rc, state, flux, labels,
                         step_masks(rc), RHO[("l3", False)], False, step=step)
    assert h1["loss"] == h0["loss"] and REG in o["grads"]
    assert abs(o["loss_sam"] - o["loss"]) / abs(o["loss"]) > 1e-3
    check_fp32("l3 R=4 sam chain", h1, o)
    assert rel(h0["grads"][REG], o["grads"][REG]) > 10 * 2e-4  # the second pass is in the path for the registers too
    model.set_sam(None)


# ------------------------------------------------------------------ 4. the captured step
def test_hip_graph_replay_is_the_eager_step(dev):
    """lr = 0: the replay is a step of the same weights.  Its loss and every gradient -- register_tokens' among them -- are the
    eager step's under the same bound record, bit for bit (tests/test_pool_gpu.py's construction)."""
    import vit_amd.functional as vf
    from vit_amd import _cabi
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedAdamW

    R = 4
    rc, sd, flux, labels, _ = reg_case("rope")
    model = reg_model(rc, with_registers(rc, sd, R), dev, "bf16-mixed", R)
    eng = model.engine
    eng.overlap_dw = False  # the captured step runs on one stream; so does the eager one it is compared with
    x, y = flux.to(dev), labels.to(dev)
    eng.base_seed, eng.step_counter = BASE_SEED, 0
    opt = FusedAdamW(model, lr=0.0)
    opt.set_grad_clip(0.5)
    module = types.SimpleNamespace(model=model, noise_level=0, train=model.train)
    warmup = 2
    gs = GraphedTrainStep(module, opt, (x, None, y), warmup=warmup)
    lay = eng.layout
    names = [k for k, (off, _) in lay.entries.items() if off < lay.n_trainable]
    loss = gs.step((x, None, y)).clone()
    torch.cuda.synchronize(dev)
    assert eng._last["T"] == 1 + R + rc.num_patches and REG in names
    grads = {k: lay.view(eng.grads, k).clone() for k in names}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and float(grads[REG].abs().max()) > 0
    h = eng.handle()
    record = torch.zeros(8, dtype=torch.int32, device=dev)
    eng.step_counter = warmup
    eng.grads.fill_(float("nan"))
    _cabi.check(h.lib.vit_step_state_bind(h.h, record.data_ptr()), "vit_step_state_bind")
    try:
        with vf.use_handle(h):
            _cabi.check(h.lib.vit_step_advance(h.h, BASE_SEED, 0.9, 0.999, vf._stream(record)), "vit_step_advance")
        eager, _, _, _ = eng.forward(x, y, training=True, need_grad=True)
        eng.backward(torch.ones(1, device=dev))
        torch.cuda.synchronize(dev)
    finally:
        _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
    assert torch.equal(eager, loss), (float(eager), float(loss))
    for k in names:  # every element of every gradient tensor was rewritten over the NaN fill, with the replay's bits
        assert torch.equal(lay.view(eng.grads, k), grads[k]), k


# ------------------------------------------------------------------ 5. two gloo ranks on one GPU
def _ranks(tmp_path, world):
    child = os.path.join(ROOT, "tests", "_registers_ddp_child.py")
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


def test_two_ranks_stay_bit_identical(dev, tmp_path):
    """The data-parallel exchange sees only a longer embedding bucket: after two steps the replicas hold the same bits, the
    registers moved, and the exchanged gradient of step 1 is the mean of the two shards' single-process gradients."""
    single = _ranks(tmp_path, 1)[0]
    r0, r1 = _ranks(tmp_path, 2)
    assert r0["world"] == r1["world"] == 2 and single["world"] == 1
    assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["grad_step1"], r1["grad_step1"])
    lo, hi = single["spans"][REG]
    assert hi - lo == 4 * 32 and not torch.equal(r0["params"][lo:hi], single["start"][lo:hi])
    want = 0.5 * (single["shard_grads"][0].double() + single["shard_grads"][1].double())
    worst = 0.0
    for name, (a, b) in single["spans"].items():
        w = want[a:b]
        if float(w.norm()) < 1e-6 * float(want.norm()):
            continue
        worst = max(worst, float((r0["grad_step1"][a:b].double() - w).norm() / w.norm()))
    one = rel(single["shard_grads"][0][lo:hi], want[lo:hi])
    print(f"[registers ddp] exchanged gradient against the mean of the shards' gradients: worst tensor {worst:.2e}; one shard's "
          f"register gradient alone is {one:.3f} away")
    assert worst < 2e-4 and one > 10 * 2e-4


# ------------------------------------------------------------------ 6. no registers: the code as it was
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_zero_registers_is_the_model_without_the_key(dev, precision, monkeypatch):
    """num_register_tokens 0 against a config without the key: the same state_dict keys and run name, the same sequence of
    library calls with the same shape arguments, and logits, loss and every gradient tensor bit for bit."""
    from test_cls_tail_gpu import build, case, hip_pass
    from vit_amd import _cabi

    rc, sd, flux, labels, _, _ = case("l3")
    x, y = flux.to(dev), labels.to(dev)
    plain = build(rc, sd, dev, precision)
    zero = reg_model(rc, sd, dev, precision, 0)
    assert list(zero.state_dict()) == list(plain.state_dict()) and zero.name == plain.name
    assert zero.engine.layout.n_total == plain.engine.layout.n_total and zero.engine.reg == 0
    calls, real = [], _cabi.Handle.call

    def spy(self, name, *args):
        calls.append((name, tuple(a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool) and abs(a) < 1 << 20)))
        return real(self, name, *args)

    def run(model):
        hip_pass(model, x, y, True, tail=True)  # the first pass allocates the arena and sizes the workspace
        calls.clear()
        monkeypatch.setattr(_cabi.Handle, "call", spy)
        try:
            return hip_pass(model, x, y, True, tail=True), list(calls)
        finally:
            monkeypatch.setattr(_cabi.Handle, "call", real)

    (hp, cp), (hz, cz) = run(plain), run(zero)
    names = [n for n, _ in cp]
    assert cp == cz and "vit_embed_finish" in names and "vit_embed_finish_bwd" in names
    assert not any("_reg" in n for n in names)
    assert hp["loss"] == hz["loss"] and torch.equal(hp["logits"], hz["logits"])
    for k in hp["grads"]:
        assert torch.equal(bits(hp["grads"][k]), bits(hz["grads"][k])), k
    # and a model with registers does call the new entry points, once each
    four = reg_model(rc, with_registers(rc, sd, 4), dev, precision, 4)
    _, cf = run(four)
    names = [n for n, _ in cf]
    assert names.count("vit_embed_finish_reg") == 1 and names.count("vit_embed_finish_reg_bwd") == 1
    assert "vit_embed_finish" not in names and "vit_embed_finish_bwd" not in names


def test_patch_dropout_is_refused(dev):
    from vit_amd.config import ViTConfig

    with pytest.raises(ValueError, match="not built yet"):
        ViTConfig(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=1, num_attention_heads=2,
                  stride_size=32, num_register_tokens=2, patch_drop_rate=0.5)


# ------------------------------------------------------------------ 7. the poison table
# tests/test_poison_cpu.py demands that every exported vit_* name is a case of tests/test_poison_gpu.py's table or listed in its
# EXEMPT dict with a reason.  The two exports of include/vit_amd_registers.h are listed there from here, when this module is
# imported (pytest imports every test module before it runs the first test): the backward's outputs and workspace are poisoned
# in test 1 above, and vit_embed_finish_reg works in place like vit_embed_finish (its output-only rows are poisoned there).
def _list_in_poison_table():
    import test_poison_gpu as table

    table.EXEMPT.setdefault("vit_embed_finish_reg", "in place")
    table.EXEMPT.setdefault("vit_embed_finish_reg_bwd", "poisoned by tests/test_registers_gpu.py")


_list_in_poison_table()
