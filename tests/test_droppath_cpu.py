"""Stochastic depth (`model.drop_path_rate`, include/vit_amd_droppath.h), the part that needs no GPU: the host restatement of
the per-sample gate and its statistics, the schedule, the config plumbing, the oracle identity the GPU parity tests rest on,
and the C ABI's argument checks.

The restatement (three lines, `path_multiplier`): (thr, scale, k0, k1) = drop_cfg(p, seed, site) with the bound record's keys
XORed in when thr != 0; r16 = drop_hash(k0, k1, 2 * b + branch) & 0xFFFF; multiplier = scale where r16 >= thr, else 0.
tests/test_droppath_gpu.py imports it from here."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dropmask as dm

SEED = 12345


def path_multiplier(p, seed, site, B, keys_xor=None):
    """float32 [B, 2]: the multiplier of sample b's attention branch [:, 0] and MLP branch [:, 1] (1 everywhere at p = 0)."""
    thr, scale, k0, k1 = dm.drop_cfg(p, seed, site)
    if thr and keys_xor is not None:
        k0, k1 = k0 ^ (keys_xor[0] & dm.M32), k1 ^ (keys_xor[1] & dm.M32)
    r16 = dm.drop_hash(k0, k1, np.arange(2 * B, dtype=np.uint64)) & np.uint64(0xFFFF)
    return np.where(r16 >= thr, np.float32(scale), np.float32(0.0)).astype(np.float32).reshape(B, 2)


def path_rates(rate, L):
    return [float(v) for v in torch.linspace(0, rate, L).tolist()]


def path_masks(rate, L, p_hidden, p_attn, seed, keys_xor=None, swap=False):
    """`masks` for oracle.refvit.forward: the engine's dropout masks, those of the two projection sites of layer i multiplied
    (in float32) by the path multiplier of site 4 + 4 i.  swap=True exchanges the two branches' gates (a negative control)."""
    base = dm.engine_masks(p_hidden, p_attn, seed, keys_xor)
    rates = path_rates(rate, L)

    def masks(site, shape):
        m = base(site, shape)
        i, which = (site - 1) // 4, (site - 1) % 4
        if site == 0 or len(shape) == 4 or which not in (1, 2):
            return m
        pm = path_multiplier(rates[i], seed, dm.site_of(i, 3), shape[0], keys_xor)[:, (which - 1) ^ int(swap)]
        return m * torch.from_numpy(pm).view(-1, 1, 1)

    return masks


# ------------------------------------------------------------------ restatement statistics
@pytest.mark.parametrize("p", [0.05, 0.1, 0.25, 0.5])
def test_restated_gate_is_unbiased_and_branches_are_independent(p):
    n = 1 << 20
    site = dm.site_of(7, 3)
    assert site == 4 + 4 * 7
    thr, scale, _, _ = dm.drop_cfg(p, SEED, site)
    m = path_multiplier(p, SEED, site, n)
    keep = m != 0
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(scale))}
    q = 1 - thr / 65536
    sigma = math.sqrt(q * (1 - q) / n)
    for br in (0, 1):
        assert abs(keep[:, br].mean() - q) <= 4 * sigma, (p, br, keep[:, br].mean(), q, sigma)
    corr = np.corrcoef(keep[:, 0].astype(np.float64), keep[:, 1].astype(np.float64))[0, 1]
    assert abs(corr) < 0.01, (p, corr)
    assert abs(float(np.float64(scale) * q) - 1.0) < 1e-6  # kept values scaled so the gate is exactly unbiased


def test_schedule_and_exact_half():
    from vit_amd.config import ViTConfig
    from vit_amd.engine import ViTEngine

    for L in (1, 2, 3, 12):
        for r in (0.1, 0.5):
            cfg = ViTConfig(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=L,
                            num_attention_heads=2, stride_size=32, drop_path_rate=r)
            eng = ViTEngine(cfg, "mae")
            want = torch.linspace(0, r, L)
            got = eng.path_rates(True)
            assert got == [v.item() for v in want] and got[0] == 0.0
            assert eng.path_rates(False) is None
            assert eng._path(got, 0, 0) is None  # layer 0 never drops: the plain calls
            if L > 1:
                assert eng._path(got, L - 1, 1) == (got[-1], 4 + 4 * (L - 1), cfg.seq_len, 1)
            cfg.drop_path_rate = 0.0  # read on every forward
            assert eng.path_rates(True) is None
    assert dm.drop_cfg(0.5, SEED, 4)[:2] == (32768, 2.0)


def test_config_carries_the_rate_and_construction_checks_it():
    from vit_amd.config import ViTConfig, get_vit_config
    from vit_amd.specvit import MyViT

    model = dict(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2,
                 stride_size=32, proj_fn="SW")
    assert get_vit_config(dict(model=dict(model))).drop_path_rate == 0.0
    assert get_vit_config(dict(model=dict(model, drop_path_rate=0.2))).drop_path_rate == 0.2
    kw = dict(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2,
              stride_size=32)
    assert ViTConfig(**kw).drop_path_rate == 0.0
    plain, with_rate = MyViT(ViTConfig(**kw), loss_name="mae"), MyViT(ViTConfig(**kw, drop_path_rate=0.3), loss_name="mae")
    assert plain.name == with_rate.name
    assert list(plain.state_dict()) == list(with_rate.state_dict())  # no new parameter, no new buffer
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="drop_path_rate"):
            MyViT(ViTConfig(**kw, drop_path_rate=bad), loss_name="mae")


# ------------------------------------------------------------------ oracle identity
def test_oracle_with_path_masks_is_the_gated_forward():
    """oracle.refvit.forward with masks = engine masks x path multiplier at the two projection sites of each layer computes
    x + m * dropout(branch): checked against a forward written out here on a 2-layer toy configuration."""
    from oracle import refvit

    rc = refvit.RefConfig(image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2,
                          stride_size=32, loss_name="mae")
    sd = refvit.make_state_dict(rc, 5)
    B, rate, seed = 16, 0.5, dm.step_seed(0x5DEECE66D2468ACE, 3)
    flux, _, labels = refvit.make_inputs(rc, B, 6)
    out = refvit.forward(rc, sd, flux, labels, training=True, output_hidden_states=True,
                         masks=path_masks(rate, 2, 0.1, 0.1, seed))
    plain = refvit.forward(rc, sd, flux, labels, training=True, output_hidden_states=True,
                           masks=dm.engine_masks(0.1, 0.1, seed))
    em = dm.engine_masks(0.1, 0.1, seed)
    D, H, dh, T = rc.hidden_size, rc.num_attention_heads, rc.head_dim, rc.seq_len
    h = torch.cat((sd["vit.embeddings.cls_token"].expand(B, -1, -1), refvit.tokenize(rc, sd, flux)), dim=1)
    h = h * em(0, (B, T, D))
    rates = path_rates(rate, 2)
    assert rates == [0.0, 0.5]
    for i in range(2):
        pre = f"vit.encoder.layer.{i}."
        lin = lambda t, n: F.linear(t, sd[pre + n + ".weight"], sd[pre + n + ".bias"])
        ln = lambda t, n: F.layer_norm(t, (D,), sd[pre + n + ".weight"], sd[pre + n + ".bias"], rc.layer_norm_eps)
        m = torch.from_numpy(path_multiplier(rates[i], seed, 4 + 4 * i, B))  # [B, 2]
        if i == 1:
            assert 0 < int((m[:, 0] == 0).sum()) < B and 0 < int((m[:, 1] == 0).sum()) < B and set(m.unique().tolist()) == {0.0, 2.0}
        else:
            assert bool((m == 1).all())
        y = ln(h, "layernorm_before")
        q, k, v = (lin(y, "attention.attention." + n).view(B, T, H, dh).transpose(1, 2) for n in ("query", "key", "value"))
        probs = F.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1) * em(1 + 4 * i, (B, H, T, T))
        ctx = (probs @ v).transpose(1, 2).reshape(B, T, D)
        h = h + m[:, 0].view(B, 1, 1) * (lin(ctx, "attention.output.dense") * em(2 + 4 * i, (B, T, D)))
        g = F.gelu(lin(ln(h, "layernorm_after"), "intermediate.dense"))
        h = h + m[:, 1].view(B, 1, 1) * (lin(g, "output.dense") * em(3 + 4 * i, (B, T, D)))
        assert float((out.hidden_states[i + 1] - h).abs().max()) <= 1e-5 * float(h.abs().max()), i
    assert torch.equal(out.hidden_states[1], plain.hidden_states[1])  # layer 0 never drops
    assert not torch.allclose(out.hidden_states[2], plain.hidden_states[2])


# ------------------------------------------------------------------ C ABI
def test_exports_and_argument_errors():
    from vit_amd import _cabi

    names = _cabi.declared_symbols()
    lib = _cabi.load()
    for name, nargs in (("vit_layernorm_fwd_residual_path", 21), ("vit_layernorm_bwd_path", 26)):
        assert name in names and hasattr(lib, name) and len(_cabi._PROTOS[name]) == nargs
    P = 64  # any non-null address: every call below fails its argument check before anything is launched or read

    def fwd(x=P, xrs=1, delta=P, rows=4, D=32, p=0.1, rps=2, branch=0):
        return lib.vit_layernorm_fwd_residual_path(None, x, xrs, delta, 1, P, P, P, P, 1, None, None, rows, D, 1e-12, p, 7, 4, rps,
                                                   branch, None)

    def bwd(dyn=P, dbias=P, dres_rs=0, rs=1, p=0.1, rps=2, branch=0, drop_p=0.0):
        return lib.vit_layernorm_bwd_path(None, P, 1, P, P, P, P, None, dres_rs, P, P, P, 4, 32, dyn, 1, dbias, drop_p, 7, 3, rs, p,
                                          4, rps, branch, None)

    cases = [(fwd(x=None), b"null pointer"), (fwd(delta=None), b"null pointer"), (fwd(p=1.0), b"path_p"), (fwd(p=-0.1), b"path_p"),
             (fwd(rps=0), b"rows_per_sample"), (fwd(branch=2), b"branch"), (fwd(branch=-1), b"branch"), (fwd(xrs=0), b"x_row_stride"),
             (fwd(xrs=1 << 30), b"x_row_stride"), (fwd(D=30), b"multiple of 4")]
    for rc, _ in cases:
        assert rc == -1
    for call, text in ((lambda: fwd(x=None), b"null pointer"), (lambda: fwd(p=1.0), b"path_p out of [0,1)"),
                       (lambda: fwd(rps=0), b"rows_per_sample=0"), (lambda: fwd(branch=2), b"branch=2"),
                       (lambda: fwd(xrs=0), b"x_row_stride=0"),
                       (lambda: bwd(dyn=None), b"null pointer"), (lambda: bwd(dbias=None), b"null pointer"),
                       (lambda: bwd(p=1.0), b"path_p out of [0,1)"), (lambda: bwd(p=-0.5), b"path_p out of [0,1)"),
                       (lambda: bwd(rps=-3), b"rows_per_sample=-3"), (lambda: bwd(branch=2), b"branch=2"),
                       (lambda: bwd(rs=0), b"row_stride=0"), (lambda: bwd(rs=2, dres_rs=2), b"compact dres"),
                       (lambda: bwd(drop_p=1.0), b"dropout_p")):
        assert call() == -1
        assert text in lib.vit_last_error(), (text, lib.vit_last_error())
