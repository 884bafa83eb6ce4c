"""CPU checks of oracle/dropmask.py (the host restatement of the kernels' dropout masks) and of the oracle's `masks=` plumbing.

The GPU side (tests/test_dropout_gpu.py, the train-mode parity tests) compares kernels against this restatement bit for bit,
so it is checked here against a second, scalar restatement written line by line from vit_amd/csrc/common.h, and for the
statistics a mask has to have."""
import numpy as np
import pytest
import torch

from oracle import dropmask as dm

M32 = 0xFFFFFFFF


# ---- scalar restatement of common.h:66-104, one element at a time (independent of the vectorised one)
def _hash_scalar(k0, k1, idx):
    x = (idx & M32) ^ k0 ^ (((idx >> 32) * 0x9E3779B9) & M32)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x = (x + k1) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def _bits_scalar(rowkey, colpair):
    x = ((colpair ^ rowkey) * 0x2C1B3C6D) & M32
    x ^= x >> 15
    x = (x * 0x297A2D39) & M32
    x ^= x >> 16
    return x


def _mult_scalar(cfg, row, col):
    thr, scale, k0, k1 = cfg
    if thr == 0:
        return 1.0
    h = _bits_scalar(_hash_scalar(k0, k1, row), col >> 1)
    r16 = (h >> 16) if (col & 1) else (h & 0xFFFF)
    return scale if r16 >= thr else 0.0


@pytest.mark.parametrize("p,thr", [(0.0, 0), (0.1, 6554), (0.5, 32768), (1e-6, 0), (1e-5, 1), (0.25, 16384),
                                   (0.99999, 65535), (0.999999, 65535), (0.9999999, 65535)])
def test_thr_and_scale_exact(p, thr):
    """thr = (unsigned)(p * 65536.0f + 0.5f), clamped to 65535; scale = 65536.0f / (65536 - thr) in float32."""
    t, s = dm.thr_scale(p)
    assert t == thr
    assert s == float(np.float32(65536.0) / np.float32(65536 - thr))
    if thr == 32768:
        assert s == 2.0
    if thr == 65535:
        assert s == 65536.0  # the clamp: one draw in 65536 survives, scaled by 65536
    if p == 0.1:
        assert s != float(np.float32(1 / 0.9))  # the kept scale is NOT 1 / (1 - p)
    cfg = dm.drop_cfg(p, 7, 3)
    assert cfg[:2] == (t, s)
    if thr == 0:  # p = 1e-6 rounds to "off": the kernels then skip the mask entirely
        assert np.all(dm.multiplier(cfg, 8, 16) == 1.0)


def test_keys_are_splitmix64_of_seed_and_site():
    # splitmix64(0x9E3779B97F4A7C15) -- the first output of the SplitMix64 generator seeded with 0
    assert dm.splitmix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    _, _, k0, k1 = dm.drop_cfg(0.1, 0, 0)
    assert (k1 << 32) | k0 == 0xE220A8397B1DCDAF
    # seed arithmetic wraps at 2^64
    big = (1 << 64) - 5
    assert dm.drop_cfg(0.1, big, 4)[2:] == dm.drop_cfg(0.1, big - (1 << 64), 4)[2:]
    assert dm.step_seed(2 ** 63, 3) == (2 ** 63 + 3 * dm.PHI) % 2 ** 64
    assert dm.step_keys(11, 5) == dm.drop_cfg(0.1, 11 + dm.PHI * 4, 0)[2:]  # the same mixer, seed + phi * step


@pytest.mark.parametrize("p,seed,site,row0", [(0.1, 1234, 7, 0), (0.3, 2 ** 63 + 17, 0, 2 ** 32 - 3), (0.5, 5, 49, 10 ** 6)])
def test_vectorised_equals_scalar_restatement(p, seed, site, row0):
    cfg = dm.drop_cfg(p, seed, site)
    rows, cols = 6, 37  # odd column count: the last pair is half used
    got = dm.multiplier(cfg, rows, cols, row0=row0)
    exp = np.array([[_mult_scalar(cfg, row0 + r, c) for c in range(cols)] for r in range(rows)], dtype=np.float32)
    assert np.array_equal(got, exp)
    # with a bound record's keys XORed in
    kx = (0xDEADBEEF, 0x01234567)
    got = dm.multiplier(cfg, rows, cols, row0=row0, keys_xor=kx)
    c2 = (cfg[0], cfg[1], cfg[2] ^ kx[0], cfg[3] ^ kx[1])
    exp = np.array([[_mult_scalar(c2, row0 + r, c) for c in range(cols)] for r in range(rows)], dtype=np.float32)
    assert np.array_equal(got, exp)
    # p = 0: the record changes nothing (resolve_drop only XORs when thr != 0)
    assert np.all(dm.multiplier(dm.drop_cfg(0.0, seed, site), rows, cols, keys_xor=kx) == 1.0)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.02])
def test_keep_rate_within_binomial_bounds(p):
    cfg = dm.drop_cfg(p, 99, 2)
    keep = dm.keep_mask(cfg, 1000, 1000)
    q = 1.0 - cfg[0] / 65536.0  # exact keep probability of a uniform 16-bit draw
    sd = (q * (1 - q) / keep.size) ** 0.5
    assert abs(keep.mean() - q) < 5 * sd, (keep.mean(), q)
    # unbiased: E[multiplier] = q * scale = 1
    assert abs(q * cfg[1] - 1.0) < 1e-6


def test_draws_are_uniform_and_uncorrelated():
    """|corr| < 0.01 over 10^6 draws between the two halves of one word, neighbouring column pairs and neighbouring rows
    (common.h:63 records 0.07 between adjacent pairs for a single multiply-xorshift round)."""
    cfg = dm.drop_cfg(0.1, 2024, 5)
    r = dm.draws(cfg, 1001, 1000).astype(np.float64)
    assert abs(r.mean() / 65535.0 - 0.5) < 2e-3
    hist = np.bincount((r.astype(np.int64) >> 12).ravel(), minlength=16) / r.size
    assert np.all(np.abs(hist - 1 / 16) < 2e-3)

    def corr(a, b):
        return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])

    body = r[:1000]
    pairs = {
        "halves of a word": corr(body[:, 0::2], body[:, 1::2]),
        "neighbouring pairs": corr(body[:, 0:-2:2], body[:, 2::2]),
        "neighbouring pairs, high halves": corr(body[:, 1:-2:2], body[:, 3::2]),
        "neighbouring rows": corr(r[:-1], r[1:]),
    }
    for what, c in pairs.items():
        assert abs(c) < 0.01, (what, c)
    # and the keep indicators themselves
    k = r >= cfg[0]
    assert abs(corr(k[:1000, 0:-2:2], k[:1000, 2::2])) < 0.01 and abs(corr(k[:-1], k[1:])) < 0.01
    # sites and seeds give independent masks
    o = dm.draws(dm.drop_cfg(0.1, 2024, 6), 1000, 1000).astype(np.float64)
    assert abs(corr(body, o)) < 0.01


def test_step_record():
    base = 0x0123456789ABCDEF
    k0, k1, bc1, rbc2, step = dm.step_record(base, 5)
    assert (k0, k1) == dm.step_keys(base, 5) and step == 5
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))  # the kernel receives the betas as float
    assert bc1 == np.float32(1.0 - b1 ** 5) and rbc2 == np.float32(1.0 / np.sqrt(1.0 - b2 ** 5))
    assert abs(float(bc1) - (1 - 0.9 ** 5)) < 1e-6


def test_layout_helpers():
    cfg = dm.drop_cfg(0.1, 3, 1)
    B, H, T, D = 2, 3, 5, 8
    a = dm.attn_multiplier(cfg, B, H, T)
    full = dm.multiplier(cfg, B * H * T, T)
    assert a.shape == (B, H, T, T)
    b, h, q, k = 1, 2, 3, 4
    assert a[b, h, q, k] == full[(b * H + h) * T + q, k]
    hm = dm.hidden_multiplier(cfg, B, T, D)
    assert hm[1, 2, 5] == dm.multiplier(cfg, B * T, D)[1 * T + 2, 5]
    assert dm.site_of(0, 0) == 1 and dm.site_of(2, 2) == 11


# ---- the oracle's masks= plumbing
def _small():
    from oracle import refvit

    rc = refvit.RefConfig(image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
                          stride_size=32, loss_name="mae")
    sd = refvit.make_state_dict(rc, 3)
    x, _, y = refvit.make_inputs(rc, 3, 4)
    return rc, sd, x, y


def test_oracle_all_keep_masks_equal_eval():
    from oracle import refvit

    rc, sd, x, y = _small()
    calls = []

    def ones(site, shape):
        calls.append((site, shape))
        return torch.ones(shape)

    ev = refvit.forward(rc, sd, x, y, output_hidden_states=True)
    tr = refvit.forward(rc, sd, x, y, training=True, masks=ones, output_hidden_states=True)
    assert torch.equal(ev.logits, tr.logits) and torch.equal(ev.loss, tr.loss)
    for a, b in zip(ev.hidden_states, tr.hidden_states):
        assert torch.equal(a, b)
    B, T, D, H = 3, rc.seq_len, rc.hidden_size, rc.num_attention_heads
    exp = [(0, (B, T, D))]
    for i in range(rc.num_hidden_layers):
        exp += [(dm.site_of(i, 0), (B, H, T, T)), (dm.site_of(i, 1), (B, T, D)), (dm.site_of(i, 2), (B, T, D))]
    assert calls == exp
    # eval mode never consults the masks
    calls.clear()
    refvit.forward(rc, sd, x, y, training=False, masks=ones)
    assert calls == []


@pytest.mark.parametrize("layer,which", [(1, 0), (1, 1), (1, 2), (2, 2), (None, None)])
def test_oracle_one_site_mask_changes_only_downstream(layer, which):
    from oracle import refvit

    rc, sd, x, y = _small()
    target = 0 if layer is None else dm.site_of(layer, which)
    real = dm.engine_masks(0.1, 0.1, 77)

    def one(site, shape):
        return real(site, shape) if site == target else torch.ones(shape)

    ev = refvit.forward(rc, sd, x, y, output_hidden_states=True)
    tr = refvit.forward(rc, sd, x, y, training=True, masks=one, output_hidden_states=True)
    first_changed = 0 if layer is None else layer + 1  # hidden_states[i + 1] is layer i's output
    for i, (a, b) in enumerate(zip(ev.hidden_states, tr.hidden_states)):
        if i < first_changed:
            assert torch.equal(a, b), i
        else:
            assert not torch.equal(a, b), i
    assert not torch.equal(ev.logits, tr.logits)


def test_engine_masks_match_site_configs():
    masks = dm.engine_masks(0.1, 0.2, 12345)
    m = masks(5, (2, 3, 7, 7)).numpy()  # attention site of layer 1
    assert np.array_equal(m, dm.attn_multiplier(dm.drop_cfg(0.2, 12345, 5), 2, 3, 7))
    m = masks(6, (2, 7, 16)).numpy()
    assert np.array_equal(m, dm.hidden_multiplier(dm.drop_cfg(0.1, 12345, 6), 2, 7, 16))
    kx = dm.step_keys(9, 4)
    m = dm.engine_masks(0.1, 0.1, 12345, keys_xor=kx)(0, (2, 7, 16)).numpy()
    assert np.array_equal(m, dm.hidden_multiplier(dm.drop_cfg(0.1, 12345, 0), 2, 7, 16, keys_xor=kx))


def test_trainer_step_takes_masks():
    from oracle import refvit

    rc, sd, x, y = _small()
    a = refvit.RefTrainer(rc, sd, training=True)
    b = refvit.RefTrainer(rc, sd, training=False)
    la = a.step(x, y, masks=lambda site, shape: torch.ones(shape))
    lb = b.step(x, y)
    assert la == lb
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k
    c = refvit.RefTrainer(rc, sd, training=True)
    assert c.step(x, y, masks=dm.engine_masks(0.1, 0.1, 5)) != lb
