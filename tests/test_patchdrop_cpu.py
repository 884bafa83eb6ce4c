"""Patch dropout (`model.patch_drop_rate`, include/vit_amd_patchdrop.h) without a GPU: the config key and timm's kept count, the
host restatement of the selection (tests/_patchdrop_ref.py) and its statistics, the C ABI's declarations and argument errors."""
import numpy as np
import pytest

from _patchdrop_ref import kept, select, select_site, slot_of, worst_sigma

KW = dict(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2,
          stride_size=32)


def cfg_with_patches(N, **kw):
    from vit_amd.config import ViTConfig

    c = ViTConfig(**dict(KW, image_size=8 * N, patch_size=8, stride_size=8), **kw)
    assert c.num_patches == N
    return c


def test_config_carries_the_rate():
    from vit_amd.config import ViTConfig, get_vit_config

    model = dict(KW, proj_fn="SW")
    assert get_vit_config(dict(model=dict(model))).patch_drop_rate == 0.0
    assert get_vit_config(dict(model=dict(model, patch_drop_rate=0.5))).patch_drop_rate == 0.5
    c = ViTConfig(**KW)
    assert c.patch_drop_rate == 0.0 and c.num_kept_patches == c.num_patches == 8
    assert ViTConfig(**KW, patch_drop_rate=0.0).num_kept_patches == 8
    assert ViTConfig(**KW, patch_drop_rate=0.5).num_kept_patches == 4


@pytest.mark.parametrize("N,rate,K", [(196, 0.5, 98), (196, 0.25, 147), (13, 0.75, 3), (9, 0.99, 1), (196, 0.001, 195)])
def test_kept_count_is_timms(N, rate, K):
    assert cfg_with_patches(N, patch_drop_rate=rate).num_kept_patches == K == kept(N, rate)


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5])
def test_rates_outside_the_unit_interval_raise(bad):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    with pytest.raises(ValueError, match="patch_drop_rate"):
        ViTConfig(**KW, patch_drop_rate=bad)
    c = ViTConfig(**KW)
    c.patch_drop_rate = bad  # set behind the constructor's back: the engine reads the rate itself
    with pytest.raises(ValueError, match="patch_drop_rate"):
        MyViT(c, loss_name="mae")


def test_no_new_parameter_and_the_engine_reads_the_rate_per_forward():
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    plain, dropping = MyViT(ViTConfig(**KW), loss_name="mae"), MyViT(ViTConfig(**KW, patch_drop_rate=0.5), loss_name="mae")
    assert plain.name == dropping.name and list(plain.state_dict()) == list(dropping.state_dict())
    eng = dropping.engine
    assert eng.patch_keep is None
    assert eng.kept_count(training=True) == 4 and eng.kept_count(training=False) is None
    assert plain.engine.kept_count(training=True) is None
    eng.cfg.patch_drop_rate = 1e-17  # 1 - rate rounds to 1 in doubles, K == N: off
    assert eng.cfg.num_kept_patches == 8 and eng.kept_count(training=True) is None
    eng.cfg.patch_drop_rate = 0.001  # int(8 * 0.999) = 7
    assert eng.kept_count(training=True) == 7
    eng.cfg.patch_drop_rate = 0.75
    assert eng.kept_count(training=True) == 2


@pytest.mark.parametrize("B,N,K", [(3, 1, 1), (5, 13, 3), (4, 196, 98), (2, 257, 256), (64, 16, 8)])
def test_restated_selection_properties(B, N, K):
    idx, slot = select(B, N, K, 0x1234567, select_site(12))
    assert idx.shape == (B, K) and slot.shape == (B, N) and idx.dtype == slot.dtype == np.int32
    assert idx.min() >= 0 and idx.max() < N and bool((np.diff(idx, axis=1) > 0).all())
    assert ((slot >= 0).sum(axis=1) == K).all()
    for b in range(B):
        assert np.array_equal(slot[b, idx[b]], np.arange(K))
        assert set(np.flatnonzero(slot[b] < 0)) == set(range(N)) - set(idx[b].tolist())
    assert np.array_equal(slot_of(idx, N), slot)
    # a bound record's keys change the draw; another site does too
    if N > K:
        other, _ = select(B, N, K, 0x1234567, select_site(12), keys_xor=(0x9E3779B9, 0x7F4A7C15))
        assert other.shape == idx.shape and (B * K < 8 or not np.array_equal(other, idx))


@pytest.mark.parametrize("B,N,K", [(4096, 16, 8), (4096, 13, 3), (2048, 196, 98)])
def test_marginal_keep_frequency(B, N, K):
    assert select_site(12) == 49
    idx, _ = select(B, N, K, 0x1234567, 49)
    w = worst_sigma(idx, N)
    print(f"(B, N, K) = ({B}, {N}, {K}): worst deviation of a patch's keep frequency from K/N = {w:.2f} sigma")
    assert w < 5.0


def test_the_site_is_free():
    from oracle import dropmask as dm

    for L in (1, 2, 12, 24):
        used = {0} | {dm.site_of(i, w) for i in range(L) for w in range(4)}
        assert select_site(L) not in used and select_site(L) == max(used) + 1


def test_exports_and_argument_errors():
    from vit_amd import _cabi

    names = _cabi.declared_symbols()
    lib = _cabi.load()
    for name, nargs in (("vit_patch_select", 9), ("vit_patch_slot", 7), ("vit_unfold_gather_cast", 12), ("vit_embed_finish_gather", 13),
                        ("vit_embed_finish_gather_bwd", 16), ("vit_rows_gather", 9), ("vit_fold_add_gather", 11)):
        assert name in names and hasattr(lib, name) and len(_cabi._PROTOS[name]) == nargs, name
    P = 64  # any non-null address: every call below fails its argument check before anything is launched or read
    for call, text in (
            (lambda: lib.vit_patch_select(None, None, P, 2, 8, 4, 1, 9, None), b"null pointer"),
            (lambda: lib.vit_patch_select(None, P, P, 2, 8, 9, 1, 9, None), b"K=9"),
            (lambda: lib.vit_patch_select(None, P, P, 2, 8, 0, 1, 9, None), b"K=0"),
            (lambda: lib.vit_patch_select(None, P, P, 2, 8193, 5, 1, 9, None), b"exceeds the supported 8192"),
            (lambda: lib.vit_patch_slot(None, P, None, 2, 8, 4, None), b"null pointer"),
            (lambda: lib.vit_unfold_gather_cast(None, P, None, P, 1, 2, 64, 8, 8, 8, 4, None), b"null pointer"),
            (lambda: lib.vit_unfold_gather_cast(None, P, P, P, 1, 2, 64, 6, 8, 8, 4, None), b"multiple of 4"),
            (lambda: lib.vit_unfold_gather_cast(None, P, P, P, 1, 2, 64, 8, 8, 9, 4, None), b"starts past the signal"),
            (lambda: lib.vit_embed_finish_gather(None, P, P, None, None, 2, 5, 9, 32, 0.0, 1, 0, None), b"null pointer"),
            (lambda: lib.vit_embed_finish_gather(None, P, P, None, P, 2, 10, 9, 32, 0.0, 1, 0, None), b"Tc=10"),
            (lambda: lib.vit_embed_finish_gather(None, P, P, None, P, 2, 5, 9, 32, 1.0, 1, 0, None), b"dropout_p"),
            (lambda: lib.vit_embed_finish_gather_bwd(None, P, None, P, 1, P, None, 2, 5, 9, 32, 0.0, 1, 0, 0, None), b"null pointer"),
            (lambda: lib.vit_embed_finish_gather_bwd(None, P, P, P, 1, P, None, 2, 5, 9, 30, 0.0, 1, 0, 0, None), b"D=30"),
            (lambda: lib.vit_rows_gather(None, P, P, P, 2, 5, 9, 6, None), b"W=6"),
            (lambda: lib.vit_fold_add_gather(None, P, P, P, 2, 64, 8, 8, 8, 9, None), b"K=9")):
        assert call() == -1
        assert text in lib.vit_last_error(), (text, lib.vit_last_error())
    # a call that passes its checks states its workspace need before anything is launched (no handle: it holds none)
    assert lib.vit_embed_finish_gather_bwd(None, P, P, P, 1, P, None, 32, 5, 9, 32, 0.0, 1, 0, 0, None) == _cabi.VIT_ERR_WORKSPACE
    assert lib.vit_workspace_needed() == 16 * 9 * 32 * 4
