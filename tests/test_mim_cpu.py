"""Masked spectrum modelling (`model.task_type: mim`, include/vit_amd_mim.h) without a GPU: the host restatement of the block
mask, the parameter layout (a 'mim' model's, and that nothing moved for 'cls' / 'reg'), config validation and the two exclusion
errors, the `model.init_from` hand-over on CPU state dicts, the restated loss against HF's SimMIM formula, and the C ABI's
declarations and argument errors."""
import json
import os
import types

import numpy as np
import pytest
import torch

import _mim_ref as mr
from _patchdrop_ref import select_site

KW = dict(image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, stride_size=32)
SEED = 0x1234567


@pytest.mark.parametrize("B,N,span,ratio", [(3, 1, 1, 0.6), (5, 13, 3, 0.6), (4, 196, 4, 0.6), (2, 4089, 7, 0.75), (6, 10, 1, 0.5),
                                             (3, 9, 2, 0.99)])
def test_restated_mask_has_kb_visible_blocks_and_a_short_last_block(B, N, span, ratio):
    from vit_amd.config import mim_blocks

    Nb, Kb = mr.blocks(N, span, ratio)
    assert (Nb, Kb) == mim_blocks(N, span, ratio) and Nb == -(-N // span) and 1 <= Kb <= Nb
    m = mr.mask(B, N, span, ratio, SEED, select_site(2))
    assert m.shape == (B, N) and m.dtype == np.int32 and set(np.unique(m)) <= {0, 1}
    last = N - (Nb - 1) * span  # the last block's length: span, or shorter
    assert 1 <= last <= span
    for b in range(B):
        per_block = [m[b, k * span:(k + 1) * span] for k in range(Nb)]
        assert all(len(set(blk.tolist())) == 1 for blk in per_block)  # a block is masked or visible as a whole
        assert len(per_block[-1]) == last
        visible = [k for k, blk in enumerate(per_block) if blk[0] == 0]
        assert len(visible) == Kb
        # the count per sample follows from whether the short block is masked
        assert int(m[b].sum()) == (Nb - Kb) * span - ((span - last) if per_block[-1][0] else 0)
    if Nb > Kb and B * Nb >= 8:
        other = mr.mask(B, N, span, ratio, SEED, select_site(2), keys_xor=(0x9E3779B9, 0x7F4A7C15))
        assert not np.array_equal(other, m)


def test_cls_and_reg_layouts_did_not_move():
    """The reference's state_dict (oracle.refvit.param_shapes, pinned on the reference) names and shapes every entry of the
    'cls' / 'reg' layouts, in `state_order`; offsets are the running ALIGN-ed sum in the engine's own order; run names are
    tests/golden/names.json's."""
    from oracle import refvit
    from vit_amd.config import ViTConfig
    from vit_amd.engine import ALIGN, ParamLayout
    from vit_amd.specvit import build_model_name

    for task, pos, nl in (("reg", None, 1), ("reg", "learned", 3), ("cls", "rope", 5)):
        cfg = ViTConfig(task_type=task, pos_encoding_type=pos, num_labels=nl, **KW)
        rc = refvit.RefConfig(task_type=task, pos_encoding_type=pos, num_labels=nl, **KW)
        lay = ParamLayout(cfg)
        shapes = refvit.param_shapes(rc)
        assert lay.state_order == list(shapes)
        assert {k: v[1] for k, v in lay.entries.items()} == {k: tuple(v) for k, v in shapes.items()}
        assert not any("mask_token" in k or k.startswith("decoder") for k in lay.entries)
        off = 0
        for name, (o, shape) in lay.entries.items():  # insertion order = buffer order
            assert o == off, name
            off += -(-int(np.prod(shape)) // ALIGN) * ALIGN
        assert lay.n_total == off and lay.head == ("classifier" if task == "cls" else "regressor")
    with open(os.path.join(os.path.dirname(__file__), "golden", "names.json")) as f:
        doc = json.load(f)
    for rec in doc["names"]:
        c = rec["case"]
        ns = types.SimpleNamespace(**{k: v for k, v in c.items() if k != "noise"})
        assert build_model_name(ns, "ViT", full_config={"noise": {"noise_level": c["noise"]}}) == rec["ViT"]
        ns.task_type = "mim"
        assert build_model_name(ns, "ViT", full_config={"noise": {"noise_level": c["noise"]}}) == rec["ViT"] + "_mim"


def test_mim_layout_and_model_surface():
    from vit_amd.config import ViTConfig
    from vit_amd.engine import ParamLayout
    from vit_amd.specvit import MyViT

    for pos in (None, "learned"):
        cfg = ViTConfig(task_type="mim", pos_encoding_type=pos, **KW)
        reg = ParamLayout(ViTConfig(task_type="reg", pos_encoding_type=pos, **KW))
        lay = ParamLayout(cfg)
        e = "vit.embeddings."
        # mask_token: inside the embedding range, the last entry of the embedding block in the buffer and in state_order
        off, shape = lay.entries[e + "mask_token"]
        assert shape == (1, 1, 32) and lay.embed_start <= off < lay.embed_end
        assert off == max(o for n, (o, _) in lay.entries.items() if n.startswith(e))
        i = lay.state_order.index(e + "mask_token")
        assert lay.state_order[i - 1] == e + "patch_embeddings.projection.bias" and lay.state_order[i + 1].startswith("vit.encoder.")
        assert lay.head == "decoder" and lay.entries["decoder.weight"][1] == (32, 32) and lay.entries["decoder.bias"][1] == (32,)
        assert lay.state_order[-2:] == ["decoder.weight", "decoder.bias"]
        # everything else is the regression model's, in its order
        strip = lambda order: [n for n in order if "mask_token" not in n and not n.startswith(("decoder", "regressor"))]
        assert strip(lay.state_order) == strip(reg.state_order)
    model = MyViT(ViTConfig(task_type="mim", **dict(KW, patch_size=16, stride_size=16)), loss_name="mae")
    sd = model.state_dict()
    assert model.name.endswith("_mim") and model.loss_name == "mim"
    assert sd["decoder.weight"].shape == (16, 32) and float(sd["vit.embeddings.mask_token"].abs().max()) == 0.0
    assert float(sd["decoder.bias"].abs().max()) == 0.0 and 0.0 < float(sd["decoder.weight"].std()) < 0.05
    assert model.engine.mim and model.engine.mim_mask is None
    with pytest.raises(ValueError, match="bool_masked_pos"):
        MyViT(ViTConfig(task_type="reg", **KW), loss_name="mae")(torch.zeros(1, 256), bool_masked_pos=torch.zeros(1, 8))
    # the evaluation masks' seed: a function of (base_seed, forwards since eval()) alone
    eng = model.engine
    eng.base_seed = 77
    model.eval()
    a = [eng.mim_seed(False, 123), eng.mim_seed(False, 456)]
    model.eval()
    assert [eng.mim_seed(False, 9), eng.mim_seed(False, 9)] == a and a[0] != a[1]
    assert a[0] == ((77 ^ 0x6D696D5F6576616C) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    assert eng.mim_seed(True, 123) == 123


def test_config_validation_and_exclusions():
    from vit_amd.config import ViTConfig, get_vit_config

    model = dict(KW, proj_fn="SW", task_type="mim")
    c = get_vit_config(dict(model=dict(model)))
    assert (c.task_type, c.mim_mask_ratio, c.mim_span, c.mim_loss, c.mim_norm_target) == ("mim", 0.6, 1, "l1", False)
    c = get_vit_config(dict(model=dict(model), mim=dict(mask_ratio=0.75, span=4, loss="MSE", norm_target=True)))
    assert (c.mim_mask_ratio, c.mim_span, c.mim_loss, c.mim_norm_target) == (0.75, 4, "mse", True)
    for bad in (0.0, 1.0, -0.1, 1.5, True, "0.5"):
        with pytest.raises(ValueError, match="mask_ratio"):
            get_vit_config(dict(model=dict(model), mim=dict(mask_ratio=bad)))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="span"):
            get_vit_config(dict(model=dict(model), mim=dict(span=bad)))
    with pytest.raises(ValueError, match="mim.loss"):
        get_vit_config(dict(model=dict(model), mim=dict(loss="huber")))
    with pytest.raises(ValueError, match="norm_target"):
        get_vit_config(dict(model=dict(model), mim=dict(norm_target="yes")))
    with pytest.raises(ValueError, match="unknown key"):
        get_vit_config(dict(model=dict(model), mim=dict(ratio=0.5)))
    # the two exclusions name both keys
    with pytest.raises(ValueError, match=r"(?s)patch_drop_rate.*mim"):
        get_vit_config(dict(model=dict(model, patch_drop_rate=0.5)))
    with pytest.raises(ValueError, match=r"(?s)augment.*mim"):
        get_vit_config(dict(model=dict(model), augment=dict(mixup_alpha=0.8)))
    with pytest.raises(ValueError, match=r"(?s)augment.*mim"):
        get_vit_config(dict(model=dict(model), augment=dict(cutmix_alpha=1.0)))
    # a section that is present for another task is not read
    assert get_vit_config(dict(model=dict(model, task_type="reg"), data=dict(param="log_g"), mim=dict(span=0))).task_type == "reg"
    assert ViTConfig(task_type="reg", mim_span=0, **KW).mim_span == 0


def test_shipped_config_loads():
    from vit_amd.config import get_vit_config, mim_blocks
    from vit_amd.utils import load_config

    cfg = load_config(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "exp", "mim_pretrain.yaml"))
    c = get_vit_config(cfg)
    assert c.task_type == "mim" and c.num_patches == 196 and (c.mim_mask_ratio, c.mim_span, c.mim_loss) == (0.6, 4, "l1")
    assert mim_blocks(c.num_patches, c.mim_span, c.mim_mask_ratio) == (49, 19)


def test_init_from_matches_by_name_and_shape(tmp_path, capsys):
    from vit_amd.builder import get_model, init_from_state
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    torch.manual_seed(5)
    pre = MyViT(ViTConfig(task_type="mim", pos_encoding_type="learned", **KW), loss_name="")
    state = {k: v.detach().clone() for k, v in pre.state_dict().items()}
    torch.manual_seed(6)
    reg = MyViT(ViTConfig(task_type="reg", pos_encoding_type="learned", **KW), loss_name="mae")
    before = {k: v.detach().clone() for k, v in reg.state_dict().items()}
    loaded, skipped_ckpt, skipped_model = init_from_state(reg, state)
    assert skipped_ckpt == ["decoder.bias", "decoder.weight", "vit.embeddings.mask_token"]
    assert skipped_model == ["regressor.bias", "regressor.weight"]
    after = reg.state_dict()
    assert set(loaded) == set(after) - set(skipped_model)
    assert all(torch.equal(after[k], state[k]) for k in loaded)
    assert all(torch.equal(after[k], before[k]) for k in skipped_model)
    text = capsys.readouterr().out
    assert "decoder.weight" in text and "mask_token" in text and "regressor.weight" in text
    # a same-named tensor of another shape is skipped on both sides; nothing matching at all raises
    other = MyViT(ViTConfig(task_type="reg", **dict(KW, hidden_size=64)), loss_name="mae")
    with pytest.raises(ValueError, match="init_from"):
        init_from_state(other, state)
    # through the config: a Lightning-layout file (names under `model.`), as the trainer writes it
    path = str(tmp_path / "pre.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in state.items()}}, path)
    model = dict(KW, proj_fn="SW", task_type="reg", pos_encoding_type="learned", init_from=path)
    got = get_model(dict(model=model, data=dict(param="log_g"), loss=dict(name="mae")))
    assert all(torch.equal(got.state_dict()[k], state[k]) for k in loaded)


def test_restated_loss_is_hfs_simmim_loss():
    """HF ViTForMaskedImageModeling with S == P, L1, span 1: (|x - rec| * mask).sum() / (mask.sum() + 1e-5) / num_channels,
    mask repeated over each patch's P samples; the restatement drops the 1e-5."""
    g = torch.Generator().manual_seed(11)
    B, N, P = 4, 12, 16
    x = torch.randn(B, N * P, generator=g)
    rec = torch.randn(B, N, P, generator=g)
    m = mr.mask(B, N, 1, 0.6, SEED, select_site(2))
    mt = torch.from_numpy(m).float()
    wide = mt.repeat_interleave(P, dim=1)  # [B, L]
    hf = ((x - rec.reshape(B, N * P)).abs() * wide).sum() / (wide.sum() + 1e-5)
    ours = mr.loss(rec, x, m, P, P, "l1")
    assert abs(float(ours) - float(hf)) <= 1e-6 * abs(float(hf)), (float(ours), float(hf))
    # the targets: ragged tail zero, normalisation per window with the unbiased variance
    t = mr.targets(torch.arange(19.0)[None, :], 8, 6, 3)  # window 2 would need samples 12 .. 19: it does not fit
    assert t[0, 0].tolist() == list(range(8)) and t[0, 1].tolist() == list(range(6, 14)) and t[0, 2].abs().max() == 0
    tn = mr.targets(x, P, P, N, norm=True)
    assert float(tn.mean(-1).abs().max()) < 1e-5 and float((tn.var(-1, unbiased=True) - 1).abs().max()) < 1e-4
    assert float(mr.loss(rec, x, np.zeros((B, N), np.int32), P, P, "mse")) == 0.0


def test_exports_and_argument_errors():
    from vit_amd import _cabi

    names = _cabi.declared_symbols()
    lib = _cabi.load()
    for name, nargs in (("vit_mim_mask", 8), ("vit_embed_finish_masked", 13), ("vit_embed_finish_masked_bwd", 16),
                        ("vit_mim_loss_fwd", 16), ("vit_mim_loss_bwd", 18)):
        assert name in names and hasattr(lib, name) and len(_cabi._PROTOS[name]) == nargs, name
    P = 64  # any non-null address: every call below fails its argument check before anything is launched or read
    for call, text in (
            (lambda: lib.vit_mim_mask(None, P, None, 2, 8, 8, 1, None), b"null pointer"),
            (lambda: lib.vit_mim_mask(None, P, P, 2, 8, 8, 0, None), b"span=0"),
            (lambda: lib.vit_mim_mask(None, P, P, 2, 13, 4, 3, None), b"Nb=4"),
            (lambda: lib.vit_embed_finish_masked(None, P, P, None, None, P, 2, 9, 32, 0.0, 1, 0, None), b"null pointer"),
            (lambda: lib.vit_embed_finish_masked(None, P, P, None, P, None, 2, 9, 32, 0.0, 1, 0, None), b"null pointer"),
            (lambda: lib.vit_embed_finish_masked(None, P, P, None, P, P, 2, 9, 30, 0.0, 1, 0, None), b"D=30"),
            (lambda: lib.vit_embed_finish_masked(None, P, P, None, P, P, 2, 9, 32, 1.0, 1, 0, None), b"dropout_p"),
            (lambda: lib.vit_embed_finish_masked_bwd(None, P, P, P, 1, P, None, None, 2, 9, 32, 0.0, 1, 0, 0, None), b"null pointer"),
            (lambda: lib.vit_embed_finish_masked_bwd(None, P, P, P, 7, P, None, P, 2, 9, 32, 0.0, 1, 0, 0, None), b"bad dtype"),
            (lambda: lib.vit_mim_loss_fwd(None, P, P, 0, P, P, None, 2, 64, 8, 8, 8, 9, 1, 0, None), b"null pointer"),
            (lambda: lib.vit_mim_loss_fwd(None, P, P, 0, P, P, P, 2, 64, 8, 8, 8, 8, 1, 0, None), b"T=8 must be N + 1"),
            (lambda: lib.vit_mim_loss_fwd(None, P, P, 0, P, P, P, 2, 64, 8, 8, 8, 9, 2, 0, None), b"kind 2"),
            (lambda: lib.vit_mim_loss_fwd(None, P, P, 0, P, P, P, 2, 64, 6, 8, 8, 9, 1, 0, None), b"multiple of 4"),
            (lambda: lib.vit_mim_loss_fwd(None, P, P, 0, P, P, P, 2, 64, 8, 8, 9, 10, 1, 0, None), b"starts past the signal"),
            (lambda: lib.vit_mim_loss_bwd(None, P, P, 0, P, None, P, P, 0, 2, 64, 8, 8, 8, 9, 1, 0, None), b"null pointer"),
            (lambda: lib.vit_mim_loss_bwd(None, P, P, 0, P, P, P, P, 0, 2, 64, 8, 8, 8, 7, 0, 0, None), b"T=7 must be N + 1"),
            (lambda: lib.vit_mim_loss_bwd(None, P, P, 0, P, P, P, P, 0, 2, 64, 8, 8, 8, 9, 4, 0, None), b"kind 4")):
        assert call() == -1
        assert text in lib.vit_last_error(), (text, lib.vit_last_error())
    # calls that pass their checks state their workspace need before anything is launched (no handle: it holds none)
    assert lib.vit_embed_finish_masked_bwd(None, P, P, P, 1, P, None, P, 32, 9, 32, 0.0, 1, 0, 0, None) == _cabi.VIT_ERR_WORKSPACE
    assert lib.vit_workspace_needed() == 2 * 16 * 9 * 32 * 4
    assert lib.vit_mim_loss_fwd(None, P, P, 0, P, P, P, 2, 64, 8, 8, 8, 9, 1, 0, None) == _cabi.VIT_ERR_WORKSPACE
    assert lib.vit_workspace_needed() == 2 * 8 * 4
