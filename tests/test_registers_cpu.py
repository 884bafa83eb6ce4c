"""Register tokens (`model.num_register_tokens`, include/vit_amd_registers.h) without a GPU: config validation and the exclusion
with patch dropout, the parameter layout (unchanged at 0, one more entry at R), the run name, the no-decay group, the initial
values (every other tensor unchanged by R), the `model.init_from` skip lists both ways, the checkpoint mismatch error, the C
ABI's declarations and argument errors, and the host restatement (tests/_registers_ref.py) against a plain torch composition
under autograd."""
import os

import numpy as np
import pytest
import torch

import _registers_ref as rr

KW = dict(image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, stride_size=32)
E = "vit.embeddings."


def test_config_validation():
    from vit_amd.config import ViTConfig, get_vit_config

    model = dict(KW, proj_fn="SW", task_type="reg")
    data = dict(param="log_g")
    assert get_vit_config(dict(model=dict(model), data=data)).num_register_tokens == 0  # absent means 0
    c = get_vit_config(dict(model=dict(model, num_register_tokens=4), data=data))
    assert c.num_register_tokens == 4 and c.num_patches == 8 and c.seq_len == 1 + 4 + 8
    assert get_vit_config(dict(model=dict(model, num_register_tokens=0), data=data)).seq_len == 9
    for bad in (-1, True, False, 1.5, 2.0, "2", None):
        with pytest.raises(ValueError, match="num_register_tokens"):
            get_vit_config(dict(model=dict(model, num_register_tokens=bad), data=data))
        with pytest.raises(ValueError, match="num_register_tokens"):
            ViTConfig(task_type="reg", num_register_tokens=bad, **KW)
    with pytest.raises(ValueError, match=r"(?s)num_register_tokens.*patch_drop_rate.*not built yet"):
        get_vit_config(dict(model=dict(model, num_register_tokens=2, patch_drop_rate=0.25), data=data))
    # either alone is fine, and so are registers with the masked task and with average pooling
    assert get_vit_config(dict(model=dict(model, num_register_tokens=0, patch_drop_rate=0.25), data=data)).seq_len == 9
    assert get_vit_config(dict(model=dict(model, task_type="mim", num_register_tokens=2))).seq_len == 11
    assert get_vit_config(dict(model=dict(model, global_pool="avg", num_register_tokens=2), data=data)).global_pool == "avg"


@pytest.mark.parametrize("task,pos", [("reg", None), ("reg", "learned"), ("cls", "rope"), ("mim", "learned")])
def test_layout(task, pos):
    from vit_amd.config import ViTConfig
    from vit_amd.engine import ALIGN, ParamLayout

    base = ParamLayout(ViTConfig(task_type=task, pos_encoding_type=pos, **KW))
    zero = ParamLayout(ViTConfig(task_type=task, pos_encoding_type=pos, num_register_tokens=0, **KW))
    # absent or 0: today's layout, entry for entry (names, offsets, shapes, both orders, every range)
    assert list(zero.entries.items()) == list(base.entries.items()) and zero.state_order == base.state_order
    assert (zero.n_total, zero.n_trainable, zero.buckets()) == (base.n_total, base.n_trainable, base.buckets())
    assert not any("register" in k for k in base.entries)
    R, D, N = 3, KW["hidden_size"], 8
    lay = ParamLayout(ViTConfig(task_type=task, pos_encoding_type=pos, num_register_tokens=R, **KW))
    assert set(lay.entries) - set(base.entries) == {E + "register_tokens"} and set(base.entries) <= set(lay.entries)
    names = list(lay.entries)
    assert names.index(E + "register_tokens") == names.index(E + "cls_token") + 1  # directly behind cls_token in the buffer ...
    i = lay.state_order.index(E + "register_tokens")
    assert lay.state_order[i - 1] == E + "cls_token"                               # ... and in state_order
    assert [n for n in lay.state_order if n != E + "register_tokens"] == base.state_order
    off, shape = lay.entries[E + "register_tokens"]
    assert shape == (1, R, D) and lay.embed_start <= off < lay.embed_end  # the embedding block's bucket and exchange
    assert lay.buckets()[-1] == (lay.embed_start, lay.embed_end)
    step = -(-R * D // ALIGN) * ALIGN
    for name, (o, s) in base.entries.items():  # everything behind it moved by the new entry's aligned size, nothing else changed
        assert lay.entries[name] == (o if name == E + "cls_token" else o + step, s), name
    if pos == "learned":  # the position table keeps its 1 + N rows
        assert lay.entries[E + "position_embeddings"][1] == (1, 1 + N, D)


def test_run_name_and_no_decay():
    from vit_amd.config import ViTConfig
    from vit_amd.optimizer import _NO_DECAY_NAMES
    from vit_amd.specvit import MyViT, build_model_name

    plain = ViTConfig(task_type="reg", **KW)
    assert build_model_name(ViTConfig(task_type="reg", num_register_tokens=0, **KW), "ViT") == build_model_name(plain, "ViT")
    assert build_model_name(ViTConfig(task_type="reg", num_register_tokens=4, **KW), "ViT") == build_model_name(plain, "ViT") + "_reg4"
    both = ViTConfig(task_type="reg", global_pool="avg", num_register_tokens=2, **KW)
    assert build_model_name(both, "ViT").endswith("_gap_reg2")
    assert MyViT(ViTConfig(task_type="mim", num_register_tokens=1, **KW), loss_name="").name.endswith("_mim_reg1")
    assert E + "register_tokens" in _NO_DECAY_NAMES


def test_initial_values():
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    def fresh(R, **kw):
        torch.manual_seed(1234)
        return MyViT(ViTConfig(task_type="reg", pos_encoding_type="learned", num_register_tokens=R, **dict(KW, **kw)),
                     loss_name="mae").state_dict()

    base = fresh(0)
    for R in (1, 4):
        sd = fresh(R)
        assert set(sd) - set(base) == {E + "register_tokens"}
        for k, v in base.items():  # the same config and seed start every other tensor from the same values
            assert torch.equal(sd[k], v), k
    # N(0, initializer_range^2): not zeros, no two registers alike, the spread of the other weights
    reg = fresh(8, hidden_size=256, num_attention_heads=4)[E + "register_tokens"]
    assert reg.shape == (1, 8, 256) and 0.018 < float(reg.std()) < 0.022 and abs(float(reg.mean())) < 2e-3
    assert all(not torch.equal(reg[0, i], reg[0, j]) for i in range(8) for j in range(i))


def test_init_from_skip_lists_both_ways(capsys):
    from vit_amd.builder import init_from_state
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    make = lambda R, seed: (torch.manual_seed(seed), MyViT(ViTConfig(task_type="reg", num_register_tokens=R, **KW), loss_name="mae"))[1]
    without, with4 = make(0, 1), make(4, 2)
    # a checkpoint without registers into a model with them: the model's registers keep their initial values
    own = with4.state_dict()[E + "register_tokens"].clone()
    loaded, skipped_ckpt, skipped_model = init_from_state(with4, {k: v.clone() for k, v in without.state_dict().items()})
    assert skipped_ckpt == [] and skipped_model == [E + "register_tokens"] and len(loaded) == len(without.state_dict())
    assert torch.equal(with4.state_dict()[E + "register_tokens"], own)
    assert "(kept as initialised): ['vit.embeddings.register_tokens']" in capsys.readouterr().out
    # the other way round: the checkpoint's registers are skipped
    loaded, skipped_ckpt, skipped_model = init_from_state(make(0, 3), {k: v.clone() for k, v in with4.state_dict().items()})
    assert skipped_ckpt == [E + "register_tokens"] and skipped_model == []
    assert "not in the model (skipped): ['vit.embeddings.register_tokens']" in capsys.readouterr().out
    # another count: skipped on both sides
    _, skipped_ckpt, skipped_model = init_from_state(make(2, 4), {k: v.clone() for k, v in with4.state_dict().items()})
    assert skipped_ckpt == skipped_model == [E + "register_tokens"]


def test_checkpoint_mismatch_names_both_values():
    import types

    from vit_amd.trainer import check_register_tokens, saved_register_tokens

    ck = lambda **model: {"state_dict": {}, "hyper_parameters": {"config": {"model": model}}}
    assert saved_register_tokens(ck(num_register_tokens=4)) == 4 and saved_register_tokens(ck()) == 0
    assert saved_register_tokens({"state_dict": {}}) is None
    cfg = lambda R: types.SimpleNamespace(num_register_tokens=R)
    check_register_tokens(ck(num_register_tokens=4), cfg(4), "--ckpt")
    check_register_tokens(ck(), cfg(0), "--ckpt")
    check_register_tokens({"state_dict": {}}, cfg(4), "--ckpt")  # a bare state_dict cannot tell
    with pytest.raises(ValueError, match=r"num_register_tokens 4, the config says 0"):
        check_register_tokens(ck(num_register_tokens=4), cfg(0), "--ckpt")
    with pytest.raises(ValueError, match=r"num_register_tokens 0, the config says 2"):
        check_register_tokens(ck(), cfg(2), "test --ckpt")


def test_trainer_refuses_a_checkpoint_of_another_register_count(tmp_path):
    import types

    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT
    from vit_amd.trainer import Trainer

    saved = MyViT(ViTConfig(task_type="reg", num_register_tokens=4, **KW), loss_name="mae")
    path = str(tmp_path / "reg4.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in saved.state_dict().items()},
                "hyper_parameters": {"config": {"model": dict(KW, num_register_tokens=4)}}}, path)
    module = types.SimpleNamespace(model=MyViT(ViTConfig(task_type="reg", num_register_tokens=2, **KW), loss_name="mae"))
    trainer = Trainer.__new__(Trainer)  # the two entry points read the file before they touch any trainer state
    trainer.checkpointer = None
    with pytest.raises(ValueError, match=r"num_register_tokens 4, the config says 2"):
        trainer._resume(module, path)
    with pytest.raises(ValueError, match=r"num_register_tokens 4, the config says 2"):
        trainer.test(module, None, ckpt_path=path)


def test_shipped_config_loads():
    from vit_amd.config import get_vit_config
    from vit_amd.utils import load_config

    root = os.path.dirname(os.path.dirname(__file__))
    c = get_vit_config(load_config(os.path.join(root, "configs", "exp", "registers.yaml")))
    m = get_vit_config(load_config(os.path.join(root, "configs", "exp", "mim_pretrain.yaml")))
    assert c.task_type == "mim" and c.num_register_tokens == 4 and c.seq_len == 201
    for k in ("image_size", "patch_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "stride", "num_patches",
              "mim_mask_ratio", "mim_span", "mim_loss"):
        assert getattr(c, k) == getattr(m, k), k  # mim_pretrain's geometry


def test_exports_and_argument_errors():
    from vit_amd import _cabi
    from vit_amd.build import HEADERS, SOURCES

    assert "registers.hip" in SOURCES and any(h.endswith("vit_amd_registers.h") for h in HEADERS)
    names = _cabi.declared_symbols()
    lib = _cabi.load()
    for name, nargs in (("vit_embed_finish_reg", 15), ("vit_embed_finish_reg_bwd", 18)):
        assert name in names and hasattr(lib, name) and len(_cabi._PROTOS[name]) == nargs, name
    P = 64  # any non-null address: every call below fails its argument check before anything is launched or read
    fwd, bwd = lib.vit_embed_finish_reg, lib.vit_embed_finish_reg_bwd
    for call, text in (
            (lambda: fwd(None, None, P, P, None, None, None, 2, 1, 8, 32, 0.0, 1, 0, None), b"null pointer"),
            (lambda: fwd(None, P, None, P, None, None, None, 2, 1, 8, 32, 0.0, 1, 0, None), b"null pointer"),
            (lambda: fwd(None, P, P, None, None, None, None, 2, 1, 8, 32, 0.0, 1, 0, None), b"null pointer"),  # R > 0 needs reg
            (lambda: fwd(None, P, P, P, None, P, None, 2, 1, 8, 32, 0.0, 1, 0, None), b"mask and mask_token"),
            (lambda: fwd(None, P, P, P, None, None, P, 2, 1, 8, 32, 0.0, 1, 0, None), b"mask and mask_token"),
            (lambda: fwd(None, P, P, P, None, None, None, 0, 1, 8, 32, 0.0, 1, 0, None), b"B=0"),
            (lambda: fwd(None, P, P, P, None, None, None, 2, 1, 0, 32, 0.0, 1, 0, None), b"N=0"),
            (lambda: fwd(None, P, P, P, None, None, None, 2, 1, 8, 0, 0.0, 1, 0, None), b"D=0"),
            (lambda: fwd(None, P, P, P, None, None, None, 2, -1, 8, 32, 0.0, 1, 0, None), b"R=-1"),
            (lambda: fwd(None, P, P, P, None, None, None, 2, 1, 8, 30, 0.0, 1, 0, None), b"D=30"),
            (lambda: fwd(None, P, P, P, None, None, None, 2, 1, 8, 32, 1.0, 1, 0, None), b"dropout_p"),
            (lambda: fwd(None, P, P, P, None, None, None, 2, 1, 8, 32, -0.5, 1, 0, None), b"dropout_p"),
            (lambda: bwd(None, None, None, P, 1, P, P, None, None, 2, 1, 8, 32, 0.0, 1, 0, 0, None), b"null pointer"),
            (lambda: bwd(None, P, None, None, 1, P, P, None, None, 2, 1, 8, 32, 0.0, 1, 0, 0, None), b"null pointer"),
            (lambda: bwd(None, P, None, P, 1, None, P, None, None, 2, 1, 8, 32, 0.0, 1, 0, 0, None), b"null pointer"),
            (lambda: bwd(None, P, None, P, 1, P, None, None, None, 2, 1, 8, 32, 0.0, 1, 0, 0, None), b"null pointer"),
            (lambda: bwd(None, P, P, P, 1, P, P, None, None, 2, 1, 8, 32, 0.0, 1, 0, 0, None), b"mask and dmask_token"),
            (lambda: bwd(None, P, None, P, 1, P, P, None, P, 2, 1, 8, 32, 0.0, 1, 0, 0, None), b"mask and dmask_token"),
            (lambda: bwd(None, P, None, P, 1, P, P, None, None, 2, -2, 8, 32, 0.0, 1, 0, 0, None), b"R=-2"),
            (lambda: bwd(None, P, None, P, 1, P, P, None, None, 2, 1, 8, 34, 0.0, 1, 0, 0, None), b"D=34"),
            (lambda: bwd(None, P, None, P, 1, P, P, None, None, 2, 1, 8, 32, 1.5, 1, 0, 0, None), b"dropout_p"),
            (lambda: bwd(None, P, None, P, 7, P, P, None, None, 2, 1, 8, 32, 0.0, 1, 0, 0, None), b"bad dtype")):
        assert call() == -1
        assert text in lib.vit_last_error(), (text, lib.vit_last_error())
    # calls that pass their checks state their workspace need before anything is launched (no handle: it holds none):
    # min(B, 16) chunks x T x D floats, twice with a mask -- at R = 0 the existing entry points' needs
    WS = _cabi.VIT_ERR_WORKSPACE
    assert bwd(None, P, None, P, 1, P, P, None, None, 32, 3, 8, 32, 0.0, 1, 0, 0, None) == WS
    assert lib.vit_workspace_needed() == 16 * 12 * 32 * 4
    assert bwd(None, P, P, P, 1, P, P, None, P, 33, 3, 8, 32, 0.0, 1, 0, 0, None) == WS
    assert lib.vit_workspace_needed() == 2 * 11 * 12 * 32 * 4  # B = 33: 11 chunks of 3
    assert bwd(None, P, None, P, 1, P, None, None, None, 32, 0, 8, 32, 0.0, 1, 0, 0, None) == WS  # R = 0: no dreg needed
    need = lib.vit_workspace_needed()
    assert lib.vit_embed_finish_bwd(None, P, P, 1, P, None, 32, 9, 32, 0.0, 1, 0, 0, None) == WS
    assert lib.vit_workspace_needed() == need == 16 * 9 * 32 * 4
    assert bwd(None, P, P, P, 1, P, None, None, P, 32, 0, 8, 32, 0.0, 1, 0, 0, None) == WS
    need = lib.vit_workspace_needed()
    assert lib.vit_embed_finish_masked_bwd(None, P, P, P, 1, P, None, P, 32, 9, 32, 0.0, 1, 0, 0, None) == WS
    assert lib.vit_workspace_needed() == need


def test_functional_checks_shapes_and_dtypes():
    import vit_amd.functional as vf
    from vit_amd._cabi import VitError

    B, R, N, D = 2, 2, 3, 8
    tok, cls, reg = torch.zeros(B, 1 + R + N, D), torch.zeros(D), torch.zeros(R, D)
    for kw, text in ((dict(R=-1), "R must be"), (dict(R=True), "R must be"), (dict(R=5), "N >= 1"), (dict(reg=None), "needs the register"),
                     (dict(reg=torch.zeros(R + 1, D)), "must hold"), (dict(cls=torch.zeros(D + 1)), "must hold"),
                     (dict(pos=torch.zeros(1 + R + N, D)), "must hold"), (dict(mask=torch.zeros(B, N, dtype=torch.int32)), "go together"),
                     (dict(tok=tok.double()), "expected torch.float32"), (dict(reg=reg.double()), "expected torch.float32")):
        a = dict(dict(tok=tok, R=R, cls=cls, reg=reg, pos=None, mask=None, mask_token=None), **kw)
        with pytest.raises(VitError, match=text):
            vf.embed_finish_reg(a["tok"], a["R"], a["cls"], a["reg"], a["pos"], a["mask"], a["mask_token"])
    with pytest.raises(VitError, match="dpatch must hold"):
        vf.embed_finish_reg_bwd(tok, R, cls, reg, dpatch=torch.zeros(B * N + 1, D))


# ------------------------------------------------------------------ the host restatement against autograd
@pytest.mark.parametrize("shape", rr.SHAPES[:5] + rr.SHAPES[-1:])
@pytest.mark.parametrize("mask_kind", rr.MASKS)
@pytest.mark.parametrize("with_pos,p", [(False, 0.0), (True, 0.1)])
def test_restatement_is_the_torch_composition(shape, mask_kind, with_pos, p):
    B, R, N, D = shape
    T = 1 + R + N
    g = torch.Generator().manual_seed(100 * B + 10 * R + N + D)
    leaf = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)
    tok, cls, reg, mtok, pos = leaf(B, T, D), leaf(D), leaf(R, D), leaf(D), leaf(1 + N, D)
    mask = rr.make_mask(mask_kind, B, N, 7)
    mult = rr.multiplier(p, 99, 0, B, T, D)
    # the composition a reader would write: cat(CLS, registers, patches-or-mask-token) + pos on CLS and patches, then dropout
    patches = tok[:, 1 + R:] if mask is None else torch.where(mask[:, :, None] != 0, mtok.view(1, 1, D), tok[:, 1 + R:])
    seq = torch.cat([cls.view(1, 1, D).expand(B, 1, D), reg.view(1, R, D).expand(B, R, D), patches], dim=1)
    if with_pos:
        seq = seq + torch.cat([pos[:1], torch.zeros(R, D), pos[1:]], dim=0)
    out = seq if mult is None else seq * mult
    with torch.no_grad():
        mine = rr.embed_fwd(tok, R, cls, reg, pos if with_pos else None, mask, mtok if mask is not None else None, mult)
    assert torch.equal(mine, out.detach())
    dtok = torch.randn(B, T, D, generator=g)
    out.backward(dtok)
    got = rr.embed_bwd(dtok, R, mask, mult, with_pos=with_pos)
    assert torch.equal(got["dpatch"].view(B, N, D), tok.grad[:, 1 + R:])  # masked rows: exact zeros in both
    gd = (dtok if mult is None else dtok * mult).double()
    close = lambda a, b, terms: bool(((a.double() - b.double()).abs() <= rr.sum_bound(B, terms) + 1e-30).all())
    assert close(got["dcls"], cls.grad, gd[:, 0])
    if R > 0:
        assert close(got["dreg"], reg.grad, gd[:, 1:1 + R])
    if with_pos:
        assert close(got["dpos"], pos.grad, torch.cat([gd[:, :1], gd[:, 1 + R:]], dim=1))
    if mask is not None:
        m = (mask != 0)[:, :, None].double()
        assert close(got["dmt"], mtok.grad if mtok.grad is not None else torch.zeros(D), (gd[:, 1 + R:] * m).reshape(B * N, D))
        if mask_kind == "none":
            assert not got["dmt"].any()
    # accumulate: one more f32 add of the old values
    old = dict(dcls=torch.ones(D), dreg=torch.ones(R, D), dpos=torch.ones(1 + N, D), dmt=torch.ones(D))
    acc = rr.embed_bwd(dtok, R, mask, mult, with_pos=with_pos, old=old)
    for k in ("dcls", "dreg", "dpos", "dmt"):
        assert (got[k] is None and acc[k] is None) or torch.equal(acc[k], got[k] + 1.0), k


def test_reduce_rows_orders():
    """Up to 16 rows: the plain ascending sum from +0; beyond: 16 strands with two alternating accumulators; beyond 512: groups
    folded first.  Integer-valued rows make every order exact, so only the wiring is checked here; a row of 2^24 and ones shows
    the order itself."""
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 16, 17, 33, 129, 402, 512, 513, 532, 1100):
        rows = torch.randint(-8, 9, (n, 5), generator=g).float()
        assert torch.equal(rr.reduce_rows(rows), rows.sum(0)), n
    rows = torch.ones(4, 1)
    rows[0, 0] = 2.0 ** 24
    assert float(rr.reduce_rows(rows)[0]) == 2.0 ** 24  # ((2^24 + 1) + 1) + 1 in f32: each add is lost
    assert float(rr.reduce_rows(rows.flip(0))[0]) == 2.0 ** 24 + 4  # ((1 + 1) + 1) + 2^24: 3 + 2^24 rounds to even, up


def test_oracle_wrapper_puts_registers_behind_cls():
    """The wrapped oracle against a transformer written out here for one layer-free model: tokens [CLS, reg, patches], the
    position rows, and that the context manager restores the module."""
    from oracle import refvit

    rc = refvit.RefConfig(image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=0, num_attention_heads=2, stride_size=32,
                          pos_encoding_type="learned", loss_name="mae")
    sd = refvit.make_state_dict(rc, 5)
    R = 3
    sd[rr.REG] = rr.register_values(R, 32, 6)
    flux, _, labels = refvit.make_inputs(rc, 2, 7)
    tokenize, tables = refvit.tokenize, refvit.rope_tables
    out = rr.oracle_forward(rc, sd, flux, labels, R, False, output_hidden_states=True)
    assert refvit.tokenize is tokenize and refvit.rope_tables is tables
    h0 = out.hidden_states[0]
    pos = sd[rr.POS]
    assert h0.shape == (2, 1 + R + 8, 32)
    assert torch.equal(h0[:, 0], (sd["vit.embeddings.cls_token"] + pos[:, :1])[:, 0].expand(2, -1))
    assert torch.equal(h0[:, 1:1 + R], sd[rr.REG].expand(2, -1, -1))  # nothing added to a register
    assert torch.equal(h0[:, 1 + R:], tokenize(rc, sd, flux) + pos[:, 1:])
    assert rr.gathered_rows(6, 2).tolist() == [0, 0, 0, 1, 2, 3]
    cos, _ = tables(8, 6, 100.0)
    with rr.registers(sd, 2):
        cos_r, _ = refvit.rope_tables(8, 6, 100.0)
    assert torch.equal(cos_r, cos[[0, 0, 0, 1, 2, 3]]) and bool((cos_r[:3] == 1).all())  # the identity rotation
