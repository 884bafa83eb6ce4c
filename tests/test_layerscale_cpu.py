"""LayerScale (`model.layer_scale_init`, include/vit_amd_layerscale.h), the part that needs no GPU: the config key, the layout
of the two per-layer lambda parameters, their parameter groups, and the new entry points' argument errors."""
import ctypes
import math

import pytest
import torch

KW = dict(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
          stride_size=32)
MODEL = dict(task_type="reg", image_size=256, patch_size=32, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
             proj_fn="SW", stride_size=32)


def models():
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    return MyViT(ViTConfig(**KW), loss_name="mae"), MyViT(ViTConfig(**KW, layer_scale_init=1e-4), loss_name="mae")


def lambda_names(L=3):
    return [f"vit.encoder.layer.{i}.layer_scale{s}.lambda1" for i in range(L) for s in (1, 2)]


def test_config_key_is_validated_at_construction():
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    assert ViTConfig(**KW).layer_scale_init is None
    for ok in (1e-6, 1e-4, 1, 1.0, 2.5):
        assert MyViT(ViTConfig(**KW, layer_scale_init=ok), loss_name="mae").engine.layer_scale
    for bad in (0, 0.0, -1e-4, float("nan"), float("inf"), -float("inf"), "1e-4", "x", True, [1.0]):
        with pytest.raises(ValueError, match="layer_scale_init"):
            MyViT(ViTConfig(**KW, layer_scale_init=bad), loss_name="mae")


def test_get_vit_config_passes_the_key_through_and_is_unchanged_without_it():
    from vit_amd.config import ViTConfig, get_vit_config

    without = get_vit_config(dict(model=dict(MODEL)))
    assert without.layer_scale_init is None
    assert get_vit_config(dict(model=dict(MODEL, layer_scale_init=1.0e-5))).layer_scale_init == 1.0e-5
    assert get_vit_config(dict(model=dict(MODEL, layer_scale_init=None))).layer_scale_init is None
    with_key = get_vit_config(dict(model=dict(MODEL, layer_scale_init=0.1)))
    for f in ViTConfig.__dataclass_fields__:
        if f != "layer_scale_init":
            assert getattr(with_key, f) == getattr(without, f), f


def test_layout_names_shapes_order_and_ranges():
    from vit_amd.engine import ALIGN

    plain, scaled = models()
    a, b = plain.engine.layout, scaled.engine.layout
    D, L = KW["hidden_size"], KW["num_hidden_layers"]
    names = lambda_names(L)
    assert not [n for n in a.entries if "lambda1" in n] and list(plain.state_dict()) == a.state_order
    assert [n for n in b.entries if "lambda1" in n] == names
    assert [n for n in b.state_order if n not in names] == a.state_order  # nothing else moved
    assert list(scaled.state_dict()) == b.state_order == [n for n, _ in scaled.named_parameters()]
    for i in range(L):
        lo, hi = b.layer_ranges[i]
        pre = f"vit.encoder.layer.{i}."
        block = [n for n in b.state_order if n.startswith(pre)]
        assert block[-2:] == names[2 * i:2 * i + 2]  # at the end of the layer's block
        after = b.entries[pre + "layernorm_after.bias"][0]
        for n in names[2 * i:2 * i + 2]:
            off, shape = b.entries[n]
            assert shape == (D,) and lo <= after < off and off + D <= hi and off % ALIGN == 0, n
        assert hi - lo == (a.layer_ranges[i][1] - a.layer_ranges[i][0]) + 2 * (-(-D // ALIGN) * ALIGN)
    pad = -(-D // ALIGN) * ALIGN
    assert b.n_trainable == a.n_trainable + 2 * L * pad and b.n_total == a.n_total + 2 * L * pad
    assert b.buckets()[1:-1] == list(reversed(b.layer_ranges))
    for n in names:
        assert torch.equal(scaled.state_dict()[n], torch.full((D,), 1e-4)), n  # init_weights fills them
    # everything else initialises as in the plain model's rules
    assert float(scaled.state_dict()["vit.encoder.layer.0.layernorm_after.weight"].min()) == 1.0
    assert float(scaled.state_dict()["vit.encoder.layer.0.output.dense.bias"].abs().max()) == 0.0


def test_strict_loading_across_the_feature_fails_both_ways():
    plain, scaled = models()
    with pytest.raises(RuntimeError, match="lambda1"):
        scaled.load_state_dict(plain.state_dict(), strict=True)
    with pytest.raises(RuntimeError, match="lambda1"):
        plain.load_state_dict(scaled.state_dict(), strict=True)
    assert sorted(scaled.load_state_dict(plain.state_dict(), strict=False).missing_keys) == sorted(lambda_names())


def test_param_groups_no_decay_and_layer_decay():
    from vit_amd.optimizer import build_param_groups

    _, scaled = models()
    by_id = {id(p): n for n, p in scaled.named_parameters()}
    L = KW["num_hidden_layers"]
    groups = build_param_groups(scaled, lr=1e-3, weight_decay=0.05, no_decay=True)
    found = {by_id[id(p)]: g for g in groups for p in g["params"]}
    for n in lambda_names(L):
        assert found[n]["weight_decay"] == 0.0, n
    assert found["vit.encoder.layer.0.output.dense.weight"]["weight_decay"] == 0.05
    groups = build_param_groups(scaled, lr=1e-3, weight_decay=0.05, layer_decay=0.5)
    found = {by_id[id(p)]: g for g in groups for p in g["params"]}
    for i in range(L):
        for s in (1, 2):
            n = f"vit.encoder.layer.{i}.layer_scale{s}.lambda1"
            assert found[n]["lr"] == found[f"vit.encoder.layer.{i}.output.dense.weight"]["lr"], n
            assert math.isclose(found[n]["lr"], 1e-3 * 0.5 ** (L + 1 - (i + 1))), n
    lrs = {found[f"vit.encoder.layer.{i}.layer_scale1.lambda1"]["lr"] for i in range(L)}
    assert len(lrs) == L


def test_symbols_exist_and_argument_errors_are_reported_without_a_gpu():
    from vit_amd import _cabi

    lib = _cabi.load()
    for sym in ("vit_layer_scale_table_write", "vit_layer_scale_fold", "vit_layer_scale_grad"):
        assert hasattr(lib, sym) and sym in _cabi._PROTOS and sym in _cabi.declared_symbols(), sym
    assert ctypes.sizeof(_cabi.LayerScaleEntry) == 96

    def err():
        return lib.vit_last_error().decode()

    table = 4096  # any non-null, 16-byte aligned address: every check comes before the first launch
    assert lib.vit_layer_scale_fold(None, None, 1, 1, _cabi.VIT_BF16, None) == -1 and "null pointer" in err()
    assert lib.vit_layer_scale_fold(None, table + 4, 1, 1, _cabi.VIT_BF16, None) == -1 and "16-byte aligned" in err()
    assert lib.vit_layer_scale_fold(None, table, 0, 1, _cabi.VIT_BF16, None) == -1 and "n_entries" in err()
    assert lib.vit_layer_scale_fold(None, table, 1, 0, _cabi.VIT_BF16, None) == -1 and "max_rows" in err()
    assert lib.vit_layer_scale_fold(None, table, 1, 1, 7, None) == -1 and "out_dtype" in err()
    assert lib.vit_layer_scale_grad(None, None, 1, 1, 0, None) == -1 and "null pointer" in err()
    assert lib.vit_layer_scale_grad(None, table, 1, 0, 0, None) == -1 and "max_rows" in err()
    assert lib.vit_layer_scale_grad(None, table, 1, 1, 2, None) == -1 and "accumulate" in err()

    def entry(**kw):
        e = (_cabi.LayerScaleEntry * 1)()
        base = dict(W=4096, b=4096, lam=4096, Wf=4096, bf=4096, dW_raw=4096, db_raw=4096, dW=4096, db=4096, dlam=4096,
                    rows=4, cols=8)
        base.update(kw)
        for k, v in base.items():
            setattr(e[0], k, v)
        return e

    write = lib.vit_layer_scale_table_write
    assert write(None, None, entry(), 1, None) == -1 and "null pointer" in err()
    assert write(None, table, None, 1, None) == -1 and "null pointer" in err()
    assert write(None, table, entry(), 0, None) == -1 and "count" in err()
    for field in ("W", "b", "lam"):
        assert write(None, table, entry(**{field: None}), 1, None) == -1 and "null pointer (W, b, lambda)" in err(), field
    for field in ("bf", "dW_raw", "db", "dlam"):  # half an output set
        assert write(None, table, entry(**{field: None}), 1, None) == -1 and "output set" in err(), field
    none = dict(Wf=None, bf=None, dW_raw=None, db_raw=None, dW=None, db=None, dlam=None)
    assert write(None, table, entry(**none), 1, None) == -1 and "output set" in err()
    assert write(None, table, entry(rows=0), 1, None) == -1 and "rows = 0" in err()
    assert write(None, table, entry(cols=0), 1, None) == -1 and "cols = 0" in err()
    assert write(None, table, entry(cols=6), 1, None) == -1 and "multiple of 4" in err()
    assert write(None, table, entry(W=4100), 1, None) == -1 and "16-byte aligned" in err()
