"""CPU suite of the fused optimizers' parameter groups: the grouped C entry points refuse bad arguments before a launch, the
table builder accepts a partition and refuses a malformed one, `opt.no_decay` / `opt.layer_decay` build the documented groups
(name by name at C1) for the fused classes and for torch's, and a multi-group state_dict is torch's own format."""
import copy

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from vit_amd import _cabi
    from vit_amd import build as vb

    vb.build(force=False, verbose=False)
    return _cabi.load()


P = 0x1000  # a non-null "device pointer": every call below must fail its argument check before it could be used
NEW = ["vit_adamw_step_groups", "vit_adamw_step_groups_dyn", "vit_adam_l2_step_groups", "vit_adam_l2_step_groups_dyn",
       "vit_sgd_step_groups", "vit_sgd_step_groups_dyn", "vit_optim_groups_write"]


def _err(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.vit_last_error().decode()
    for n in needles:
        assert n in msg, msg


def test_new_symbols_are_declared_bound_and_exported(lib):
    from vit_amd import _cabi

    for name in NEW:
        assert name in _cabi._PROTOS and name in _cabi.declared_symbols() and hasattr(lib, name), name
    # the grouped forms take the plain ones' arguments with (base, seg_end, seg_group, n_segments, groups, n_groups) in place
    # of the scalars the group table now carries: lr + weight_decay (Adam), lr + momentum + weight_decay (SGD)
    assert len(_cabi._PROTOS["vit_adamw_step_groups"]) == len(_cabi._PROTOS["vit_adamw_step"]) + 6 - 2
    assert len(_cabi._PROTOS["vit_sgd_step_groups"]) == len(_cabi._PROTOS["vit_sgd_step"]) + 6 - 3


def test_grouped_adam_argument_errors(lib):
    for name in ("vit_adamw_step_groups", "vit_adam_l2_step_groups"):
        fn = getattr(lib, name)

        def call(p=P, g=P, m=P, v=P, n=8, base=0, se=P, sg=P, ns=1, gr=P, ng=1, step=1):
            return fn(None, p, g, m, v, None, n, base, se, sg, ns, gr, ng, 0.9, 0.999, 1e-8, step, None, 0.0, None)

        for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(step=0)):
            _err(lib, call(**kw), name, "bad arguments")
        for kw in (dict(se=None), dict(sg=None), dict(gr=None)):
            _err(lib, call(**kw), name, "null table")
        _err(lib, call(n=0), name, "n = 0")
        _err(lib, call(n=-4), name, "n = -4")
        _err(lib, call(ns=0), name, "n_segments = 0")
        _err(lib, call(ng=0), name, "n_groups = 0")
        _err(lib, call(base=-4), name, "base = -4")
        _err(lib, call(base=6), name, "base = 6")  # a 16-byte vector would straddle a boundary


def test_grouped_sgd_argument_errors(lib):
    def call(p=P, g=P, buf=None, n=8, base=0, se=P, sg=P, ns=1, gr=P, ng=1, nesterov=0):
        return lib.vit_sgd_step_groups(None, p, g, buf, None, n, base, se, sg, ns, gr, ng, nesterov, None, 0.0, None)

    _err(lib, call(p=None), "vit_sgd_step_groups", "null")
    _err(lib, call(g=None), "vit_sgd_step_groups", "null")
    _err(lib, call(se=None), "null table")
    _err(lib, call(n=0), "n = 0")
    _err(lib, call(ns=-1), "n_segments = -1")
    _err(lib, call(ng=0), "n_groups = 0")
    _err(lib, call(base=-8), "base = -8")
    _err(lib, call(nesterov=1), "nesterov")  # no buffer


def test_grouped_dyn_forms_need_a_bound_record_and_the_writer_its_pointers(lib):
    import ctypes as C

    tables = (8, 0, P, P, 1, P, 1)
    for name in ("vit_adamw_step_groups_dyn", "vit_adam_l2_step_groups_dyn"):
        _err(lib, getattr(lib, name)(None, P, P, P, P, None, *tables, 0.9, 0.999, 1e-8, None, 0.0, None), name,
             "no step state bound")
    _err(lib, lib.vit_sgd_step_groups_dyn(None, P, P, P, None, *tables, 0, None, 0.0, None), "vit_sgd_step_groups_dyn",
         "no step state bound")
    vals = (C.c_float * 3)(1e-3, 0.0, 0.0)
    _err(lib, lib.vit_optim_groups_write(None, None, 1, vals, None), "vit_optim_groups_write", "null")
    _err(lib, lib.vit_optim_groups_write(None, P, 1, None, None), "vit_optim_groups_write", "null")
    _err(lib, lib.vit_optim_groups_write(None, P, 0, vals, None), "n_groups = 0")


# ------------------------------------------------------------------------------------------------------------ table builder
def test_table_builder_accepts_a_partition_and_merges_neighbours():
    import vit_amd.functional as vf

    t = vf.optim_group_tables([(0, 8, 0), (8, 256, 1), (264, 8, 1), (272, 760, 0)], 2, "cpu")
    assert t.seg_end.tolist() == [8, 272, 1032] and t.seg_group.tolist() == [0, 1, 0]
    assert t.seg_end.dtype == torch.int64 and t.seg_group.dtype == torch.int32
    assert t.groups.shape == (2, 4) and t.groups.dtype == torch.float32 and (t.n_segments, t.n_groups) == (3, 2)
    # a gap (parameters no group owns) falls to the segment behind it; the last end may be the buffer's odd length
    t = vf.optim_group_tables([(8, 8, 1), (1024, 3, 0)], 2, "cpu", total=1027)
    assert t.seg_end.tolist() == [16, 1027] and t.seg_group.tolist() == [1, 0]


@pytest.mark.parametrize("triples,total,needle", [
    ([(8, 8, 0), (0, 8, 1)], None, "sorted"),            # unsorted
    ([(0, 16, 0), (8, 8, 1)], None, "overlap"),          # overlapping
    ([(0, 8, 0), (10, 6, 1)], None, "aligned"),          # misaligned offset
    ([(0, 6, 0), (8, 8, 1)], None, "aligned"),           # misaligned end that is not the last
    ([(0, 8, 0), (8, 7, 1)], 16, "aligned"),             # odd last end that is not the buffer's length
    ([(0, 8, 0), (8, 8, 2)], None, "group 2"),           # group index out of range
    ([(0, 8, -1)], None, "group -1"),
    ([(0, 0, 0)], None, "empty"),
    ([], None, "at least one"),
])
def test_table_builder_refuses_a_malformed_partition(triples, total, needle):
    import vit_amd.functional as vf

    with pytest.raises(ValueError, match=needle):
        vf.optim_group_tables(triples, 2, "cpu", total=total)


# ------------------------------------------------------------------------------------------------------------------ factory
def _c1(pos=None, proj_fn="C1D"):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    cfg = ViTConfig(task_type="reg", image_size=4096, patch_size=32, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
                    stride_size=32, num_labels=1, proj_fn=proj_fn, pos_encoding_type=pos)
    return MyViT(cfg, loss_name="mae")


@pytest.fixture(scope="module")
def vit():
    return _c1()


def _opt(conf):
    return conf["optimizer"] if isinstance(conf, dict) else conf


def _names(model, group):
    by_id = {id(p): n for n, p in model.named_parameters()}
    return [by_id[id(p)] for p in group["params"]]


def _no_decay_rule(model):
    """The issue's rule, restated: at most one dimension, or the class token, or the position embeddings."""
    return {n for n, p in model.named_parameters()
            if p.ndim <= 1 or n in ("vit.embeddings.cls_token", "vit.embeddings.position_embeddings")}


def _assert_partition(model, opt):
    seen = [id(p) for g in opt.param_groups for p in g["params"]]
    assert len(seen) == len(set(seen)) and set(seen) == {id(p) for p in model.parameters()}


def test_neither_key_gives_one_group_with_todays_keys(vit):
    from vit_amd.optimizer import FusedAdamW, OptModule

    for conf in ({"type": "AdamW", "weight_decay": 0.05}, {"type": "AdamW", "weight_decay": 0.05, "no_decay": False,
                                                           "layer_decay": None}):
        opt = _opt(OptModule.from_config(conf)(vit))
        assert type(opt) is FusedAdamW and len(opt.param_groups) == 1
        assert set(opt.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay"}
        assert len(opt.param_groups[0]["params"]) == len(list(vit.parameters()))


@pytest.mark.parametrize("pos", [None, "learned"])
def test_no_decay_membership_name_by_name(pos):
    from vit_amd.optimizer import FusedAdamW, OptModule

    model = _c1(pos)
    opt = _opt(OptModule.from_config({"type": "AdamW", "lr": 1e-3, "weight_decay": 0.05, "no_decay": True})(model))
    assert type(opt) is FusedAdamW and len(opt.param_groups) == 2
    decay, skip = opt.param_groups
    assert (decay["weight_decay"], skip["weight_decay"]) == (0.05, 0.0) and decay["lr"] == skip["lr"] == 1e-3
    assert set(_names(model, skip)) == _no_decay_rule(model)
    _assert_partition(model, opt)
    # spelled out: the Conv1D patch weight [D, 1, P] decays, the class token [1, 1, D] does not
    w = "vit.embeddings.patch_embeddings.projection.weight"
    assert dict(model.named_parameters())[w].ndim == 3 and w in _names(model, decay)
    layer = "vit.encoder.layer.1."
    expect_skip = {"vit.embeddings.cls_token", "vit.embeddings.patch_embeddings.projection.bias", "vit.layernorm.weight",
                   "vit.layernorm.bias", "regressor.bias", layer + "layernorm_before.weight", layer + "layernorm_after.bias",
                   layer + "attention.attention.query.bias", layer + "output.dense.bias"}
    expect_decay = {"regressor.weight", layer + "attention.attention.key.weight", layer + "intermediate.dense.weight"}
    if pos == "learned":
        expect_skip.add("vit.embeddings.position_embeddings")
    else:
        assert "vit.embeddings.position_embeddings" not in dict(model.named_parameters())
    assert expect_skip <= set(_names(model, skip)) and expect_decay <= set(_names(model, decay))


def test_no_decay_takes_a_list_of_name_patterns(vit):
    from vit_amd.optimizer import OptModule

    opt = _opt(OptModule.from_config({"type": "AdamW", "weight_decay": 0.05, "no_decay": ["*.bias", "vit.layernorm.*"]})(vit))
    decay, skip = opt.param_groups
    want = {n for n, _ in vit.named_parameters() if n.endswith(".bias") or n.startswith("vit.layernorm.")}
    assert set(_names(vit, skip)) == want and skip["weight_decay"] == 0.0 and decay["weight_decay"] == 0.05
    _assert_partition(vit, opt)


def test_layer_decay_gives_the_five_rates(vit):
    from vit_amd.optimizer import OptModule

    lr, f = 1e-3, 0.75
    opt = _opt(OptModule.from_config({"type": "AdamW", "lr": lr, "weight_decay": 0.05, "layer_decay": f})(vit))
    assert [g["lr"] for g in opt.param_groups] == [lr * f ** k for k in (4, 3, 2, 1, 0)]  # L = 3: ids 0 .. 4
    assert all(g["weight_decay"] == 0.05 for g in opt.param_groups)
    assert all(n.startswith("vit.embeddings.") for n in _names(vit, opt.param_groups[0]))
    for i in range(3):
        assert all(n.startswith(f"vit.encoder.layer.{i}.") for n in _names(vit, opt.param_groups[i + 1]))
    assert set(_names(vit, opt.param_groups[4])) == {"vit.layernorm.weight", "vit.layernorm.bias", "vit.pooler.dense.weight",
                                                     "vit.pooler.dense.bias", "regressor.weight", "regressor.bias"}
    _assert_partition(vit, opt)


def test_both_keys_give_the_product_of_groups(vit):
    from vit_amd.optimizer import OptModule

    lr, f = 1e-3, 0.75
    opt = _opt(OptModule.from_config({"type": "AdamW", "lr": lr, "weight_decay": 0.05, "no_decay": True,
                                      "layer_decay": f})(vit))
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == \
           [(lr * f ** k, wd) for k in (4, 3, 2, 1, 0) for wd in (0.05, 0.0)]
    rule = _no_decay_rule(vit)
    for g in opt.param_groups:
        assert all((n in rule) == (g["weight_decay"] == 0.0) for n in _names(vit, g))
    _assert_partition(vit, opt)


def test_a_preprocessor_keeps_lr_under_layer_decay():
    from vit_amd.optimizer import build_param_groups

    class WithPre(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.preprocessor = torch.nn.Linear(4, 4)
            self.vit = torch.nn.ModuleDict({"encoder": torch.nn.ModuleDict({"layer": torch.nn.ModuleList(
                [torch.nn.Linear(4, 4), torch.nn.Linear(4, 4)])})})

    model = WithPre()
    groups = build_param_groups(model, 1e-2, 0.1, layer_decay=0.5)
    by_id = {id(p): n for n, p in model.named_parameters()}
    rates = {by_id[id(p)]: g["lr"] for g in groups for p in g["params"]}
    assert rates["preprocessor.weight"] == 1e-2 and rates["vit.encoder.layer.1.weight"] == 1e-2 * 0.5
    assert rates["vit.encoder.layer.0.bias"] == 1e-2 * 0.5 ** 2


def test_the_same_groups_reach_torch_optimizers(vit):
    from vit_amd.optimizer import OptModule

    conf = {"lr": 1e-3, "weight_decay": 0.05, "no_decay": True, "layer_decay": 0.75}
    fused = _opt(OptModule.from_config(dict(conf, type="AdamW"))(vit))
    rms = _opt(OptModule.from_config(dict(conf, type="RMSprop"))(vit))
    assert type(rms) is torch.optim.RMSprop and len(rms.param_groups) == len(fused.param_groups) == 10
    for a, b in zip(fused.param_groups, rms.param_groups):
        assert [id(p) for p in a["params"]] == [id(p) for p in b["params"]]
        assert (a["lr"], a["weight_decay"]) == (b["lr"], b["weight_decay"])
    lin = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3))  # not a MyViT
    sgd = _opt(OptModule.from_config({"type": "SGD", "lr": 1e-2, "weight_decay": 0.1, "no_decay": True})(lin))
    assert type(sgd) is torch.optim.SGD and [g["weight_decay"] for g in sgd.param_groups] == [0.1, 0.0]
    assert [tuple(p.shape) for p in sgd.param_groups[0]["params"]] == [(3, 4)]
    assert len(sgd.param_groups[1]["params"]) == 3
    assert type(_opt(OptModule.from_config({"type": "SGD"})(lin))) is torch.optim.SGD  # neither key: as before
    assert len(_opt(OptModule.from_config({"type": "SGD"})(lin)).param_groups) == 1


def test_one_cycle_receives_the_list_of_rates(vit):
    from vit_amd.optimizer import OptModule

    lr, f = 1e-3, 0.75
    conf = OptModule.from_config({"type": "AdamW", "lr": lr, "layer_decay": f, "lr_sch": "onecycle", "steps_per_epoch": 4,
                                  "epochs": 2})(vit)
    groups = conf["optimizer"].param_groups
    assert [g["max_lr"] for g in groups] == [lr * f ** k for k in (4, 3, 2, 1, 0)]  # a scalar max_lr would flatten them
    assert [g["lr"] for g in groups] == pytest.approx([lr * f ** k / 25 for k in (4, 3, 2, 1, 0)])
    assert conf["lr_scheduler"]["interval"] == "step"


# ------------------------------------------------------------------------------------------------------- the fused classes
def test_groups_by_name_at_construction_and_by_add_param_group(vit):
    from vit_amd.optimizer import FusedAdamW

    names = [n for n, _ in vit.named_parameters()]
    biases = [n for n in names if n.endswith(".bias")]
    rest = [p for n, p in vit.named_parameters() if not n.endswith(".bias")]
    opt = FusedAdamW(vit, lr=1e-3, weight_decay=0.05, param_groups=[{"params": rest}, {"params": biases, "weight_decay": 0.0,
                                                                                      "lr": 5e-4}])
    assert [(g["lr"], g["weight_decay"], g["betas"]) for g in opt.param_groups] == \
           [(1e-3, 0.05, (0.9, 0.999)), (5e-4, 0.0, (0.9, 0.999))]  # omitted keys take the defaults
    assert _names(vit, opt.param_groups[1]) == biases
    with pytest.raises(ValueError, match="does not have"):
        FusedAdamW(vit, param_groups=[{"params": ["no.such.parameter"]}])
    part = FusedAdamW(vit, lr=1e-3, param_groups=[{"params": rest}])
    assert len(part._group_index) == len(rest)
    part.add_param_group({"params": [dict(vit.named_parameters())[n] for n in biases], "weight_decay": 0.0})
    assert len(part.param_groups) == 2 and len(part._group_index) == len(names)
    assert part._graph_signature() == opt._graph_signature() != None  # noqa: E711  (the partition is part of a capture)


def test_one_group_capture_signature_is_the_partition(vit):
    """A capture of a one-group optimizer pins the partition like any other: it holds the segment table's address."""
    from vit_amd.optimizer import FusedAdamW, FusedSGD

    rest = [p for n, p in vit.named_parameters() if not n.endswith(".bias")]
    biases = [p for n, p in vit.named_parameters() if n.endswith(".bias")]
    opt = FusedAdamW(vit, lr=1e-3, param_groups=[{"params": rest}])
    old = opt._graph_signature()
    assert len(opt.param_groups) == 1 and old == opt._partition_signature() == (tuple(id(p) for p in rest),)
    opt._graph_validate(old)
    opt.add_param_group({"params": biases, "weight_decay": 0.0})
    with pytest.raises(ValueError, match="repartitioned"):
        opt._graph_validate(old)
    sgd = FusedSGD(vit, lr=1e-2)
    old = sgd._graph_signature()
    assert len(sgd.param_groups) == 1 and old == (False, sgd._partition_signature())
    sgd._graph_validate(old)
    moved = sgd.param_groups[0]["params"].pop()
    sgd.add_param_group({"params": [moved]})
    with pytest.raises(ValueError, match="repartitioned"):
        sgd._graph_validate(old)


def test_groups_that_disagree_on_what_the_kernel_shares_raise(vit):
    from vit_amd.optimizer import FusedAdamW, FusedSGD

    w = [p for p in vit.parameters() if p.ndim > 1]
    b = [p for p in vit.parameters() if p.ndim <= 1]
    opt = FusedAdamW(vit, param_groups=[{"params": w}, {"params": b, "betas": (0.9, 0.95)}])
    with pytest.raises(ValueError, match="betas"):
        opt._check_shared()
    with pytest.raises(ValueError, match="eps"):
        FusedAdamW(vit, param_groups=[{"params": w}, {"params": b, "eps": 1e-6}])._check_shared()
    with pytest.raises(ValueError, match="nesterov"):
        FusedSGD(vit, momentum=0.9, param_groups=[{"params": w}, {"params": b, "nesterov": True}])._check_shared()
    sgd = FusedSGD(vit, momentum=0.9, param_groups=[{"params": w}, {"params": b, "dampening": 0.5}])
    with pytest.raises(ValueError, match="dampening"):
        sgd._check_shared()
    FusedAdamW(vit, param_groups=[{"params": w}, {"params": b, "betas": [0.9, 0.999]}])._check_shared()  # agree


@pytest.mark.parametrize("kind", ["adamw", "adam", "sgd"])
def test_multi_group_state_dict_is_torchs_format(vit, kind):
    """A format check (no step): the fused optimizer's state_dict loads into the torch class built with the same groups, the
    torch one -- with state -- loads back, and what the fused optimizer then reports is that state, tensor for tensor."""
    from vit_amd.optimizer import FusedAdamW, FusedSGD, build_param_groups

    def groups():
        return build_param_groups(vit, 1e-3, 0.05, no_decay=True, layer_decay=0.75)

    if kind == "sgd":
        fused, ref = FusedSGD(vit, lr=1e-3, momentum=0.9, param_groups=groups()), torch.optim.SGD(groups(), lr=1e-3, momentum=0.9)
        keys = ("momentum_buffer",)
    else:
        fused = FusedAdamW(vit, lr=1e-3, adam_l2=(kind == "adam"), param_groups=groups())
        ref = (torch.optim.Adam if kind == "adam" else torch.optim.AdamW)(groups(), lr=1e-3)
        keys = ("exp_avg", "exp_avg_sq")
    sd = fused.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in ref.state_dict()["param_groups"]]
    ref.load_state_dict(copy.deepcopy(sd))
    assert [(g["lr"], g["weight_decay"]) for g in ref.param_groups] == [(g["lr"], g["weight_decay"]) for g in fused.param_groups]
    # give torch a state (what a step would have left) and carry it back
    gen = torch.Generator().manual_seed(0)
    for p in (p for g in ref.param_groups for p in g["params"]):
        ref.state[p] = {k: torch.rand(p.shape, generator=gen) for k in keys}
        if kind != "sgd":
            ref.state[p]["step"] = torch.tensor(3.0)
    ref.param_groups[3]["lr"] = 7e-4
    back = ref.state_dict()
    fused.load_state_dict(copy.deepcopy(back))
    assert fused.param_groups[3]["lr"] == 7e-4
    again = fused.state_dict()
    lay = vit.engine.layout
    stepped = [i for i, p in enumerate(p for g in fused.param_groups for p in g["params"])
               if not any(p is q for q in (dict(vit.named_parameters())[n] for n in ("vit.pooler.dense.weight",
                                                                                     "vit.pooler.dense.bias")))]
    assert sorted(again["state"]) == stepped and len(stepped) == len(lay.entries) - 2
    for i in stepped:
        for k in keys:
            assert torch.equal(again["state"][i][k], back["state"][i][k]), (i, k)
    if kind != "sgd":
        assert fused._step == 3
