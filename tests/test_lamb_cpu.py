"""Fused LAMB, the parts that need no GPU: the factory (`opt.type: lamb`), the per-parameter table builder, what FusedLamb
refuses, and the argument checks of vit_lamb_step / _groups / _groups_dyn (every one fails before anything could be launched)."""
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from vit_amd import _cabi
    from vit_amd import build as vb

    vb.build(force=False, verbose=False)
    return _cabi.load()


P = 0x1000  # a non-null "device pointer": every call below must fail its argument check before it could be used
NEW = ["vit_lamb_step", "vit_lamb_step_groups", "vit_lamb_step_groups_dyn"]


def _err(lib, rc, *needles):
    assert rc == -1, rc
    msg = lib.vit_last_error().decode()
    for n in needles:
        assert n in msg, msg


@pytest.fixture(scope="module")
def vit():
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    cfg = ViTConfig(task_type="reg", image_size=4096, patch_size=32, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
                    stride_size=32, num_labels=1, proj_fn="C1D")
    return MyViT(cfg, loss_name="mae")


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_the_library_exports_what_cabi_declares(lib):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    for name in NEW:
        assert name in _cabi._PROTOS and name in _cabi.declared_symbols() and hasattr(lib, name), name
    assert [s for s in _cabi.declared_symbols() if not hasattr(lib, s)] == []
    # by value: AdamW's arguments + always_adapt, trust_clip, trust; the table forms trade lr and weight_decay for the six table arguments
    assert len(_cabi._PROTOS["vit_lamb_step"]) == len(_cabi._PROTOS["vit_adamw_step"]) + 3
    assert len(_cabi._PROTOS["vit_lamb_step_groups"]) == len(_cabi._PROTOS["vit_lamb_step"]) + 6 - 2
    assert len(_cabi._PROTOS["vit_lamb_step_groups_dyn"]) == len(_cabi._PROTOS["vit_lamb_step_groups"]) - 1
    header = open(_cabi.HEADER_PATH.replace("vit_amd.h", "vit_amd_optim.h")).read()
    assert f"#define VIT_LAMB_TILE {vf.LAMB_TILE} " in header


def test_by_value_argument_errors(lib):
    def call(p=P, g=P, m=P, v=P, n=8, step=1):
        return lib.vit_lamb_step(None, p, g, m, v, None, n, 1e-3, 0.9, 0.999, 1e-6, 0.0, 0, 0, step, None, 0.0, None, None)

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-8), dict(step=0)):
        _err(lib, call(**kw), "vit_lamb_step", "bad arguments")


def test_table_argument_errors(lib):
    def call(p=P, g=P, m=P, v=P, n=8, base=0, se=P, sg=P, ns=1, gr=P, ng=1, step=1, trust=P):
        return lib.vit_lamb_step_groups(None, p, g, m, v, None, n, base, se, sg, ns, gr, ng, 0.9, 0.999, 1e-6, 0, 0, step, None,
                                        0.0, trust, None)

    name = "vit_lamb_step_groups"
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(step=0)):
        _err(lib, call(**kw), name, "bad arguments")
    for kw in (dict(se=None), dict(sg=None), dict(gr=None)):
        _err(lib, call(**kw), name, "null table")
    _err(lib, call(trust=None), name, "null trust")
    _err(lib, call(n=0), name, "n = 0")
    _err(lib, call(n=-4), name, "n = -4")
    _err(lib, call(ns=0), name, "n_segments = 0")
    _err(lib, call(ng=0), name, "n_groups = 0")
    _err(lib, call(base=-4), name, "base = -4")
    _err(lib, call(base=6), name, "base = 6")


def test_the_dyn_form_needs_a_bound_record(lib):
    rc = lib.vit_lamb_step_groups_dyn(None, P, P, P, P, None, 8, 0, P, P, 1, P, 1, 0.9, 0.999, 1e-6, 0, 0, None, 0.0, P, None)
    _err(lib, rc, "vit_lamb_step_groups_dyn", "no step state bound")


# ------------------------------------------------------------------------------------------------------------ table builder
def test_param_tables_do_not_merge_and_keep_gaps_apart():
    import vit_amd.functional as vf

    # neighbours of one group stay two segments; the pad behind a tensor (its numel rounded up) is the tensor's
    t = vf.optim_param_tables([(0, 8, 0), (8, 256, 1), (264, 8, 1), (272, 760, 0)], 2, "cpu")
    assert isinstance(t, vf.GroupTables) and t.seg_end.tolist() == [8, 264, 272, 1032] and t.seg_group.tolist() == [0, 1, 1, 0]
    assert t.seg_end.dtype == torch.int64 and t.seg_group.dtype == torch.int32 and (t.n_segments, t.n_groups) == (4, 2)
    assert t.starts == [0, 8, 264, 272] and t.segment_of == [0, 1, 2, 3]
    merged = vf.optim_group_tables([(0, 8, 0), (8, 256, 1), (264, 8, 1), (272, 760, 0)], 2, "cpu")
    assert merged.seg_end.tolist() == [8, 272, 1032]  # the existing builder is as it was
    # a gap -- in front, or between two tensors -- is a segment of its own that no group owns: it enters nobody's norm
    t = vf.optim_param_tables([(8, 8, 1), (1024, 3, 0)], 2, "cpu", total=1027)
    assert t.seg_end.tolist() == [8, 16, 1024, 1027] and t.seg_group.tolist() == [-1, 1, -1, 0] and t.segment_of == [1, 3]
    # whole segments only
    t.check_run(8, 8)
    t.check_run(0, 1027)
    t.check_run(1024, 3)
    for base, n in ((8, 4), (12, 4), (8, 1000), (1020, 7), (8, 0)):
        with pytest.raises(ValueError, match="cuts a parameter tensor"):
            t.check_run(base, n)


@pytest.mark.parametrize("triples,total,needle", [
    ([(8, 8, 0), (0, 8, 1)], None, "sorted"), ([(0, 16, 0), (8, 8, 1)], None, "overlap"), ([(0, 8, 0), (10, 6, 1)], None, "aligned"),
    ([(0, 8, 0), (8, 7, 1)], 16, "aligned"), ([(0, 8, 0), (8, 8, 2)], None, "group 2"), ([(0, 0, 0)], None, "empty"),
    ([], None, "at least one"),
])
def test_param_tables_refuse_what_the_group_tables_refuse(triples, total, needle):
    import vit_amd.functional as vf

    with pytest.raises(ValueError, match=needle):
        vf.optim_param_tables(triples, 2, "cpu", total=total)


def test_the_table_call_refuses_merged_tables_and_cut_runs():
    """Refused where the host builds the call, before a handle or the GPU is asked for anything."""
    import vit_amd.functional as vf

    buf, trust = torch.zeros(32), torch.zeros(4)
    merged = vf.optim_group_tables([(0, 16, 0), (16, 16, 0)], 1, "cpu")
    t = vf.optim_param_tables([(0, 16, 0), (16, 16, 0)], 1, "cpu")
    with pytest.raises(ValueError, match="per-parameter tables"):
        vf.lamb_step_groups(buf, buf, buf, buf, None, merged, trust)
    with pytest.raises(ValueError, match="cuts a parameter tensor"):
        vf.lamb_step_groups(buf[:24], buf[:24], buf[:24], buf[:24], None, t, trust)
    with pytest.raises(ValueError, match="cuts a parameter tensor"):
        vf.lamb_step_groups(buf[8:], buf[8:], buf[8:], buf[8:], None, t, trust, base=8)


# ------------------------------------------------------------------------------------------------------------------ factory
def test_opt_module_resolves_lamb_and_its_keys(vit):
    from vit_amd.optimizer import FusedAdamW, FusedLamb, FusedOptimizer, OptModule

    opt = OptModule.from_config({"type": "LAMB", "lr": 2e-3, "weight_decay": 0.02})(vit)
    assert type(opt) is FusedLamb and isinstance(opt, FusedAdamW) and isinstance(opt, FusedOptimizer)
    assert len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["betas"], g["eps"], g["always_adapt"], g["trust_clip"]) == \
           (2e-3, 0.02, (0.9, 0.999), 1e-6, False, False)
    assert FusedLamb._STATE == ("_m", "_v") and FusedLamb._SHARED == ("betas", "eps", "always_adapt", "trust_clip")
    assert opt._graph_betas() == (0.9, 0.999) and opt.last_trust_ratios is None
    mod = OptModule.from_config({"type": "lamb", "lr": 1e-3, "weight_decay": 0.05, "eps": 1e-5, "always_adapt": True,
                                 "trust_clip": True, "no_decay": True, "layer_decay": 0.75})
    assert "lamb" not in mod.opt_fns  # that table stays the reference's: lamb is resolved ahead of it
    opt = mod(vit)
    assert type(opt) is FusedLamb and len(opt.param_groups) == 10
    assert all((g["eps"], g["always_adapt"], g["trust_clip"]) == (1e-5, True, True) for g in opt.param_groups)
    assert {g["weight_decay"] for g in opt.param_groups} == {0.05, 0.0}
    assert [g["lr"] for g in opt.param_groups[::2]] == [1e-3 * 0.75 ** k for k in (4, 3, 2, 1, 0)]
    # the keys are read for this type only
    adamw = OptModule.from_config({"type": "AdamW", "lr": 1e-3, "eps": 1e-5, "always_adapt": True})(vit)
    assert type(adamw) is FusedAdamW and adamw.param_groups[0]["eps"] == 1e-8 and "always_adapt" not in adamw.param_groups[0]
    # a scheduler goes over it like over any other
    conf = OptModule.from_config({"type": "lamb", "lr": 1e-3, "lr_sch": "cosine", "T_max": 10})(vit)
    assert type(conf["optimizer"]) is FusedLamb and conf["lr_scheduler"]["interval"] == "epoch"


def test_lamb_on_a_model_that_is_not_a_myvit_raises():
    from vit_amd.optimizer import OptModule

    lin = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3))
    with pytest.raises(ValueError, match="torch has no LAMB"):
        OptModule.from_config({"type": "lamb", "lr": 1e-3})(lin)
    with pytest.raises(KeyError):  # as before for a type nobody knows
        OptModule.from_config({"type": "lars", "lr": 1e-3})(lin)


def test_a_zero1_reducer_is_refused(vit):
    from vit_amd.optimizer import FusedLamb

    class Stub:
        def __init__(self, mode):
            self.mode = mode

    opt = FusedLamb(vit, lr=1e-3)
    with pytest.raises(ValueError, match="zero1"):
        opt.attach_reducer(Stub("zero1"))
    assert opt._reducer is None
    red = Stub("allreduce")
    opt.attach_reducer(red)
    assert opt._reducer is red
    opt.attach_reducer(None)  # a single process
    assert opt._reducer is None


def test_groups_must_agree_on_what_the_kernels_share(vit):
    from vit_amd.optimizer import FusedLamb

    w = [p for p in vit.parameters() if p.ndim > 1]
    b = [p for p in vit.parameters() if p.ndim <= 1]
    for key, value in (("always_adapt", True), ("trust_clip", True), ("eps", 1e-8), ("betas", (0.9, 0.95))):
        with pytest.raises(ValueError, match=key):
            FusedLamb(vit, param_groups=[{"params": w}, {"params": b, key: value}])._check_shared()


def test_the_partition_is_one_segment_per_parameter(vit):
    import vit_amd.functional as vf
    from vit_amd.optimizer import FusedLamb, build_param_groups

    opt = FusedLamb(vit, lr=1e-3, weight_decay=0.05, param_groups=build_param_groups(vit, 1e-3, 0.05, no_decay=True))
    t = opt._partition()[2]
    lay = vit.engine.layout
    owned = [n for n in vit._param_names if lay.entries[n][0] < lay.n_trainable]
    assert isinstance(t, vf.ParamTables) and t.n_segments == len(owned) == len(opt._trust_names) and -1 not in t.owners
    assert t.starts == sorted(lay.entries[n][0] for n in owned)
    assert opt._trust.shape == (t.n_segments,) and bool((opt._trust == 1).all())
    # a parameter no group owns: its segment stays, owned by nobody, and its neighbours' segments end where they ended
    rest = [p for n, p in vit.named_parameters() if n != "vit.encoder.layer.1.output.dense.bias"]
    part = FusedLamb(vit, lr=1e-3, param_groups=[{"params": rest}])._partition()[2]
    assert part.n_segments == t.n_segments and part.owners.count(-1) == 1 and part.ends == t.ends
