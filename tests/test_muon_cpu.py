"""Fused Muon, the parts that need no GPU: the factory (`opt.type: muon`), the matrix / AdamW split, what is refused, the ABI
table of include/vit_amd_muon.h with its poison and footprint coverage, the table builders, torch's `_adjust_lr`, and the yardstick
of tests/test_muon_gpu.py: the float64 restatement (tests/_muon_ref.py) against torch.optim.Muon on the CPU."""
import ctypes

import pytest
import torch

import _muon_ref as mr

SHAPES = [(32, 32), (32, 128), (128, 32), (96, 32), (192, 768), (768, 192)]


@pytest.fixture(scope="module")
def lib():
    from vit_amd import _cabi
    from vit_amd import build as vb

    vb.build(force=False, verbose=False)
    return _cabi.load()


def _vit(**kw):
    """The `l3` case's geometry (tests/test_cls_tail_gpu.py: C1, D = 32, F = 128, three layers)."""
    from test_cls_tail_gpu import case
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    rc = case("l3")[0]
    base = dict(task_type=rc.task_type, image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
                stride_size=rc.stride_size, num_labels=rc.num_labels)
    base.update(kw)
    return MyViT(ViTConfig(**base), loss_name="mae")


@pytest.fixture(scope="module")
def vit():
    return _vit()


# ------------------------------------------------------------------------------------------------------------------ factory
def test_opt_module_builds_a_fused_muon_with_its_defaults(vit):
    from vit_amd.optimizer import FusedAdamW, FusedMuon, FusedOptimizer, OptModule

    opt = OptModule.from_config({"type": "Muon", "lr": 2e-3, "weight_decay": 0.02})(vit)
    assert type(opt) is FusedMuon and isinstance(opt, FusedAdamW) and isinstance(opt, FusedOptimizer)
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["betas"], g["eps"]) == (2e-3, 0.02, (0.9, 0.999), 1e-8)
    assert (g["momentum"], g["nesterov"], g["ns_steps"], g["ns_coefficients"], g["muon_eps"], g["adjust_lr"]) == \
           (0.95, True, 5, (3.4445, -4.775, 2.0315), 1e-7, "match_rms_adamw")
    assert FusedMuon._STATE == ("_m", "_v", "_buf") and opt.last_ns_norms is None and opt._graph_betas() == (0.9, 0.999)
    mod = OptModule.from_config({"type": "muon", "lr": 1e-3, "weight_decay": 0.05, "no_decay": True, "layer_decay": 0.75,
                                 "muon": {"momentum": 0.9, "nesterov": False, "ns_steps": 3, "ns_coefficients": [3.0, -4.0, 2.0],
                                          "eps": 1e-6, "adjust_lr": "original"}})
    assert "muon" not in mod.opt_fns
    opt = mod(vit)
    assert type(opt) is FusedMuon and len(opt.param_groups) == 10
    assert all((g["momentum"], g["nesterov"], g["ns_steps"], g["ns_coefficients"], g["muon_eps"], g["adjust_lr"]) ==
               (0.9, False, 3, (3.0, -4.0, 2.0), 1e-6, "original") for g in opt.param_groups)
    # the section is read for this type only, and a scheduler goes over the optimizer like over any other
    adamw = OptModule.from_config({"type": "AdamW", "lr": 1e-3, "muon": {"nonsense": 1}})(vit)
    assert type(adamw) is FusedAdamW and "momentum" not in adamw.param_groups[0]
    conf = OptModule.from_config({"type": "muon", "lr": 1e-3, "lr_sch": "cosine", "T_max": 10, "warmup": {"epochs": 2}})(vit)
    assert type(conf["optimizer"]) is FusedMuon and conf["lr_scheduler"]["interval"] == "epoch"


def test_the_shipped_config_resolves(vit):
    import os

    import yaml

    from vit_amd.optimizer import FusedMuon, OptModule

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "exp", "muon.yaml")))
    base = yaml.safe_load(open(os.path.join(root, "configs", "baseline.yaml")))
    assert cfg["model"] == base["model"]  # baseline.yaml's geometry
    conf = OptModule.from_config(cfg["opt"])(vit)
    assert type(conf["optimizer"]) is FusedMuon and "SequentialLR" in type(conf["lr_scheduler"]["scheduler"]).__name__


@pytest.mark.parametrize("section,needle", [({"momentun": 0.9}, "unknown keys"), ({"lr": 1e-3}, "unknown keys"),
                                            ({"adjust_lr": "rms"}, "adjust_lr"), ({"momentum": 1.0}, "momentum"),
                                            ({"ns_steps": 100}, "ns_steps"), ({"ns_coefficients": [1.0, 2.0]}, "ns_coefficients"),
                                            ({"eps": 0.0}, "eps")])
def test_bad_muon_keys_raise(vit, section, needle):
    from vit_amd.optimizer import OptModule

    with pytest.raises(ValueError, match=needle):
        OptModule.from_config({"type": "muon", "lr": 1e-3, "muon": section})(vit)


def test_muon_on_a_model_that_is_not_a_myvit_raises():
    from vit_amd.optimizer import OptModule

    lin = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3))
    with pytest.raises(ValueError, match="FusedMuon"):
        OptModule.from_config({"type": "muon", "lr": 1e-3})(lin)


def test_a_zero1_reducer_is_refused(vit):
    from vit_amd.optimizer import FusedMuon

    class Stub:
        def __init__(self, mode):
            self.mode = mode

    opt = FusedMuon(vit, lr=1e-3)
    with pytest.raises(ValueError, match="zero1"):
        opt.attach_reducer(Stub("zero1"))
    assert opt._reducer is None
    red = Stub("allreduce")
    opt.attach_reducer(red)
    assert opt._reducer is red


# ------------------------------------------------------------------------------------------------------------------ the split
def test_the_split_names_exactly_the_six_stems_per_layer(vit):
    from vit_amd.optimizer import MUON_STEMS, FusedMuon

    opt = FusedMuon(vit, lr=1e-3)
    mats, rest = opt.muon_split()
    want = [f"vit.encoder.layer.{i}.{stem}.weight" for i in range(3) for stem in MUON_STEMS]
    assert sorted(mats) == sorted(want) and len(mats) == 18
    lay = vit.engine.layout
    assert sorted(mats + rest) == sorted(n for n in vit._param_names if lay.entries[n][0] < lay.n_trainable)
    assert all(len(lay.entries[n][1]) == 2 for n in mats)
    for n in ("vit.embeddings.patch_embeddings.projection.weight", "regressor.weight", "vit.embeddings.cls_token",
              "vit.encoder.layer.0.attention.attention.query.bias", "vit.encoder.layer.2.layernorm_after.weight", "vit.layernorm.bias"):
        assert n in rest, n
    # compact offsets: one matrix behind the other in flat-buffer order
    xo = 0
    for name, _, off, xoff, rows, cols in opt._matrices():
        assert (off, (rows, cols)) == lay.entries[name] and xoff == xo
        xo += rows * cols


def test_registers_layerscale_and_a_mim_decoder_land_on_the_adamw_side():
    from vit_amd.optimizer import FusedMuon

    model = _vit(task_type="mim", num_register_tokens=4, layer_scale_init=1e-5)
    mats, rest = FusedMuon(model, lr=1e-3).muon_split()
    assert len(mats) == 18 and all(".weight" in n and "encoder.layer" in n for n in mats)
    for n in ("vit.embeddings.register_tokens", "vit.embeddings.mask_token", "decoder.weight", "decoder.bias",
              "vit.encoder.layer.0.layer_scale1.lambda1", "vit.encoder.layer.2.layer_scale2.lambda1",
              "vit.embeddings.position_embeddings" if "vit.embeddings.position_embeddings" in model._param_names else "decoder.bias"):
        assert n in rest, n


def test_a_parameter_no_group_owns_is_on_neither_side(vit):
    from vit_amd.optimizer import FusedMuon

    skip = "vit.encoder.layer.1.intermediate.dense.weight"
    opt = FusedMuon(vit, lr=1e-3, param_groups=[{"params": [p for n, p in vit.named_parameters() if n != skip]}])
    mats, rest = opt.muon_split()
    assert skip not in mats and skip not in rest and len(mats) == 17
    full = {m[0]: m[3] for m in FusedMuon(vit, lr=1e-3)._matrices()}
    assert all(full[m[0]] == m[3] for m in opt._matrices())  # the others keep their place in the compact buffers


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_the_muon_table_is_complete(lib):
    """Every function vit_amd_muon.h declares is exported and has a prototype in _PROTOS_MUON -- a table of its own: the header
    is outside vit_amd.h's include closure and its names outside _PROTOS."""
    import vit_amd.functional as vf
    from vit_amd import _cabi

    declared = _cabi.declared_muon_symbols()
    assert len(declared) == 5 and set(declared) == set(_cabi._PROTOS_MUON)
    assert not set(_cabi._PROTOS_MUON) & set(_cabi._PROTOS) and not set(declared) & set(_cabi.declared_symbols())
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == _cabi._PROTOS_MUON[name] and fn.restype is ctypes.c_int, name
    header = open(_cabi.MUON_HEADER_PATH).read()
    assert '#include "vit_amd.h"' in header
    assert "vit_amd_muon.h" not in open(_cabi.HEADER_PATH).read()
    assert f"#define VIT_MUON_TILE {vf.MUON_TILE} " in header and f"#define VIT_MUON_GEMM_TILE {vf.MUON_GEMM_TILE} " in header
    assert ctypes.sizeof(_cabi.MuonMat) == 48 and ctypes.sizeof(_cabi.MuonProblem) == 72


def test_every_muon_export_has_a_poison_and_a_footprint_case():
    import test_muon_gpu as tg
    from vit_amd import _cabi

    poison = {e for c in tg.POISON_CASES for e in c.entries}
    foot = {e for c in tg.FOOTPRINT_CASES for e in c.entries}
    assert poison == set(_cabi._PROTOS_MUON), sorted(set(_cabi._PROTOS_MUON) ^ poison)
    assert foot == set(_cabi._PROTOS_MUON), sorted(set(_cabi._PROTOS_MUON) ^ foot)
    for table in (tg.POISON_CASES, tg.FOOTPRINT_CASES):
        ids = [c.id for c in table]
        assert len(ids) == len(set(ids)), ids


P = 0x1000  # a non-null "device pointer": every call below must fail its argument check before it could be used


def test_argument_errors(lib):
    def err(rc, *needles):
        assert rc == -1, rc
        msg = lib.vit_last_error().decode()
        assert all(n in msg for n in needles), msg

    err(lib.vit_muon_momentum(None, None, P, P, P, 1, 1, 0.95, 1, None, 0.0, P, None), "vit_muon_momentum", "null pointer")
    err(lib.vit_muon_momentum(None, P, P, P, P, 0, 1, 0.95, 1, None, 0.0, P, None), "n_mats = 0")
    err(lib.vit_muon_momentum(None, P, P, P, P, 1, 1, 1.0, 1, None, 0.0, P, None), "momentum")
    err(lib.vit_muon_norms(None, P, 1, None, 1e-7, P, P, None), "vit_muon_norms", "null pointer")
    err(lib.vit_muon_norms(None, P, 1, P, 0.0, P, P, None), "eps")
    err(lib.vit_muon_normalize(None, P, P, P, 1, 1, P, None), "alias")
    err(lib.vit_muon_normalize(None, P, P + 64, P, 1, 0, P, None), "n_ttiles = 0")
    err(lib.vit_muon_gemm_grouped(None, None, 1, P, 1, 1, None), "vit_muon_gemm_grouped", "null pointer")
    err(lib.vit_muon_gemm_grouped(None, P, 1, P, 0, 1, None), "n_tiles = 0")
    err(lib.vit_muon_apply(None, P, None, None, P, 1, 1, P, 1, None), "vit_muon_apply", "null pointer")
    err(lib.vit_muon_apply(None, P, None, P, P, 1, 1, P, 0, None), "n_groups = 0")


# ------------------------------------------------------------------------------------------------------------ table builders
def test_the_matrix_table_counts_tiles_and_refuses_bad_matrices():
    import vit_amd.functional as vf

    t = vf.muon_mat_table([(0, 0, 32, 32, 0, 1.0), (1024, 1024, 96, 128, 1, 2.0), (13312 + 8, 13312, 128, 32, 0, 0.5)], "cpu")
    assert (t.n_mats, t.n_tiles, t.n_ttiles) == (3, 1 + 3 + 1, 1 + 3 * 4 + 4)
    raw = (vf._cabi.MuonMat * 3).from_buffer_copy(bytes(t.mats.numpy()))
    assert [(m.off, m.xoff, m.rows, m.cols, m.group, m.ratio, m.tile0, m.ttile0) for m in raw] == \
           [(0, 0, 32, 32, 0, 1.0, 0, 0), (1024, 1024, 96, 128, 1, 2.0, 1, 1), (13320, 13312, 128, 32, 0, 0.5, 4, 13)]
    t.check_run(0, 13320 + 4096)
    for base, n in ((8, 20000), (0, 13320 + 4095), (0, 1000)):
        with pytest.raises(ValueError, match="cuts the matrix"):
            t.check_run(base, n)
    for bad, needle in (([(0, 0, 24, 32, 0, 1.0)], "multiples of 16"), ([(0, 0, 0, 32, 0, 1.0)], "multiples of 16"),
                        ([(4, 0, 32, 32, 0, 1.0)], "multiples of 8"), ([(0, 0, 32, 32, 0, 1.0), (512, 1024, 32, 32, 0, 1.0)], "overlap"),
                        ([(0, 0, 32, 32, 0, 1.0), (1024, 512, 32, 32, 0, 1.0)], "overlap"), ([], "at least one"),
                        ([(0, 0, 32, 32, -1, 1.0)], "group")):
        with pytest.raises(ValueError, match=needle):
            vf.muon_mat_table(bad, "cpu")
    with pytest.raises(ValueError, match="past its buffer"):
        vf.muon_mat_table([(0, 0, 32, 32, 0, 1.0)], "cpu", total=1000)


def test_the_problem_table_maps_tiles_and_refuses_bad_problems():
    import vit_amd.functional as vf

    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    t = vf.muon_problem_table([(z(32, 48), z(80, 48), None, z(32, 80), 1.0, 0.0), (z(192, 64), z(192, 64), z(192, 192), z(192, 192), 2.0, 3.0)],
                              True, "cpu")
    assert (t.n_problems, t.n_tiles, t.shapes) == (2, 2 + 9, [(32, 80, 48), (192, 192, 64)])
    assert t.tiles.tolist()[:3] == [[0, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]] and t.tiles.tolist()[-1] == [1, 2, 2, 0]
    x = z(64, 64)
    for probs, bt, needle in (([(z(32, 48), z(80, 32), None, z(32, 80), 1.0, 0.0)], True, "expected a bf16 matrix"),
                              ([(z(24, 32), z(32, 32), None, z(24, 32), 1.0, 0.0)], True, "multiples of 16"),
                              ([(z(32, 32), z(32, 32), None, z(32, 32), 1.0, 2.0)], False, "needs R"),
                              ([(x, x, None, x, 1.0, 0.0)], True, "overlaps an operand"),
                              ([(z(32, 32).float(), z(32, 32), None, z(32, 32), 1.0, 0.0)], True, "expected a bf16 matrix"),
                              ([(z(32, 36)[:, :32], z(32, 32), None, z(32, 32), 1.0, 0.0)], True, "leading dimension"),
                              ([], True, "at least one")):
        with pytest.raises(ValueError, match=needle):
            vf.muon_problem_table(probs, bt, "cpu")
    # the rule is table-wide: C of one problem must overlap neither an operand nor the output of ANOTHER problem
    y, w = z(32, 32), z(64, 32)
    with pytest.raises(ValueError, match="overlaps an operand of the launch"):
        vf.muon_problem_table([(z(32, 32), z(32, 32), None, y, 1.0, 0.0), (y, z(32, 32), None, z(32, 32), 1.0, 0.0)], True, "cpu")
    with pytest.raises(ValueError, match="overlaps an operand of the launch"):
        vf.muon_problem_table([(z(32, 32), z(32, 32), None, w[16:48], 1.0, 0.0), (z(32, 32), z(32, 32), w[:32], z(32, 32), 1.0, 1.0)],
                              True, "cpu")
    with pytest.raises(ValueError, match="outputs of problems 0 and 1 overlap"):
        vf.muon_problem_table([(z(32, 32), z(32, 32), None, w[:32], 1.0, 0.0), (z(32, 32), z(32, 32), None, w[16:48], 1.0, 0.0)],
                              True, "cpu")


def test_load_state_dict_keeps_the_buffer_in_place_and_takes_the_legacy_layout(vit):
    """A captured step holds the momentum buffer's address, so a load copies into the existing buffer; a dict without "state"
    (FusedAdamW's flat layout of old) goes to the base class."""
    from vit_amd.optimizer import FusedMuon

    opt = FusedMuon(vit, lr=1e-3)
    mats = opt._matrices()
    opt._buf = torch.full((opt._mat_total,), 7.0)
    index = {id(p): i for i, p in enumerate(opt._all_params())}
    _, p, _, xoff, rows, cols = mats[3]
    state = {index[id(p)]: {"momentum_buffer": torch.full((rows, cols), 2.0)}}
    held, ptr = opt._buf, opt._buf.data_ptr()
    opt.load_state_dict({"state": state, "param_groups": []})
    assert opt._buf is held and opt._buf.data_ptr() == ptr
    assert bool((opt._buf[xoff:xoff + rows * cols] == 2.0).all()) and float(opt._buf.sum()) == 2.0 * rows * cols
    n = vit.engine.flat.numel()
    opt.load_state_dict({"step": 5, "m": torch.ones(n), "v": torch.ones(n), "param_groups": []})
    assert opt._step == 5 and opt._buf is held and bool((opt._m == 1).all())


def test_ratio_equals_torchs_adjust_lr():
    import vit_amd.functional as vf
    from torch.optim._muon import _adjust_lr

    for rows, cols in SHAPES + [(768, 768), (3072, 768), (768, 3072)]:
        for mode in ("original", "match_rms_adamw", "none"):
            want = _adjust_lr(1.0, mode, torch.Size((rows, cols)))
            assert vf.muon_adjust_ratio(mode, rows, cols) == want == mr.ratio(mode, rows, cols), (mode, rows, cols)
    assert vf.muon_adjust_ratio("none", 64, 16) == 1.0 and vf.muon_adjust_ratio("original", 64, 16) == 2.0
    with pytest.raises(ValueError, match="adjust_lr"):
        vf.muon_adjust_ratio("rms", 16, 16)


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_the_restatement_against_torch_muon(shape):
    """e_ref = rel(torch.optim.Muon, the unrounded f64 iteration) on an N(0, 1) matrix: 1.2e-2 .. 1.9e-2 over these shapes.  The
    restatement WITH the contract's rounding points -- a second, independent bf16 implementation -- must itself lie within the
    margin the GPU tests grant the kernels, and the unrounded one must not be the rounded one."""
    gen = torch.Generator().manual_seed(1000 + shape[0] * 7 + shape[1])
    u = torch.randn(*shape, generator=gen)
    e, exact = mr.e_ref(u)
    emu = mr.rel(mr.newton_schulz(u, rounded=True), exact)
    print(f"[muon yardstick {shape}] e_ref {e:.3e}, emulation {emu:.3e}, ratio {emu / e:.2f}")
    assert exact.shape == u.shape and 2e-3 < e < 5e-2
    assert emu <= mr.MARGIN * e
    sv = torch.linalg.svdvals(exact)
    assert float(sv.max()) < 1.3  # the quintic's band from above; a square matrix's smallest singular values stay small
    wrong = mr.rel(mr.newton_schulz(u, coefficients=(3.4445, -4.775, 2.5), rounded=True), exact)
    assert wrong > 4 * mr.MARGIN * e  # a wrong coefficient is far outside the margin


def test_the_restated_momentum_is_torchs():
    gen = torch.Generator().manual_seed(5)
    g = [torch.randn(32, 48, generator=gen) for _ in range(3)]
    W = torch.nn.Parameter(torch.zeros(32, 48))
    opt = torch.optim.Muon([W], lr=1e-3, weight_decay=0.0, momentum=0.95, nesterov=True)
    buf = torch.zeros(32, 48, dtype=torch.float64)
    for s in range(3):
        W.grad = g[s].clone()
        opt.step()
        buf, _ = mr.momentum_update(buf, g[s].double())
        got = opt.state[W]["momentum_buffer"].double()
        assert float((got - buf).abs().max()) <= 4 * (s + 1) * 2.0 ** -24 * float(buf.abs().max())
