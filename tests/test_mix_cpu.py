"""Host side of Mixup / CutMix (`augment:`, include/vit_amd_mix.h, vit_amd/mix.py): what can be checked without a GPU.  The kernels,
the soft losses and the trainer's use of the mixer are tests/test_mix_gpu.py's."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mix_ref as ref


def config(task="reg", augment=None, **model):
    cfg = {
        "model": dict(name="vit", task_type=task, image_size=512, patch_size=32, hidden_size=32, num_hidden_layers=1,
                      num_attention_heads=2, stride_size=32, proj_fn="SW", **model),
        "train": dict(batch_size=4, ep=2, precision="32"),
        "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0},
    }
    if augment is not None:
        cfg["augment"] = augment
    return cfg


SYMBOLS = ("vit_mix_plan_write", "vit_mix_signal", "vit_mix_targets")


def test_mix_symbols_are_exported_and_prototyped():
    from vit_amd import _cabi
    from vit_amd import build as vb

    vb.build(force=False, verbose=False)
    lib = _cabi.load()
    declared = _cabi.declared_symbols()
    for sym in SYMBOLS:
        assert sym in declared, f"{sym} is not declared by a header vit_amd.h includes"
        assert hasattr(lib, sym), f"{sym} declared but not exported"
        assert sym in _cabi._PROTOS, f"{sym} has no ctypes prototype"
    assert set(_cabi._PROTOS) == set(declared)
    assert lib.vit_version() == 100
    assert ctypes.sizeof(_cabi.MixRow) == 32
    assert (_cabi.LOSS_SOFT_CE, _cabi.LOSS_BCE) == (3, 4)


def test_mix_argument_errors_launch_nothing():
    """Every refusal comes back as VIT_ERR_ARG (-1) with a message, from the checks in front of the launch: the pointers below
    are not device memory (there is no GPU), so a call that got as far as a launch would not return -1."""
    from vit_amd import _cabi

    lib = _cabi.load()
    x, out, plan, lab = 0x10000, 0x20000, 0x30000, 0x40000  # 16-byte aligned, never dereferenced
    rows = (_cabi.MixRow * 2)()
    B, L, C = 4, 8, 3

    def refused(rc, *words):
        assert rc == -1
        msg = lib.vit_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(lib.vit_mix_plan_write(None, None, 1, rows, None), "vit_mix_plan_write", "null")
    refused(lib.vit_mix_plan_write(None, plan, 1, None, None), "vit_mix_plan_write", "null")
    refused(lib.vit_mix_plan_write(None, plan, 0, rows, None), "vit_mix_plan_write", "n_rows = 0")
    refused(lib.vit_mix_plan_write(None, plan + 8, 1, rows, None), "vit_mix_plan_write", "16-byte")

    refused(lib.vit_mix_signal(None, None, out, plan, 1, B, L, None), "vit_mix_signal", "null")
    refused(lib.vit_mix_signal(None, x, None, plan, 1, B, L, None), "vit_mix_signal", "null")
    refused(lib.vit_mix_signal(None, x, out, None, 1, B, L, None), "vit_mix_signal", "null")
    refused(lib.vit_mix_signal(None, x, out, plan, 1, 0, L, None), "vit_mix_signal", "B = 0")
    refused(lib.vit_mix_signal(None, x, out, plan, 1, -2, L, None), "vit_mix_signal", "B = -2")
    refused(lib.vit_mix_signal(None, x, out, plan, 1, B, 0, None), "vit_mix_signal", "L = 0")
    for n_rows in (0, 2, B + 1, -1):
        refused(lib.vit_mix_signal(None, x, out, plan, n_rows, B, L, None), "vit_mix_signal", f"n_rows = {n_rows}")
    refused(lib.vit_mix_signal(None, x + 4, out, plan, 1, B, L, None), "vit_mix_signal", "16-byte")
    refused(lib.vit_mix_signal(None, x, out + 8, plan, 1, B, L, None), "vit_mix_signal", "16-byte")
    refused(lib.vit_mix_signal(None, x, out, plan + 4, 1, B, L, None), "vit_mix_signal", "16-byte")
    refused(lib.vit_mix_signal(None, x, x + 16, plan, 1, B, L, None), "vit_mix_signal", "overlap")          # out inside x
    refused(lib.vit_mix_signal(None, x + B * L * 4 - 16, x, plan, 1, B, L, None), "vit_mix_signal", "overlap")  # x's tail in out

    for kind in (0, 1):
        refused(lib.vit_mix_targets(None, None, kind, out, plan, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "null")
        refused(lib.vit_mix_targets(None, lab, kind, None, plan, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "null")
        refused(lib.vit_mix_targets(None, lab, kind, out, None, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "null")
        refused(lib.vit_mix_targets(None, lab, kind, out, plan, 1, 0, C, 1.0, 0.0, None), "vit_mix_targets", "B = 0")
        refused(lib.vit_mix_targets(None, lab, kind, out, plan, 1, B, 0, 1.0, 0.0, None), "vit_mix_targets", "C = 0")
        refused(lib.vit_mix_targets(None, lab, kind, out, plan, 1, B, -1, 1.0, 0.0, None), "vit_mix_targets", "C = -1")
        refused(lib.vit_mix_targets(None, lab, kind, out, plan, 2, B, C, 1.0, 0.0, None), "vit_mix_targets", "n_rows = 2")
        refused(lib.vit_mix_targets(None, lab, kind, out + 4, plan, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "aligned")
        refused(lib.vit_mix_targets(None, lab, kind, out, plan + 8, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "aligned")
        refused(lib.vit_mix_targets(None, lab + 2, kind, out, plan, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "aligned")
        refused(lib.vit_mix_targets(None, out, kind, out, plan, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "overlaps")
    refused(lib.vit_mix_targets(None, lab, 2, out, plan, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "label_kind = 2")
    refused(lib.vit_mix_targets(None, lab + 4, 1, out, plan, 1, B, C, 1.0, 0.0, None), "vit_mix_targets", "aligned")  # int64: 8 bytes
    for on, off in ((float("nan"), 0.0), (1.0, float("inf")), (float("-inf"), 0.0)):
        refused(lib.vit_mix_targets(None, lab, 1, out, plan, 1, B, C, on, off, None), "vit_mix_targets", "finite")


def test_soft_loss_kinds_state_their_workspace_before_any_launch():
    """The forward of the two soft kinds leaves B row losses in the workspace: with a NULL handle (no workspace) the call
    comes back with VIT_ERR_WORKSPACE and that need; a kind past VIT_LOSS_BCE is an argument error in both directions."""
    from vit_amd import _cabi

    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no device exists to launch on")
    lib = _cabi.load()
    P = 0x10000
    B, T, D, C = 37, 6, 192, 7
    for kind in (_cabi.LOSS_SOFT_CE, _cabi.LOSS_BCE):
        assert lib.vit_head_loss_fwd(None, P, P, P, P, P, P, B, T, D, C, kind, None) == -4
        assert lib.vit_workspace_needed() == B * 4
        assert lib.vit_head_loss_bwd(None, P, P, P, P, P, P, P, P, B, T, D, C, kind, 0, None) == -4
        assert lib.vit_workspace_needed() == B * C * 4
    assert lib.vit_head_loss_fwd(None, P, P, P, P, P, P, B, T, D, C, 5, None) == -1
    assert lib.vit_head_loss_bwd(None, P, P, P, P, P, P, P, P, B, T, D, C, 5, 0, None) == -1


# ------------------------------------------------------------------------------------------------------------ Mixup.draw
def test_draw_is_a_function_of_seed_rank_and_call_number():
    from vit_amd.mix import Mixup

    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem")
    a, b = Mixup(seed=3, rank=0, **kw), Mixup(seed=3, rank=0, **kw)
    seq = [a.draw(6, 4096) for _ in range(5)]
    assert seq == [b.draw(6, 4096) for _ in range(5)]
    assert a.n == 5 and a.state_dict() == {"n": 5}
    assert all(len(rows) == 6 for rows in seq) and len({tuple(r) for r in seq[0]}) > 1
    assert len(Mixup(seed=3, mixup_alpha=0.8, mode="batch").draw(6, 4096)) == 1
    other_rank, other_seed = Mixup(seed=3, rank=1, **kw), Mixup(seed=4, rank=0, **kw)
    assert [other_rank.draw(6, 4096) for _ in range(5)] != seq and [other_seed.draw(6, 4096) for _ in range(5)] != seq
    # resume: a fresh mixer told the counter continues the sequence exactly
    c = Mixup(seed=3, rank=0, **kw)
    c.load_state_dict({"n": 3})
    assert [c.draw(6, 4096) for _ in range(2)] == seq[3:]
    # the same call number on another generator object: call n draws from default_rng([seed, rank, n])
    rng = np.random.default_rng([3, 0, 0])
    first = Mixup(seed=3, rank=0, **kw)._draw_row(rng, 4096)
    assert first == seq[0][0]


def test_prob_zero_and_no_alpha_give_identity_rows():
    from vit_amd.mix import IDENTITY_ROW, Mixup

    assert IDENTITY_ROW == ref.IDENTITY
    for m in (Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0, mode="elem"), Mixup(label_smoothing=0.1, num_classes=5, mode="elem")):
        for _ in range(8):
            assert m.draw(5, 100) == [IDENTITY_ROW] * 5


def test_draw_invariants_over_4096_draws():
    from vit_amd.mix import Mixup

    L, n = 4096, 4096
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5, mode="batch", seed=11)
    rows = [m.draw(8, L)[0] for _ in range(n)]
    ulp = float(np.spacing(np.float32(1.0)))
    n_cut, lams = 0, []
    for w, u, lo, hi, wy, uy in rows:
        assert 0 <= lo <= hi <= L
        for v in (w, u, wy, uy):
            assert v == float(np.float32(v))  # exact f32 values: what crosses the ABI is what was drawn
        assert abs((w + u) - 1.0) <= ulp and abs((wy + uy) - 1.0) <= ulp
        if u == 0.0:  # CutMix
            n_cut += 1
            assert w == 1.0 and uy == float(np.float32((hi - lo) / L)) and wy == float(np.float32(1.0 - (hi - lo) / L))
        else:
            assert (lo, hi) == (0, 0) and (wy, uy) == (w, u)
            lams.append(w)
    # the CutMix share under switch_prob = 0.5: within 5 binomial standard errors
    assert abs(n_cut / n - 0.5) <= 5 * math.sqrt(0.25 / n), n_cut
    assert len(lams) > 1000


def test_lam_mean_for_alpha_0p8():
    """Beta(a, a) has mean 0.5 and variance 1 / (4 (2a + 1)) = 0.0962 at a = 0.8: the standard error over 4096 draws is 0.0048;
    the mean is asserted within 5 of them (0.024)."""
    from vit_amd.mix import Mixup

    m = Mixup(mixup_alpha=0.8, seed=5)
    lam = [m.draw(4, 4096)[0][0] for _ in range(4096)]
    se = math.sqrt(1.0 / (4 * (2 * 0.8 + 1)) / 4096)
    assert abs(se - 0.0048) < 1e-4
    print(f"mean lam {np.mean(lam):.4f}")
    assert abs(float(np.mean(lam)) - 0.5) <= 5 * se


# ------------------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("augment", [None, {}, dict(mixup_alpha=0, cutmix_alpha=0, prob=1.0, switch_prob=0.5, mode="batch", label_smoothing=0.0),
                                     dict(mixup_alpha=0.0, cutmix_alpha=0.0)])
def test_off_by_default_no_mixer_object_exists(augment):
    from vit_amd.module import ViTLModule

    for task in ("reg", "cls"):
        extra = dict(num_labels=5) if task == "cls" else {}
        module = ViTLModule(config=config(task, augment, **extra))
        assert module.mixer is None


def test_a_configured_block_builds_the_mixer():
    from vit_amd._cabi import LOSS_BCE, LOSS_CE, LOSS_SOFT_CE
    from vit_amd.module import ViTLModule

    m = ViTLModule(config=config("reg", dict(mixup_alpha=0.8, mode="elem", seed=9))).mixer
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob, m.mode, m.num_classes, m.seed, m.n) == (0.8, 0.0, 1.0, 0.5, "elem", None, 9, 0)
    module = ViTLModule(config=config("cls", dict(cutmix_alpha=1.0, label_smoothing=0.1, soft_loss="bce"), num_labels=5))
    assert module.mixer.num_classes == 5 and module.mixer.label_smoothing == 0.1
    eng = module.model.engine
    assert eng.loss_kind == LOSS_CE and eng.soft_loss_kind == LOSS_BCE and module.loss_name == "ce"
    module = ViTLModule(config=config("cls", dict(label_smoothing=0.1), num_labels=5))  # plain label smoothing
    assert module.mixer is not None and module.model.engine.soft_loss_kind == LOSS_SOFT_CE
    on, off = module.mixer.on_off()
    assert (on, off) == ref.on_off(0.1, 5)


@pytest.mark.parametrize("task,augment,word", [
    ("reg", dict(mixup_alpha=0.8, label_smoothing=0.1), "label_smoothing"),
    ("reg", dict(mixup_alpha=0.8, soft_loss="ce"), "soft_loss"),
    ("reg", dict(soft_loss="bce"), "soft_loss"),
    ("reg", dict(mixup_alpha=-0.1), "mixup_alpha"),
    ("cls", dict(cutmix_alpha=-1.0), "cutmix_alpha"),
    ("reg", dict(mixup_alpha=0.8, prob=1.5), "prob"),
    ("reg", dict(mixup_alpha=0.8, prob=-0.1), "prob"),
    ("reg", dict(prob=2.0), "prob"),
    ("reg", dict(mixup_alpha=0.8, mode="pair"), "mode"),
    ("reg", dict(mixup_alpha=0.8, mode="half"), "mode"),
    ("cls", dict(mixup_alpha=0.8, soft_loss="focal"), "soft_loss"),
    ("cls", dict(label_smoothing=1.0), "label_smoothing"),
    ("reg", dict(mixup=0.8), "unknown"),
])
def test_config_errors_at_build_time(task, augment, word):
    from vit_amd.module import ViTLModule

    extra = dict(num_labels=5) if task == "cls" else {}
    with pytest.raises(ValueError, match=word):
        ViTLModule(config=config(task, augment, **extra))


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("s", [0.0, 0.1, 0.3])
def test_target_yardstick_against_torch(s):
    """F.cross_entropy(z, y, label_smoothing=s) is F.cross_entropy(z, smoothed one-hot rows); the yardstick's one-hot rows are
    those rows, its mixed targets are convex combinations of them (rows sum to 1), and its soft losses are torch's."""
    B, C = 6, 7
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(B, C, generator=gen, dtype=torch.float64)
    y = torch.randint(0, C, (B,), generator=gen)
    on, off = ref.on_off(s, C)
    oh = torch.from_numpy(ref.one_hot(y.numpy(), C, on, off))
    assert abs(float(F.cross_entropy(z, y, label_smoothing=s)) - float(F.cross_entropy(z, oh))) < 1e-6
    rows = [(1.0, 0.0, 0, 0, ref.f32(0.37), ref.f32(1 - 0.37)), ref.IDENTITY, (1.0, 0.0, 3, 9, ref.f32(0.75), ref.f32(0.25))] * 2
    t, bound, copied = ref.mix_targets_cls(y.numpy(), rows, C, s)
    assert np.abs(t.sum(axis=1) - 1.0).max() < 1e-6
    assert list(copied) == [False, True, False] * 2 and np.array_equal(t[1], oh.numpy()[1])
    assert abs(ref.soft_ce(z.numpy(), t) - float(F.cross_entropy(z, torch.from_numpy(t)))) < 1e-6
    assert abs(ref.bce(z.numpy(), t) - float(F.binary_cross_entropy_with_logits(z, torch.from_numpy(t)))) < 1e-6
    # a label outside [0, C) selects no `on` entry
    assert np.array_equal(ref.one_hot(np.array([C, -1]), C, on, off), np.full((2, C), float(np.float32(off))))


def test_signal_yardstick_by_hand():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    rows = [(0.25, 0.75, 0, 0, 0.25, 0.75), ref.IDENTITY, (1.0, 0.0, 1, 3, 0.5, 0.5)]
    out, kind, bound = ref.mix_signal(x, rows)
    assert out[0].tolist() == [0.25 * 0 + 0.75 * 8, 0.25 * 1 + 0.75 * 9, 0.25 * 2 + 0.75 * 10, 0.25 * 3 + 0.75 * 11]
    assert out[1].tolist() == [4, 5, 6, 7] and out[2].tolist() == [8, 1, 2, 11]
    assert kind.tolist() == [[2] * 4, [0] * 4, [0, 1, 1, 0]]
    assert bound[2].tolist() == [0, 0, 0, 0] and bound[0, 1] == 0.25 * 1 + 0.75 * 9
    # out-of-range spans are clamped; the middle row of an odd batch is its own partner
    out2, kind2, _ = ref.mix_signal(x, [(1.0, 0.0, -5, 13, 0.0, 1.0)])
    assert np.array_equal(out2, x[::-1]) and np.array_equal(out2[1], x[1])  # the full span: every row is its partner
    assert kind2[1].tolist() == [0] * 4
