"""Parameter groups in the fused optimizer steps on the MI355X, from the kernels (vit_amd/csrc/optim.hip: `*_step_groups`) up
to the trainer.

Gates.  Kernel level: the grouped call is `torch.equal` to the ungrouped entry point called slice by slice with each group's
numbers (p, state buffers, bf16 shadow, after each of three steps) -- the same arithmetic, so no tolerance; a sub-run stepped
with its `base` is `torch.equal` to the whole-buffer call.  Against torch.optim built with the same groups: rel < 1e-6, the
kernel-level gate of tests/test_optim_gpu.py (for AdamW's second moment see test_grouped_kernel_equals_torch_with_the_same_groups).  Model level: rel < 2e-6 per
tensor, that file's model-level gate.  Captured step against eager step: bit for bit."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_NORM = 0.5
BIG = 4096 * 256 * 4 + 1032  # past one full pass of the launch's grid (tests/test_optim_gpu.py: SIZES): the stride loop runs twice
# name -> (n, segment ends, group of each segment).  One segment | two of 8 | a boundary inside a wave's 256-element row |
# the n & 3 tail in the last segment | more segments than a wave has lanes | a second pass of the grid-stride loop.
# One segment (a one-group optimizer: the kernel takes the row once and runs the plain loop): 8 | with the n & 3 tail | a
# second pass of the loop
LAYOUTS = {
    "n8": (8, [8], [0]),
    "one1027": (1027, [1027], [0]),
    "onebig": (BIG, [BIG], [0]),
    "n16": (16, [8, 16], [0, 1]),
    "n1032": (1032, [8, 264, 1032], [0, 1, 2]),
    "n1027": (1027, [8, 1024, 1027], [0, 1, 2]),
    "300x8": (2400, [8 * (i + 1) for i in range(300)], [i % 3 for i in range(300)]),
    "big": (BIG, [264, 1000 * 1024 + 8, 1000 * 1024 + 16, 4096 * 256 * 4 - 512, BIG], [0, 1, 2, 1, 0]),
}
# sub-runs [0, a), [a, b), [b, n): every cut a multiple of 4 (16-byte accesses) that lies INSIDE a segment
CUTS = {"one1027": (12, 1000), "onebig": (1000 * 1024 + 12, 4096 * 256 * 4 + 4), "n16": (4, 12), "n1032": (100, 600), "n1027": (12, 1000), "300x8": (100, 1204), "big": (1000 * 1024 + 12, 4096 * 256 * 4 + 4)}
# (lr, weight_decay, momentum) of groups 0..2; group 2 has no momentum: its part of the buffer must stay untouched
HYPER = {"adamw": [(1e-3, 0.01, 0.0), (3e-4, 0.0, 0.0), (2e-3, 0.1, 0.0)],
         "adam_l2": [(1e-3, 0.01, 0.0), (3e-4, 0.0, 0.0), (2e-3, 0.1, 0.0)],
         "sgd": [(0.1, 0.01, 0.9), (0.03, 0.0, 0.8), (0.2, 0.1, 0.0)]}
KINDS = ["adamw", "adam_l2", "sgd"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


_INPUTS = {}


def _inputs(n):
    """(p0, g0) on the host, made once per size and never modified."""
    if n not in _INPUTS:
        gen = torch.Generator().manual_seed(2000 + n % 997)
        p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        g0[0] = 1.0 + g0[0].abs()  # the norm is above MAX_NORM whatever n: the clip coefficient is not 1
        _INPUTS[n] = (p0, g0)
    return _INPUTS[n]


def _tables(dev, layout, kind):
    import vit_amd.functional as vf

    n, ends, owners = LAYOUTS[layout]
    triples = [(a, b - a, gi) for a, b, gi in zip([0] + ends[:-1], ends, owners)]
    n_groups = max(owners) + 1
    t = vf.optim_group_tables(triples, n_groups, dev, total=n)
    assert vf.optim_groups_write(t, HYPER[kind][:n_groups]) and not vf.optim_groups_write(t, HYPER[kind][:n_groups])
    return t, triples


class _State:
    def __init__(self, dev, n, kind, poison=False):
        self.kind = kind
        self.p = _inputs(n)[0].to(dev)
        fill = float("nan") if poison else 0.0
        self.bufs = [torch.full((n,), fill, device=dev) for _ in range(1 if kind == "sgd" else 2)]
        self.pb = torch.zeros(n, dtype=torch.bfloat16, device=dev)

    def all(self):
        return [self.p, *self.bufs, self.pb]

    def grouped(self, g, tables, step, sq, a=0, b=None):
        import vit_amd.functional as vf

        b = self.p.numel() if b is None else b
        kw = dict(base=a, sqnorm=sq, max_norm=MAX_NORM)
        if self.kind == "sgd":
            vf.sgd_step_groups(self.p[a:b], g[a:b], self.bufs[0][a:b], self.pb[a:b], tables, **kw)
        else:
            vf.adamw_step_groups(self.p[a:b], g[a:b], self.bufs[0][a:b], self.bufs[1][a:b], self.pb[a:b], tables, step=step,
                                 l2=self.kind == "adam_l2", **kw)

    def plain(self, g, a, b, hyper, step, sq):
        import vit_amd.functional as vf

        lr, wd, mu = hyper
        kw = dict(lr=lr, weight_decay=wd, sqnorm=sq, max_norm=MAX_NORM)
        if self.kind == "sgd":
            vf.sgd_step(self.p[a:b], g[a:b], self.bufs[0][a:b], self.pb[a:b], momentum=mu, **kw)
        else:
            fn = vf.adam_l2_step if self.kind == "adam_l2" else vf.adamw_step
            fn(self.p[a:b], g[a:b], self.bufs[0][a:b], self.bufs[1][a:b], self.pb[a:b], step=step, **kw)


def _sq(g, clip):
    import vit_amd.functional as vf

    return vf.grad_sqnorm(g) if clip else None


# ---------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_kernel_equals_the_plain_one_slice_by_slice(dev, kind, layout, clip):
    n = LAYOUTS[layout][0]
    tables, triples = _tables(dev, layout, kind)
    one, ref = _State(dev, n, kind), _State(dev, n, kind)
    g0 = _inputs(n)[1].to(dev)
    for step in range(1, 4):
        g = g0 * step
        sq = _sq(g, clip)
        one.grouped(g, tables, step, sq)
        for a, numel, gi in triples:
            ref.plain(g, a, a + numel, HYPER[kind][gi], step, sq)
        for x, y, what in zip(one.all(), ref.all(), ("p", "state0", "state1/shadow", "shadow")):
            assert torch.equal(x, y), (step, what, int((x != y).sum()))
        assert torch.equal(one.pb, one.p.to(torch.bfloat16))
    assert torch.isfinite(one.p).all() and not torch.equal(one.p, _inputs(n)[0].to(dev))


@pytest.mark.parametrize("layout", list(CUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_sub_runs_with_their_base_equal_the_whole_buffer(dev, kind, layout):
    """What frozen parameters and `zero1` shards do: [a, b) stepped with base = a, starting and ending mid-segment."""
    n = LAYOUTS[layout][0]
    tables, _ = _tables(dev, layout, kind)
    whole, parts = _State(dev, n, kind), _State(dev, n, kind)
    g0 = _inputs(n)[1].to(dev)
    a, b = CUTS[layout]
    ends = LAYOUTS[layout][1]
    assert a % 4 == 0 and b % 4 == 0 and a not in ends and b not in ends and 0 < a < b < n
    for step in range(1, 4):
        g = g0 * step
        sq = _sq(g, True)
        whole.grouped(g, tables, step, sq)
        for lo, hi in ((b, n), (0, a), (a, b)):  # in any order
            parts.grouped(g, tables, step, sq, lo, hi)
        for x, y in zip(whole.all(), parts.all()):
            assert torch.equal(x, y), step


def test_a_poisoned_momentum_buffer_stays_poisoned_without_momentum(dev):
    import vit_amd.functional as vf

    n, ends, owners = LAYOUTS["n1032"]
    tables, triples = _tables(dev, "n1032", "sgd")
    assert vf.optim_groups_write(tables, [(lr, wd, 0.0) for lr, wd, _ in HYPER["sgd"]])
    one, ref = _State(dev, n, "sgd", poison=True), _State(dev, n, "sgd", poison=True)
    g = _inputs(n)[1].to(dev)
    one.grouped(g, tables, 1, None)
    for a, numel, gi in triples:
        ref.plain(g, a, a + numel, HYPER["sgd"][gi][:2] + (0.0,), 1, None)
    assert torch.isnan(one.bufs[0]).all() and torch.isfinite(one.p).all() and torch.equal(one.p, ref.p)
    # and a group without momentum beside groups with one: only ITS part of the buffer is left alone
    tables, _ = _tables(dev, "n1032", "sgd")
    two = _State(dev, n, "sgd")
    two.bufs[0][264:] = float("nan")
    two.grouped(g, tables, 1, None)
    assert torch.isnan(two.bufs[0][264:]).all() and torch.isfinite(two.bufs[0][:264]).all() and torch.isfinite(two.p).all()


# --------------------------------------------------------------------------------------------------------- against torch
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_kernel_equals_torch_with_the_same_groups(dev, kind, layout, clip):
    """The twin: torch.optim.AdamW / Adam / SGD over one tensor per segment, grouped as the table groups them.  rel < 1e-6 on
    p and on every state buffer torch keeps -- except AdamW's exp_avg_sq: vit_adamw_step forms 1.f - 0.999f where torch rounds
    1 - 0.999 after the subtraction, 1.3e-5 apart (include/vit_amd_optim.h; the Adam-L2 form follows torch and is gated)."""
    import vit_amd.functional as vf

    n, ends, owners = LAYOUTS[layout]
    tables, triples = _tables(dev, layout, kind)
    p0, g0 = _inputs(n)
    twins = [p0[a:a + k].clone().requires_grad_(True) for a, k, _ in triples]
    hyper = HYPER[kind][:max(owners) + 1]
    groups = [{"params": [t for t, (_, _, gi) in zip(twins, triples) if gi == i], "lr": lr, "weight_decay": wd,
               **({"momentum": mu} if kind == "sgd" else {})} for i, (lr, wd, mu) in enumerate(hyper)]
    cls = {"adamw": torch.optim.AdamW, "adam_l2": torch.optim.Adam, "sgd": torch.optim.SGD}[kind]
    ref = cls(groups, lr=1.0)
    ours = _State(dev, n, kind)
    for step in range(1, 4):
        gs = g0 * step
        for t, (a, k, _) in zip(twins, triples):
            t.grad = gs[a:a + k].clone()
        gd = gs.to(dev)
        sq = None
        if clip:  # the kernel gets the very norm torch clipped with (tests/test_optim_gpu.py: _clip_like_torch)
            norm = torch.nn.utils.clip_grad_norm_(twins, MAX_NORM)
            assert float(norm) > MAX_NORM
            sq = (norm.to(dev, torch.float32) ** 2).reshape(1)
            ours_norm = float(vf.grad_sqnorm(gd).sqrt())
            assert abs(ours_norm - float(gs.double().norm())) <= 1.5e-6 * float(gs.double().norm())
        ref.step()
        ours.grouped(gd, tables, step, sq)
        e = rel(ours.p, torch.cat([t.detach() for t in twins]))
        assert e < 1e-6, (step, e)
        assert torch.equal(ours.pb, ours.p.to(torch.bfloat16))
        keys = ("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq") if kind == "adam_l2" else ("exp_avg",)
        for key, buf in zip(keys, ours.bufs):
            for t, (a, k, gi) in zip(twins, triples):
                if kind == "sgd" and hyper[gi][2] == 0:
                    assert "momentum_buffer" not in ref.state[t] or ref.state[t]["momentum_buffer"] is None
                    assert float(buf[a:a + k].abs().max()) == 0  # untouched
                    continue
                e = rel(buf[a:a + k], ref.state[t][key])
                assert e < 1e-6, (step, key, a, e)


# ----------------------------------------------------------------------------------------------------------- model level
def _model_run(dev, kind, grouped):
    """Three clipped steps of the fused optimizer on C1 beside its torch twin on identical gradients; returns the model's
    final parameters by name."""
    from test_optim_gpu import _assert_same, _hand_over_grads
    from test_parity_gpu import setup
    from vit_amd.optimizer import FusedAdamW, FusedSGD, build_param_groups

    rc, g, sd, model, x, labels = setup("c1", dev)
    model.eval()
    twins = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    start = [p.detach().clone() for p in model.parameters()]
    lr, wd = (1e-2, 0.05) if kind == "sgd" else (1e-3, 0.05)
    groups = build_param_groups(model, lr, wd, no_decay=True, layer_decay=0.75) if grouped else None
    kw = dict(lr=lr, weight_decay=wd, **({"momentum": 0.9} if kind == "sgd" else {}))
    if grouped:
        twin_of = {id(p): tw for p, tw in zip(model.parameters(), twins)}
        ref_params = [dict(grp, params=[twin_of[id(p)] for p in grp["params"]]) for grp in groups]
        assert len(groups) == 2 * (rc.num_hidden_layers + 2)
    else:
        ref_params = twins
    if kind == "sgd":
        fused, ref = FusedSGD(model, param_groups=groups, **kw), torch.optim.SGD(ref_params, **kw)
    else:
        fused, ref = FusedAdamW(model, param_groups=groups, **kw), torch.optim.AdamW(ref_params, **kw)
    fused.set_grad_clip(MAX_NORM)
    for s in range(3):
        fused.zero_grad()
        model(x, labels=labels).loss.backward()
        with_grad = _hand_over_grads(model, twins)
        norm = torch.nn.utils.clip_grad_norm_(with_grad, MAX_NORM)
        fused.step()
        ref.step()
        got = float(fused.last_grad_norm.sqrt())
        assert abs(got - float(norm)) <= 1e-6 * float(norm), (s, got, float(norm))
        _assert_same(model, twins, start, s)
    assert len(with_grad) < len(twins)  # the pooler: in a group, without a gradient, untouched
    return {n: p.detach().clone() for n, p in model.named_parameters()}, fused


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_fused_optimizer_with_groups_equals_torch_on_the_model(dev, kind):
    grouped, opt = _model_run(dev, kind, True)
    plain, _ = _model_run(dev, kind, False)
    t = opt._partition()[2]
    assert t.n_groups == 10 and t.n_segments > 8 * 3  # decaying and non-decaying runs alternate inside every layer
    # the torch twin with weight_decay = 0 on these tensors was matched at 2e-6 above; and that IS another update than the one
    # decaying group gives them: every LayerNorm gain (~1, so 5e-5 of decay per AdamW step shows) and some bias
    ln = [n for n in grouped if "layernorm" in n and n.endswith(".weight")]
    bias = [n for n in grouped if n.endswith(".bias") and "pooler" not in n]
    assert len(ln) == 7 and len(bias) > 20
    assert all(not torch.equal(grouped[n], plain[n]) for n in ln)
    assert any(not torch.equal(grouped[n], plain[n]) for n in bias)
    assert not torch.equal(grouped["vit.encoder.layer.0.intermediate.dense.weight"],
                           plain["vit.encoder.layer.0.intermediate.dense.weight"])  # layer_decay: another rate


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_groups_with_a_trainable_preprocessor_and_a_frozen_layer(dev, kind):
    """Parameters outside the flat buffer (a trainable input preprocessor) take the plain kernel with THEIR group's numbers,
    and a frozen layer splits the flat buffer into two active runs, each one grouped launch with its base: three clipped steps
    against the torch twin with the same groups, at the model-level gate."""
    from oracle import refvit
    from test_optim_gpu import _assert_same, _hand_over_grads
    from vit_amd.config import ViTConfig
    from vit_amd.optimizer import FusedAdamW, FusedSGD, build_param_groups
    from vit_amd.preprocessor import LinearPreprocessor
    from vit_amd.specvit import MyViT

    L_in, r = 96, 64
    rc = refvit.RefConfig(image_size=r, patch_size=16, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
                          stride_size=16, loss_name="mae")
    sd = refvit.make_state_dict(rc, 71)
    gen = torch.Generator().manual_seed(72)
    P0, b0 = torch.randn(r, L_in, generator=gen) / L_in ** 0.5, torch.randn(r, generator=gen) * 0.1
    x, labels = torch.randn(5, L_in, generator=gen).to(dev), torch.rand(5, generator=gen).to(dev)
    cfg = ViTConfig(task_type="reg", image_size=r, patch_size=16, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
                    stride_size=16)
    model = MyViT(cfg, loss_name="mae", preprocessor=LinearPreprocessor(P0.clone(), bias=b0.clone(), freeze=False))
    model.set_precision("32")
    model.load_state_dict({**sd, "preprocessor.linear.weight": P0, "preprocessor.linear.bias": b0}, strict=True)
    model = model.to(dev).eval()
    for n, prm in model.named_parameters():
        if n.startswith("vit.encoder.layer.1."):
            prm.requires_grad_(False)
    lr, wd = (1e-2, 0.05) if kind == "sgd" else (1e-3, 0.05)
    groups = build_param_groups(model, lr, wd, no_decay=True, layer_decay=0.75)
    by_id = {id(q): n for n, q in model.named_parameters()}
    where = {by_id[id(q)]: (g["lr"], g["weight_decay"]) for g in groups for q in g["params"]}
    assert where["preprocessor.linear.weight"] == (lr, wd) and where["preprocessor.linear.bias"] == (lr, 0.0)
    assert where["vit.encoder.layer.0.output.dense.bias"] == (lr * 0.75 ** 3, 0.0)
    twins = [torch.nn.Parameter(q.detach().clone()) for q in model.parameters()]
    start = [q.detach().clone() for q in model.parameters()]
    twin_of = {id(q): tw for q, tw in zip(model.parameters(), twins)}
    ref_groups = [dict(g, params=[twin_of[id(q)] for q in g["params"]]) for g in groups]
    kw = dict(lr=lr, weight_decay=wd, **({"momentum": 0.9} if kind == "sgd" else {}))
    if kind == "sgd":
        fused, ref = FusedSGD(model, param_groups=groups, **kw), torch.optim.SGD(ref_groups, **kw)
    else:
        fused, ref = FusedAdamW(model, param_groups=groups, **kw), torch.optim.AdamW(ref_groups, **kw)
    assert len(fused._extras) == 2
    fused.set_grad_clip(MAX_NORM)
    for s in range(3):
        fused.zero_grad()
        model(x, labels=labels).loss.backward()
        assert len(fused._active_ranges()) == 2  # the frozen layer in the middle
        norm = torch.nn.utils.clip_grad_norm_(_hand_over_grads(model, twins), MAX_NORM)
        fused.step()
        ref.step()
        got = float(fused.last_grad_norm.sqrt())
        assert abs(got - float(norm)) <= 1e-6 * float(norm), (s, got, float(norm))
        _assert_same(model, twins, start, s)
    moved = {n: not torch.equal(q.detach(), q0) for (n, q), q0 in zip(model.named_parameters(), start)}
    assert moved["preprocessor.linear.weight"] and moved["preprocessor.linear.bias"] and moved["regressor.weight"]
    assert not any(v for n, v in moved.items() if n.startswith("vit.encoder.layer.1."))


@pytest.mark.parametrize("n_groups", [1, 2])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_a_frozen_flat_buffer_beside_a_trainable_preprocessor(dev, kind, n_groups):
    """No parameter of the flat buffer is stepped: the ViT is frozen and the optimizer is built over what still trains, the
    preprocessor outside the flat buffer.  (The head keeps requires_grad, in no group: the model runs a backward only while some
    parameter of the flat buffer wants a gradient.)  There is no run and no table to build -- the step takes the by-value kernel
    on the preprocessor alone, three clipped steps against the torch twin at the model-level gate, and the flat buffer keeps its
    bits."""
    from oracle import refvit
    from test_optim_gpu import _assert_same, _hand_over_grads
    from vit_amd.config import ViTConfig
    from vit_amd.optimizer import FusedAdamW, FusedSGD
    from vit_amd.preprocessor import LinearPreprocessor
    from vit_amd.specvit import MyViT

    L_in, r = 96, 64
    rc = refvit.RefConfig(image_size=r, patch_size=16, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
                          stride_size=16, loss_name="mae")
    sd = refvit.make_state_dict(rc, 71)
    gen = torch.Generator().manual_seed(72)
    P0, b0 = torch.randn(r, L_in, generator=gen) / L_in ** 0.5, torch.randn(r, generator=gen) * 0.1
    x, labels = torch.randn(5, L_in, generator=gen).to(dev), torch.rand(5, generator=gen).to(dev)
    cfg = ViTConfig(task_type="reg", image_size=r, patch_size=16, hidden_size=32, num_hidden_layers=3, num_attention_heads=2,
                    stride_size=16)
    model = MyViT(cfg, loss_name="mae", preprocessor=LinearPreprocessor(P0.clone(), bias=b0.clone(), freeze=False))
    model.set_precision("32")
    model.load_state_dict({**sd, "preprocessor.linear.weight": P0, "preprocessor.linear.bias": b0}, strict=True)
    model = model.to(dev).eval()
    for n, prm in model.named_parameters():
        if n.startswith("vit."):
            prm.requires_grad_(False)
    named = dict(model.named_parameters())
    w, b = named["preprocessor.linear.weight"], named["preprocessor.linear.bias"]
    lr, wd = (1e-2, 0.05) if kind == "sgd" else (1e-3, 0.05)
    groups = [{"params": [w, b]}] if n_groups == 1 else [{"params": [w]}, {"params": [b], "lr": lr * 0.5, "weight_decay": 0.0}]
    twins = [torch.nn.Parameter(q.detach().clone()) for q in model.parameters()]
    start = [q.detach().clone() for q in model.parameters()]
    twin_of = {id(q): tw for q, tw in zip(model.parameters(), twins)}
    ref_groups = [dict(g, params=[twin_of[id(q)] for q in g["params"]]) for g in groups]
    kw = dict(lr=lr, weight_decay=wd, **({"momentum": 0.9} if kind == "sgd" else {}))
    if kind == "sgd":
        fused, ref = FusedSGD(model, param_groups=groups, **kw), torch.optim.SGD(ref_groups, **kw)
    else:
        fused, ref = FusedAdamW(model, param_groups=groups, **kw), torch.optim.AdamW(ref_groups, **kw)
    assert len(fused.param_groups) == n_groups and len(fused._extras) == 2
    with pytest.raises(ValueError, match="no parameter group owns"):
        fused._partition()  # the state in question: a table cannot be built, and the step must not ask for one
    fused.set_grad_clip(MAX_NORM)
    flat0 = model.engine.flat.detach().clone()
    for s in range(3):
        fused.zero_grad()
        model(x, labels=labels).loss.backward()
        assert fused._active_ranges() == []
        _hand_over_grads(model, twins)
        norm = torch.nn.utils.clip_grad_norm_([twin_of[id(w)], twin_of[id(b)]], MAX_NORM)
        fused.step()
        ref.step()
        got = float(fused.last_grad_norm.sqrt())
        assert abs(got - float(norm)) <= 1e-6 * float(norm), (s, got, float(norm))
        _assert_same(model, twins, start, s)
    assert fused._step == 3 and torch.equal(model.engine.flat, flat0)
    assert not torch.equal(w.detach(), start[list(named).index("preprocessor.linear.weight")])


# -------------------------------------------------------------------------------------------------------------- trainer
def _opt_cfg(kind):
    """SGD under one-cycle: every group's lr AND momentum move on every step.  AdamW without a scheduler: one-cycle would also
    cycle beta1, which a captured step freezes with or without groups (it is a kernel argument); the test moves the groups'
    rates itself instead, each group by its own factor on every step."""
    cfg = {"type": kind, "lr": 1e-2 if kind == "SGD" else 1e-3, "weight_decay": 0.05, "no_decay": True, "layer_decay": 0.75}
    if kind == "SGD":
        cfg["lr_sch"] = "onecycle"
    return cfg


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
@pytest.mark.parametrize("kind", ["AdamW", "SGD"])
def test_hip_graph_step_with_groups_equals_eager(dev, kind, precision):
    """Every group's rate (under one-cycle also SGD's momentum) moves on every step: the group table is rewritten ahead of each replay,
    and four replays == four eager steps bit for bit (the pattern of test_optim_gpu.py::_graph_vs_eager, dropout off)."""
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedOptimizer

    batches = list(Batches(64, 5))
    finals = {}
    for mode in ("eager", "graph"):
        cfg = c1_config(precision=precision, hip_graph=(mode == "graph"))
        cfg["opt"] = _opt_cfg(kind)
        cfg["data"]["num_samples"] = 64
        module, trainer = make(cfg)
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        opt = trainer.optimizer
        assert isinstance(opt, FusedOptimizer) and len(opt.param_groups) == 10
        losses, trace = [], []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for i in range(4):
                if kind == "AdamW" and i:
                    for k, grp in enumerate(opt.param_groups):
                        grp["lr"] *= 1.0 - 0.05 * (k + i)
                trace.append(tuple((g["lr"], g.get("momentum"), g["weight_decay"]) for g in opt.param_groups))
                b = tuple(t.cuda() for t in batches[i % 2])
                losses.append(float(trainer.training_step(module, b, i)))
        assert not [w for w in caught if "hip_graph" in str(w.message)], [str(w.message) for w in caught]
        state = [getattr(opt, name).detach().cpu().clone() for name in opt._STATE]
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in module.model.state_dict().items()}, state,
                        float(opt.last_grad_norm), opt._step, trace)
        if mode == "graph":
            assert trainer.use_graph
            assert len(trainer._graphed) == 1 and all(isinstance(g, GraphedTrainStep) for g in trainer._graphed.values())
    e, g = finals["eager"], finals["graph"]
    assert e[0] == g[0], (e[0], g[0])
    for k in e[1]:
        assert torch.equal(e[1][k], g[1][k]), k
    assert len(e[2]) == len(g[2]) >= 1 and all(torch.equal(a, b) for a, b in zip(e[2], g[2]))
    assert e[3] == g[3] and e[4] == g[4] == 4 and e[5] == g[5]
    assert e[0][0] != e[0][2]  # the parameters moved
    assert len(set(e[5])) == 4 and len({lr for lr, _, _ in e[5][0]}) == 5  # rates change every step; five depths
    assert {wd for _, _, wd in e[5][0]} == {0.05, 0.0}


def test_repartitioning_after_capture_falls_back_to_eager(dev):
    from test_trainer_gpu import Batches, c1_config, make

    cfg = c1_config(precision="bf16-mixed", hip_graph=True)
    cfg["opt"] = _opt_cfg("AdamW")
    module, trainer = make(cfg)
    trainer._setup(module)
    module.train()
    b = tuple(t.to(dev) for t in next(iter(Batches(16, 5))))
    trainer.training_step(module, b, 0)
    opt = trainer.optimizer
    assert trainer.use_graph and len(opt.param_groups) == 10
    moved = opt.param_groups[2]["params"].pop()  # a layer-0 weight joins layer 1's group
    opt.param_groups[4]["params"].append(moved)
    before = module.model.engine.flat.detach().clone()
    with pytest.warns(UserWarning, match="repartitioned"):
        loss = trainer.training_step(module, b, 1)
    assert not trainer.use_graph and torch.isfinite(loss) and trainer.global_step == 2
    assert not torch.equal(before, module.model.engine.flat)
    assert opt._group_index[id(moved)] == 4  # the eager step rebuilt the tables from the new partition
