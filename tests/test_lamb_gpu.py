"""Fused LAMB on the MI355X, from the three kernels (vit_amd/csrc/optim.hip: vit_lamb_step*) up to the trainer.

The yardstick (tests/_lamb_ref.py): there is no torch LAMB, so the formulas of include/vit_amd_optim.h are restated in plain torch
ops as a torch.optim.Optimizer on CPU tensors and run twice on the same f32 inputs -- in float64 (the reference) and in float32.
The f32 run's distance from the f64 run, per tensor in max-norm, is d32; the kernels must lie within 4 * d32 + 1 ulp of the f64
run for p, m, v and the trust ratio.  The measured d32 are printed.  Inputs are chosen so that the restatement itself is
well-conditioned (p ~ N(0, 0.02), g ~ N(0, 1e-3), zeros only where a case places them).

Everything else is bit for bit: sub-runs of whole segments against the whole-buffer call, the by-value entry point against a
one-segment table, the captured step against the eager step, a resumed run against an uninterrupted one, two ranks."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

from _lamb_ref import RefLamb, bound, f32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = 0.05  # below the test gradients' norm (~0.15): the clip coefficient is not 1
HYPER = [(1e-3, 0.05), (3e-4, 0.0), (2e-3, 0.1)]  # (lr, weight_decay) of groups 0..2; group 1 adapts only under always_adapt


def _layout():
    """[(name, numel)] of the kernel tests' flat buffer, ~2.2e4 elements.  T = vf.LAMB_TILE: a tile is cut at T from a segment's
    start, so T - 4 | T | T + 4 | 2 T + 8 are one short tile | one full | full + the shortest | two full + one short; 8 and 16
    are the shortest segments; `zero` is all zero (p, g, state), `still` has no gradient and no state, `large` is scaled so
    that its ratio is above 1; the last segment's end is not a multiple of 4 (the scalar tail)."""
    import vit_amd.functional as vf

    T = vf.LAMB_TILE
    return [("n8", 8), ("n16", 16), ("t-4", T - 4), ("zero", 16), ("t", T), ("still", 24), ("large", 32), ("t+4", T + 4),
            ("2t+8", 2 * T + 8), ("tail", 1027)]  # `large` (index 6) decays with two groups and with three: its ratio is a real one


_DATA = {}


def _data():
    """(p0, [g of step 1..3]) on the host, made once and never modified."""
    if not _DATA:
        gen = torch.Generator().manual_seed(4242)
        names = _layout()
        n = sum(k for _, k in names)
        p0 = torch.randn(n, generator=gen) * 0.02
        gs = [torch.randn(n, generator=gen) * 1e-3 for _ in range(3)]
        off = 0
        for name, k in names:
            if name in ("zero", "still"):
                for g in gs:
                    g[off:off + k] = 0
            if name == "zero":
                p0[off:off + k] = 0
            if name == "large":
                p0[off:off + k] *= 5000.0  # ||p|| ~ 100 * sqrt(32) against ||u|| <~ sqrt(32)
            off += k
        _DATA["x"] = (p0, gs)
    return _DATA["x"]


def _spans():
    out, off = [], 0
    for name, k in _layout():
        out.append((name, off, k))
        off += k
    return out


def _tables(dev, n_groups):
    import vit_amd.functional as vf

    spans = _spans()
    n = spans[-1][1] + spans[-1][2]
    owners = [i % n_groups for i in range(len(spans))]
    t = vf.optim_param_tables([(off, k, gi) for (_, off, k), gi in zip(spans, owners)], n_groups, dev, total=n)
    vf.optim_groups_write(t, [(lr, wd, 0.0) for lr, wd in HYPER[:n_groups]])
    return t, owners, n


def _sq(g):
    """The squared gradient norm as the f32 the step kernels read."""
    return f32(float(g.double().pow(2).sum()))


def _restate(dtype, owners, n_groups, always_adapt, trust_clip, clip, steps=3):
    """The restatement over the kernel tests' tensors: per step [(p, m, v, trust) per tensor]."""
    p0, gs = _data()
    params = [torch.nn.Parameter(p0[off:off + k].to(dtype).clone()) for _, off, k in _spans()]
    groups = [{"params": [q for q, gi in zip(params, owners) if gi == j], "lr": HYPER[j][0], "weight_decay": HYPER[j][1]}
              for j in range(n_groups)]
    opt = RefLamb(groups, always_adapt=always_adapt, trust_clip=trust_clip, max_norm=MAX_NORM if clip else None)
    out = []
    for s in range(steps):
        for q, (_, off, k) in zip(params, _spans()):
            q.grad = gs[s][off:off + k].to(dtype).clone()
        opt.step(sqnorm=_sq(gs[s]) if clip else None)
        out.append([(q.detach().clone(), opt.state[q]["m"].clone(), opt.state[q]["v"].clone(), opt.trust[id(q)].clone())
                    for q in params])
    return out


_REF = {}


def _reference(n_groups, always_adapt, trust_clip, clip):
    key = (n_groups, always_adapt, trust_clip, clip)
    if key not in _REF:
        owners = [i % n_groups for i in range(len(_layout()))]
        _REF[key] = (_restate(torch.float64, owners, n_groups, always_adapt, trust_clip, clip),
                     _restate(torch.float32, owners, n_groups, always_adapt, trust_clip, clip))
    return _REF[key]


def _worse(worst, what, d32, err, allowed):
    """Per kind, over every tensor and step: the largest d32, the largest kernel error, the largest error / allowed."""
    a, b, c = worst.get(what, (0.0, 0.0, 0.0))
    worst[what] = (max(a, d32), max(b, err), max(c, err / allowed))


def _show(worst):
    return ", ".join(f"{k} (d32 {v[0]:.3e}, error {v[1]:.3e}, error / allowed {v[2]:.3f})" for k, v in worst.items())


def _device_state(dev, n):
    p0, gs = _data()
    return dict(p=p0.to(dev).clone(), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev),
                pb=torch.zeros(n, device=dev, dtype=torch.bfloat16), gs=[g.to(dev) for g in gs])


def _kernel_step(st, t, trust, s, always_adapt, trust_clip, clip, lo=0, hi=None):
    import vit_amd.functional as vf

    hi = st["p"].numel() if hi is None else hi
    sq = torch.tensor([_sq(_data()[1][s])], device=st["p"].device) if clip else None
    vf.lamb_step_groups(st["p"][lo:hi], st["gs"][s][lo:hi], st["m"][lo:hi], st["v"][lo:hi], st["pb"][lo:hi], t, trust, base=lo,
                        always_adapt=always_adapt, trust_clip=trust_clip, step=s + 1, sqnorm=sq, max_norm=MAX_NORM)


# ------------------------------------------------------------------------------------------------ 1. kernel against restatement
@pytest.mark.parametrize("adapt_clip", [(False, False), (True, False), (False, True)], ids=["plain", "always_adapt", "trust_clip"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("n_groups", [2, 3])
def test_kernel_against_the_restatement(dev, n_groups, clip, adapt_clip):
    always_adapt, trust_clip = adapt_clip
    t, owners, n = _tables(dev, n_groups)
    ref64, ref32 = _reference(n_groups, always_adapt, trust_clip, clip)
    st = _device_state(dev, n)
    trust = torch.zeros(t.n_segments, device=dev)
    p0 = _data()[0]
    worst = {}
    for s in range(3):  # steps 1 and 3 are asked for; 2 rides along
        g_before = st["gs"][s].clone()
        _kernel_step(st, t, trust, s, always_adapt, trust_clip, clip)
        torch.cuda.synchronize()
        assert torch.equal(st["gs"][s], g_before)  # g is only read
        assert torch.equal(st["pb"], st["p"].bfloat16())
        got_trust = trust.cpu()
        for i, (name, off, k) in enumerate(_spans()):
            wd = HYPER[owners[i]][1]
            for what, got, r64, r32 in (("p", st["p"][off:off + k].cpu(), ref64[s][i][0], ref32[s][i][0]),
                                        ("m", st["m"][off:off + k].cpu(), ref64[s][i][1], ref32[s][i][1]),
                                        ("v", st["v"][off:off + k].cpu(), ref64[s][i][2], ref32[s][i][2]),
                                        ("trust", got_trust[i:i + 1], ref64[s][i][3], ref32[s][i][3])):
                d32, allowed = bound(r64, r32)
                err = float((got.double().reshape(-1) - r64.double().reshape(-1)).abs().max())
                _worse(worst, what, d32, err, allowed)
                assert err <= allowed, (s + 1, name, what, err, d32, allowed)
            r = float(got_trust[i])
            if name == "zero":  # every zero-norm branch: r is exactly 1 and p stays where it was
                assert r == 1.0 and torch.equal(st["p"][off:off + k].cpu(), p0[off:off + k])
            if name == "still" and wd == 0:  # no gradient, no state, no decay: u = 0
                assert r == 1.0 and torch.equal(st["p"][off:off + k].cpu(), p0[off:off + k])
            if wd == 0 and not always_adapt:
                assert r == 1.0, (name, r)
            if wd == 0 and always_adapt and name not in ("zero", "still"):
                assert r != 1.0, (name, r)
            if name == "large":
                assert wd != 0  # the tensor scaled so that its ratio is above 1 -- clipped to exactly 1 under trust_clip
                assert (r == 1.0) if trust_clip else (r > 5.0), (name, r)
            if trust_clip:
                assert r <= 1.0
    print(f"[lamb kernel] groups {n_groups} clip {clip} always_adapt {always_adapt} trust_clip {trust_clip}: worst " + _show(worst))


def test_the_restatement_agrees_with_itself_on_the_zero_norm_branches():
    """Before relying on it: on every tensor whose ratio is decided by a zero norm or by `adapt`, the f32 and the f64 run take the
    same branch (their ratio is exactly 1 in both)."""
    for key in [(2, False, False, True), (3, True, False, False)]:
        ref64, ref32 = _reference(*key)
        for s in range(3):
            for (name, _, _), a, b in zip(_spans(), ref64[s], ref32[s]):
                assert (float(a[3]) == 1.0) == (float(b[3]) == 1.0), (key, s, name)
                if name == "zero":
                    assert float(a[3]) == 1.0


# ------------------------------------------------------------------------------------------------ 2. sub-runs of whole segments
def test_sub_runs_of_whole_segments_equal_the_whole_buffer_call(dev):
    t, owners, n = _tables(dev, 3)
    whole, parts = _device_state(dev, n), _device_state(dev, n)
    trust_w, trust_p = torch.zeros(t.n_segments, device=dev), torch.zeros(t.n_segments, device=dev)
    spans = _spans()
    cuts = [0, spans[2][1], spans[3][1], spans[7][1], n]  # segment starts; the second sub-run is one segment of T - 4 elements
    for s in range(3):
        _kernel_step(whole, t, trust_w, s, True, False, True)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            _kernel_step(parts, t, trust_p, s, True, False, True, lo, hi)
        for key in ("p", "m", "v", "pb"):
            assert torch.equal(whole[key], parts[key]), (s, key)
        assert torch.equal(trust_w, trust_p), s
    assert float(trust_w.min()) > 0 and len(set(trust_w.tolist())) > 5


def test_a_run_that_cuts_a_tensor_is_refused(dev):
    t, owners, n = _tables(dev, 2)
    st = _device_state(dev, n)
    trust = torch.zeros(t.n_segments, device=dev)
    with pytest.raises(ValueError, match="cuts a parameter tensor"):
        _kernel_step(st, t, trust, 0, False, False, False, 0, _spans()[2][1] + 8)
    with pytest.raises(ValueError, match="cuts a parameter tensor"):
        _kernel_step(st, t, trust, 0, False, False, False, 4, n)
    assert torch.equal(st["p"].cpu(), _data()[0])


# ------------------------------------------------------------------------------------------------ 3. by value == table
@pytest.mark.parametrize("n", ["8", "T+4", "2T+11"])
def test_by_value_equals_the_one_segment_table(dev, n):
    import vit_amd.functional as vf

    n = {"8": 8, "T+4": vf.LAMB_TILE + 4, "2T+11": 2 * vf.LAMB_TILE + 11}[n]
    gen = torch.Generator().manual_seed(n)
    p0, g0 = (torch.randn(n, generator=gen) * 0.02).to(dev), (torch.randn(n, generator=gen) * 1e-3).to(dev)
    sq = torch.tensor([_sq(g0.cpu())], device=dev)
    t = vf.optim_param_tables([(0, n, 0)], 1, dev, total=n)
    vf.optim_groups_write(t, [(1e-3, 0.05, 0.0)])
    a = dict(p=p0.clone(), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev), pb=torch.zeros(n, device=dev, dtype=torch.bfloat16))
    b = {k: x.clone() for k, x in a.items()}
    ta, tb = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    for step in (1, 2):
        vf.lamb_step(a["p"], g0, a["m"], a["v"], a["pb"], lr=1e-3, weight_decay=0.05, step=step, sqnorm=sq, max_norm=0.01, trust=ta)
        vf.lamb_step_groups(b["p"], g0, b["m"], b["v"], b["pb"], t, tb, step=step, sqnorm=sq, max_norm=0.01)
        for k in a:
            assert torch.equal(a[k], b[k]), (step, k)
        assert torch.equal(ta, tb) and float(ta) > 0 and float(ta) != 1.0
    c = {k: x.clone() for k, x in b.items()}
    vf.lamb_step(a["p"], g0, a["m"], a["v"], a["pb"], lr=1e-3, weight_decay=0.05, step=3, sqnorm=sq, max_norm=0.01)  # trust=None
    vf.lamb_step_groups(c["p"], g0, c["m"], c["v"], c["pb"], t, tb, step=3, sqnorm=sq, max_norm=0.01)
    assert all(torch.equal(a[k], c[k]) for k in a)


# ------------------------------------------------------------------------------------------------ 4. poison
def test_poison_outside_the_runs_and_in_a_gap_stays_out_of_every_norm(dev):
    """The buffer: [front | A | B | gap | C | back]; A, B, C are tensors of two groups, the gap is a tensor no group owns, front and
    back lie outside every run.  p, m and v are NaN in front, gap and back.  Stepped as two runs (A B, then C) and as one run
    over the table's whole extent (the gap, a segment of its own with group -1, is skipped): the poison stays, every ratio is
    finite, and A, B, C come out bit for bit as from a buffer without poison."""
    import vit_amd.functional as vf

    T = vf.LAMB_TILE
    front, A, B, gap, Cn, back = 16, T + 4, 8, 24, 40, 16
    offs = [front, front + A, front + A + B + gap]
    n = front + A + B + gap + Cn + back
    t = vf.optim_param_tables([(offs[0], A, 0), (offs[1], B, 1), (offs[2], Cn, 0)], 2, dev)
    assert t.owners == [-1, 0, 1, -1, 0]
    vf.optim_groups_write(t, [(1e-3, 0.05, 0.0), (3e-4, 0.0, 0.0)])
    gen = torch.Generator().manual_seed(99)
    p0, g0 = (torch.randn(n, generator=gen) * 0.02).to(dev), (torch.randn(n, generator=gen) * 1e-3).to(dev)
    dirty = torch.zeros(n, dtype=torch.bool, device=dev)
    for lo, hi in ((0, front), (offs[1] + B, offs[2]), (offs[2] + Cn, n)):
        dirty[lo:hi] = True
    runs = [(offs[0], offs[1] + B), (offs[2], offs[2] + Cn)]
    results = {}
    for mode in ("clean", "two runs", "one run"):
        st = dict(p=p0.clone(), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev),
                  pb=torch.zeros(n, device=dev, dtype=torch.bfloat16))
        if mode != "clean":
            for k in ("p", "m", "v"):
                st[k][dirty] = float("nan")
        trust = torch.full((t.n_segments,), -7.0, device=dev)
        for step in (1, 2):
            for lo, hi in (runs if mode != "one run" else [(offs[0], offs[2] + Cn)]):
                vf.lamb_step_groups(st["p"][lo:hi], g0[lo:hi], st["m"][lo:hi], st["v"][lo:hi], st["pb"][lo:hi], t, trust, base=lo,
                                    always_adapt=True, step=step)
        if mode != "clean":
            for k in ("p", "m", "v"):
                assert bool(torch.isnan(st[k][dirty]).all()), (mode, k)
            assert not bool(st["pb"][dirty].float().abs().sum())  # the shadow of what no run covers is not written
        assert trust[[0, 3]].tolist() == [-7.0, -7.0]  # the gaps' entries are nobody's
        assert bool(torch.isfinite(trust[[1, 2, 4]]).all()) and float(trust[[1, 2, 4]].min()) > 0
        results[mode] = ({k: x[~dirty].clone() for k, x in st.items()}, trust.clone())
    for mode in ("two runs", "one run"):
        for k, x in results["clean"][0].items():
            assert torch.equal(x, results[mode][0][k]), (mode, k)
        assert torch.equal(results["clean"][1], results[mode][1]), mode


# ------------------------------------------------------------------------------------------------ 5. / 6. model level
def _small_model(dev, precision, layers, preprocessor=False):
    from oracle import refvit
    from vit_amd.config import ViTConfig
    from vit_amd.preprocessor import LinearPreprocessor
    from vit_amd.specvit import MyViT

    L_in, r = 96, 64
    rc = refvit.RefConfig(image_size=r, patch_size=16, hidden_size=32, num_hidden_layers=layers, num_attention_heads=2,
                          stride_size=16, loss_name="mae")
    sd = refvit.make_state_dict(rc, 71)
    gen = torch.Generator().manual_seed(72)
    P0, b0 = torch.randn(r, L_in, generator=gen) / L_in ** 0.5, torch.randn(r, generator=gen) * 0.1
    x, labels = torch.randn(5, L_in if preprocessor else r, generator=gen).to(dev), torch.rand(5, generator=gen).to(dev)
    cfg = ViTConfig(task_type="reg", image_size=r, patch_size=16, hidden_size=32, num_hidden_layers=layers, num_attention_heads=2,
                    stride_size=16)
    if preprocessor:
        model = MyViT(cfg, loss_name="mae", preprocessor=LinearPreprocessor(P0.clone(), bias=b0.clone(), freeze=False))
        sd = {**sd, "preprocessor.linear.weight": P0, "preprocessor.linear.bias": b0}
    else:
        model = MyViT(cfg, loss_name="mae")
    model.set_precision(precision)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval(), x, labels


def _twin_optimizers(model, groups, lr, wd, clip):
    """The restatement twice (f64, f32) over CPU twins of the model's parameters, with the same groups."""
    out = []
    for dtype in (torch.float64, torch.float32):
        twins = [torch.nn.Parameter(q.detach().cpu().to(dtype).clone()) for q in model.parameters()]
        twin_of = {id(q): tw for q, tw in zip(model.parameters(), twins)}
        ref_groups = [dict(g, params=[twin_of[id(q)] for q in g["params"]]) for g in groups]
        out.append((twins, RefLamb(ref_groups, lr=lr, weight_decay=wd, max_norm=clip)))
    return out


def _model_steps(dev, model, x, labels, fused, refs, steps=3, expect_runs=None):
    """`steps` clipped steps of `fused` beside the two restatements fed the same gradients and the same f32 squared norm; every
    tensor's p, m, v and trust ratio within 4 * d32 + 1 ulp of the f64 run.  Returns the worst (d32, error, error / allowed) per kind."""
    eng, lay = model.engine, model.engine.layout
    names = [n for n, _ in model.named_parameters()]
    worst = {}
    for s in range(steps):
        fused.zero_grad()
        model(x, labels=labels).loss.backward()
        if expect_runs is not None:
            assert len(fused._active_ranges()) == expect_runs
        grads = [None if q.grad is None else q.grad.detach().cpu().clone() for q in model.parameters()]
        fused.step()
        sq = float(fused.last_grad_norm)  # the f32 the kernels read
        exact = sum(float(g.double().pow(2).sum()) for g in grads if g is not None)  # every gradient, the extras' included
        assert abs(sq - exact) <= 1e-6 * exact, (s, sq, exact)
        for twins, ref in refs:
            for tw, g in zip(twins, grads):
                tw.grad = None if g is None else g.to(tw.dtype)
            ref.step(sqnorm=sq)
        (tw64, ref64), (tw32, ref32) = refs
        tnames, tvals = fused.last_trust_ratios
        trust_of = dict(zip(tnames, tvals.cpu().tolist()))
        for name, q, a, b, g in zip(names, model.parameters(), tw64, tw32, grads):
            if g is None:  # the pooler, a frozen layer: untouched by all three
                assert torch.equal(q.detach().cpu().double(), a.detach()), name
                continue
            if name in lay.entries:
                off, k = lay.entries[name][0], lay.numel(name)
                m, v = fused._m[off:off + k].cpu(), fused._v[off:off + k].cpu()
            else:
                m, v = (buf.cpu() for buf in fused._extra_state[id(q)])
            for what, got, r64, r32 in (("p", q.detach().cpu(), a.detach(), b.detach()), ("m", m, ref64.state[a]["m"], ref32.state[b]["m"]),
                                        ("v", v, ref64.state[a]["v"], ref32.state[b]["v"]),
                                        ("trust", torch.tensor([trust_of[name]]), ref64.trust[id(a)], ref32.trust[id(b)])):
                d32, allowed = bound(r64, r32)
                err = float((got.double().reshape(-1) - r64.double().reshape(-1)).abs().max())
                _worse(worst, what, d32, err, allowed)
                assert err <= allowed, (s + 1, name, what, err, d32, allowed)
        if eng.precision == "bf16":
            n = lay.n_trainable
            assert torch.equal(eng.shadow[:n], eng.flat[:n].bfloat16())
    return worst


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_fused_lamb_on_the_model_against_the_restatement(dev, precision):
    from vit_amd.optimizer import FusedLamb, build_param_groups

    model, x, labels = _small_model(dev, precision, layers=2)
    lr, wd = 1e-3, 0.05
    groups = build_param_groups(model, lr, wd, no_decay=True, layer_decay=0.75)
    fused = FusedLamb(model, lr=lr, weight_decay=wd, param_groups=groups)
    fused.set_grad_clip(0.5)
    assert fused.last_trust_ratios is None
    refs = _twin_optimizers(model, groups, lr, wd, 0.5)
    worst = _model_steps(dev, model, x, labels, fused, refs)
    t = fused._partition()[2]
    assert t.n_groups == 2 * (2 + 2) and t.n_segments == len(fused._trust_names)  # one segment per tensor, no gaps
    names, ratios = fused.last_trust_ratios
    assert len(names) == ratios.numel() and names == sorted(names, key=lambda n: model.engine.layout.entries[n][0])
    decayed = [r for n, r in zip(names, ratios.tolist()) if n.endswith("dense.weight")]
    plain = [r for n, r in zip(names, ratios.tolist()) if n.endswith(".bias")]
    assert all(r != 1.0 and r > 0 for r in decayed) and all(r == 1.0 for r in plain)
    print(f"[lamb model {precision}] worst " + _show(worst))


def test_a_frozen_layer_and_a_trainable_preprocessor(dev):
    """The frozen middle layer splits the flat buffer into two active runs (two table launches, each of whole tensors); the
    preprocessor's two parameters, outside the flat buffer, take vit_lamb_step with their group's numbers and their gradients
    join the clipping norm (checked against the f64 sum over every gradient inside `_model_steps`)."""
    from vit_amd.optimizer import FusedLamb, build_param_groups

    model, x, labels = _small_model(dev, "32", layers=3, preprocessor=True)
    for n, prm in model.named_parameters():
        if n.startswith("vit.encoder.layer.1."):
            prm.requires_grad_(False)
    lr, wd = 1e-3, 0.05
    groups = build_param_groups(model, lr, wd, no_decay=True, layer_decay=0.75)
    fused = FusedLamb(model, lr=lr, weight_decay=wd, param_groups=groups)
    assert len(fused._extras) == 2
    fused.set_grad_clip(0.5)
    start = {n: q.detach().clone() for n, q in model.named_parameters()}
    refs = _twin_optimizers(model, groups, lr, wd, 0.5)
    worst = _model_steps(dev, model, x, labels, fused, refs, expect_runs=2)
    names, ratios = fused.last_trust_ratios
    got = dict(zip(names, ratios.tolist()))
    assert set(names[-2:]) == {"preprocessor.linear.weight", "preprocessor.linear.bias"}
    assert got["preprocessor.linear.weight"] not in (0.0, 1.0) and got["preprocessor.linear.bias"] == 1.0
    for n, q in model.named_parameters():
        frozen = n.startswith("vit.encoder.layer.1.")
        assert torch.equal(q.detach(), start[n]) == (frozen or "pooler" in n), n
        if frozen:
            assert got[n] == 1.0  # never stepped: its entry keeps the initial 1
    print("[lamb frozen + preprocessor] worst " + _show(worst))


# ------------------------------------------------------------------------------------------------ 7. captured == eager
LAMB_CFG = {"type": "lamb", "lr": 2e-3, "weight_decay": 0.05, "no_decay": True, "layer_decay": 0.75, "always_adapt": True}


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_hip_graph_step_equals_eager(dev, precision):
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedLamb

    batches = list(Batches(64, 5))
    finals = {}
    for mode in ("eager", "graph"):
        cfg = c1_config(precision=precision, hip_graph=(mode == "graph"))
        cfg["opt"] = dict(LAMB_CFG)
        cfg["data"]["num_samples"] = 64
        module, trainer = make(cfg)
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        opt = trainer.optimizer
        assert type(opt) is FusedLamb and len(opt.param_groups) == 10 and opt.param_groups[0]["always_adapt"] is True
        losses = []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for i in range(4):
                if i:
                    for k, grp in enumerate(opt.param_groups):
                        grp["lr"] *= 1.0 - 0.05 * (k + i)
                b = tuple(t.cuda() for t in batches[i % 2])
                losses.append(float(trainer.training_step(module, b, i)))
        assert not [w for w in caught if "hip_graph" in str(w.message)], [str(w.message) for w in caught]
        names, ratios = opt.last_trust_ratios
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in module.model.state_dict().items()},
                        [getattr(opt, name).detach().cpu().clone() for name in opt._STATE], float(opt.last_grad_norm), opt._step,
                        names, ratios.cpu().clone())
        if mode == "graph":
            assert trainer.use_graph
            assert len(trainer._graphed) == 1 and all(isinstance(g, GraphedTrainStep) for g in trainer._graphed.values())
    e, g = finals["eager"], finals["graph"]
    assert e[0] == g[0], (e[0], g[0])
    for k in e[1]:
        assert torch.equal(e[1][k], g[1][k]), k
    assert len(e[2]) == 2 and all(torch.equal(a, b) for a, b in zip(e[2], g[2]))
    assert e[3] == g[3] and e[4] == g[4] == 4
    assert e[5] == g[5] and torch.equal(e[6], g[6]) and len(set(e[6].tolist())) > 10
    assert e[0][0] != e[0][2]  # the parameters moved


def test_repartitioning_after_capture_falls_back_to_eager(dev):
    from test_trainer_gpu import Batches, c1_config, make

    cfg = c1_config(precision="bf16-mixed", hip_graph=True)
    cfg["opt"] = dict(LAMB_CFG)
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
    assert opt._group_index[id(moved)] == 4


# ------------------------------------------------------------------------------------------------ 8. resume
def test_resume_is_bit_identical_and_an_adamw_state_dict_loads(dev):
    from vit_amd.optimizer import FusedAdamW, FusedLamb, build_param_groups

    def fresh(cls=FusedLamb):
        model, x, labels = _small_model(dev, "bf16-mixed", layers=2)
        groups = build_param_groups(model, 1e-3, 0.05, no_decay=True, layer_decay=0.75)
        opt = cls(model, lr=1e-3, weight_decay=0.05, param_groups=groups)
        opt.set_grad_clip(0.5)
        return model, x, labels, opt

    def one_step(model, x, labels, opt):
        opt.zero_grad()
        model(x, labels=labels).loss.backward()
        opt.step()

    model, x, labels, opt = fresh()
    for _ in range(2):
        one_step(model, x, labels, opt)
    sd, weights = opt.state_dict(), {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert sd["param_groups"][0]["always_adapt"] is False and sd["param_groups"][0]["eps"] == 1e-6
    one_step(model, x, labels, opt)
    model2, _, _, opt2 = fresh()
    model2.load_state_dict(weights)
    opt2.load_state_dict(sd)
    assert opt2._step == 2
    one_step(model2, x, labels, opt2)
    n = model.engine.layout.n_trainable
    assert torch.equal(model.engine.flat[:n], model2.engine.flat[:n])
    assert torch.equal(opt._m[:n], opt2._m[:n]) and torch.equal(opt._v[:n], opt2._v[:n])
    assert torch.equal(opt.last_trust_ratios[1], opt2.last_trust_ratios[1])
    # a FusedAdamW checkpoint: the same two moments in the same format
    model3, _, _, adamw = fresh(FusedAdamW)
    one_step(model3, x, labels, adamw)
    model4, _, _, opt4 = fresh()
    opt4.load_state_dict(adamw.state_dict())
    assert opt4._step == 1 and torch.equal(opt4._m[:n], adamw._m[:n]) and torch.equal(opt4._v[:n], adamw._v[:n])
    assert opt4.param_groups[0]["eps"] == 1e-8 and opt4.param_groups[0]["always_adapt"] is False  # AdamW's eps came along
    one_step(model4, x, labels, opt4)
    assert opt4._step == 2 and bool(torch.isfinite(model4.engine.flat[:n]).all())


# ------------------------------------------------------------------------------------------------ 9. two ranks
def test_two_ranks_stay_bit_identical(tmp_path):
    """Two gloo ranks on the one GPU under the all-reduce exchange: every rank holds the averaged gradient, computes the same
    ratios and, after three steps, the same bits."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    child = os.path.join(ROOT, "tests", "_lamb_ddp_child.py")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), VIT_DIST_BACKEND="gloo")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, child, str(tmp_path)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[-2000:] for o in outs)
    a, b = (torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2))
    assert a["world"] == 2 and a["mode"] == "allreduce" and a["steps"] == 3
    n = a["n_trainable"]
    for key in ("params", "m", "v", "trust"):
        assert torch.equal(a[key], b[key]), key
    assert a["norms"] == b["norms"] and a["names"] == b["names"]
    assert not torch.equal(a["params"][:n], a["start"][:n]) and len(set(a["trust"].tolist())) > 10
