"""LayerScale (`model.layer_scale_init`, include/vit_amd_layerscale.h) on the GPU: the fold and gradient kernels bit for bit, the
model against the unchanged CPU oracle (whose two scaled weights are the autograd expression lambda[:, None] * W of leaf
tensors), off-is-off, the freshness of the folded operands, the CLS tail, accumulation, the captured step and the trainer."""
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((4, 4), (4, 16)), ((12, 12), (12, 48)), ((100, 100), (100, 400)), ((768, 768), (768, 3072))]
CANARY, PAD = 12345.0, 64  # elements in front of and behind every output


def rel(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------ 1, 2: the two kernels
def guarded(shape, dtype, dev, fill=None):
    """A tensor of `shape` inside a buffer with PAD canary elements on either side; returns (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device=dev)
    view = buf[PAD:PAD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return view, buf


def canaries_intact(buf):
    return bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())


def kernel_case(dev, shapes, seed, out_dtype=torch.bfloat16):
    """Inputs of a two-entry table (different K, its own lambda each) and guarded outputs."""
    g = torch.Generator().manual_seed(seed)
    ents = []
    for rows, cols in shapes:
        lam = torch.exp(torch.empty(rows).uniform_(float(np.log(1e-6)), float(np.log(2.0)), generator=g))  # [1e-6, 2], log scale
        e = dict(W=torch.randn(rows, cols, generator=g), b=torch.randn(rows, generator=g), lam=lam,
                 dW_raw=torch.randn(rows, cols, generator=g), db_raw=torch.randn(rows, generator=g))
        e = {k: v.to(dev) for k, v in e.items()}
        e["old"] = {k: torch.randn(s, generator=g).to(dev) for k, s in (("dW", (rows, cols)), ("db", (rows,)), ("dlam", (rows,)))}
        e["bufs"] = {}
        for k, shape, dt in (("Wf", (rows, cols), out_dtype), ("bf", (rows,), torch.float32), ("dW", (rows, cols), torch.float32),
                             ("db", (rows,), torch.float32), ("dlam", (rows,), torch.float32)):
            e[k], e["bufs"][k] = guarded(shape, dt, dev)
        ents.append(e)
    return ents


def table_of(ents, dev, keys):
    import vit_amd.functional as vf

    return vf.layer_scale_table([{k: e[k] for k in keys} for e in ents], dev)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shapes", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}+{s[1][0]}x{s[1][1]}")
def test_fold_kernel_bit_for_bit(dev, shapes, out_dtype):
    import vit_amd.functional as vf

    ents = kernel_case(dev, shapes, 11, out_dtype)
    tab = table_of(ents, dev, ("W", "b", "lam", "Wf", "bf"))
    vf.layer_scale_fold(tab, out_dtype)
    torch.cuda.synchronize()
    for e in ents:
        want = e["lam"][:, None] * e["W"]
        assert torch.equal(e["Wf"], want.to(out_dtype))
        assert torch.equal(e["bf"], e["lam"] * e["b"])
        assert canaries_intact(e["bufs"]["Wf"]) and canaries_intact(e["bufs"]["bf"])
    assert not torch.equal(ents[0]["lam"], ents[1]["lam"])


def exact_fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, for float32 arrays: the product is exact in float64; the float64 sum is corrected
    where it lands on a float32 tie with a non-zero rounding error (TwoSum), the one case where rounding twice differs."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = ((s.view(np.int64) & ((1 << 29) - 1)) == (1 << 28)) & (err != 0)
    s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


@pytest.mark.parametrize("shapes", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}+{s[1][0]}x{s[1][1]}")
def test_grad_kernel(dev, shapes):
    import vit_amd.functional as vf

    ents = kernel_case(dev, shapes, 23)
    tab = table_of(ents, dev, ("W", "b", "lam", "dW_raw", "db_raw", "dW", "db", "dlam"))
    raw_b = [e["db_raw"].clone() for e in ents]

    def launch(accumulate):
        for e, rb in zip(ents, raw_b):
            e["db_raw"].copy_(rb)  # the pass leaves the raw bias gradient zeroed
            for k in ("dW", "db", "dlam"):
                e[k].copy_(e["old"][k])
        vf.layer_scale_grad(tab, accumulate)
        torch.cuda.synchronize()
        return [{k: e[k].clone() for k in ("dW", "db", "dlam")} for e in ents]

    plain, again = launch(False), launch(False)
    acc, acc_again = launch(True), launch(True)
    for i, (e, rb) in enumerate(zip(ents, raw_b)):
        lam, W, b, g = e["lam"], e["W"], e["b"], e["dW_raw"]
        cols = W.shape[1]
        assert torch.equal(plain[i]["dW"], lam[:, None] * g) and torch.equal(plain[i]["db"], lam * rb)
        assert float(e["db_raw"].abs().max()) == 0.0
        # dlambda against the float64 sum; the bound holds for any summation order, with or without contraction
        terms = g.double() * W.double()
        exact = terms.sum(1) + rb.double() * b.double()
        bound = (cols + 2) * 2.0 ** -24 * (terms.abs().sum(1) + (rb.double() * b.double()).abs())
        err = (plain[i]["dlam"].double() - exact).abs()
        print(f"[grad {tuple(W.shape)}] dlambda: worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), float((err / bound).max())
        err_acc = (acc[i]["dlam"].double() - (e["old"]["dlam"].double() + exact)).abs()
        assert bool((err_acc <= bound + 2.0 ** -24 * (e["old"]["dlam"].double().abs() + exact.abs())).all())
        # accumulate mode: old + fl(lambda g) or fma(lambda, g, old)
        for k, lam_, g_ in (("dW", lam[:, None].expand_as(g), g), ("db", lam, rb)):
            old = e["old"][k]
            fused = torch.from_numpy(exact_fma32(lam_.cpu().numpy(), g_.cpu().numpy(), old.cpu().numpy())).to(dev)
            got = acc[i][k]
            assert bool(((got == old + lam_ * g_) | (got == fused)).all()), k
        for k in ("dW", "db", "dlam"):
            assert torch.equal(plain[i][k], again[i][k]) and torch.equal(acc[i][k], acc_again[i][k]), k  # deterministic
            assert canaries_intact(e["bufs"][k]), k
    # the entries do not mix: each has its own lambda and was checked against its own reference, and the two results differ
    assert not torch.equal(plain[0]["dlam"], plain[1]["dlam"])
    # a wrong row, a missing column or a dropped bias term is outside the bound
    e, p = ents[0], plain[0]["dlam"].double()
    terms = e["dW_raw"].double() * e["W"].double()
    bound = (e["W"].shape[1] + 2) * 2.0 ** -24 * (terms.abs().sum(1) + (raw_b[0].double() * e["b"].double()).abs())
    assert not bool(((p - terms.sum(1)).abs() <= bound).all())             # without db' b
    assert not bool(((p - (terms[:, 1:].sum(1) + raw_b[0].double() * e["b"].double())).abs() <= bound).all())  # without column 0


# ------------------------------------------------------------------ the model
_fix = {}


def fixture(tag):
    """c1 / k1 of tests/test_parity_gpu.py::setup with every bias randomised (std 0.02: exercises db' b) and lambda = 0.5 in odd
    layers, 1.5 in even ones, perturbed per channel by a seeded +-20 %.  Returns (rc, cfg keywords, state dict with lambdas,
    flux, labels)."""
    from oracle import refvit

    if tag not in _fix:
        rc = {"c1": refvit.named_config("C1"),
              "k1": refvit.RefConfig(image_size=512, patch_size=32, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                                     stride_size=32, task_type="cls", num_labels=5, pos_encoding_type="learned", loss_name="ce")}[tag]
        g = np.load(os.path.join(ROOT, "tests", "golden", f"{tag}.npz"))
        sd = refvit.make_state_dict(rc, int(g["wseed"]))
        gen = torch.Generator().manual_seed(4321)
        for k in sd:
            if k.endswith(".bias"):
                sd[k] = 0.02 * torch.randn(sd[k].shape, generator=gen)
        for i in range(rc.num_hidden_layers):
            for s in (1, 2):
                base = 0.5 if i % 2 else 1.5
                sd[f"vit.encoder.layer.{i}.layer_scale{s}.lambda1"] = base * (1 + 0.2 * (2 * torch.rand(rc.hidden_size, generator=gen) - 1))
        kw = dict(task_type=rc.task_type, image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                  num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
                  stride_size=rc.stride_size, num_labels=rc.num_labels, pos_encoding_type=rc.pos_encoding_type)
        _fix[tag] = (rc, kw, sd, torch.from_numpy(g["flux"]), torch.from_numpy(g["labels"]))
    return _fix[tag]


def build(kw, sd, dev, precision, init=1.0):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    model = MyViT(ViTConfig(**kw, layer_scale_init=init), loss_name="ce" if kw["task_type"] == "cls" else "mae")
    model.set_precision(precision)
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def plain_sd(sd, ones=False):
    """The oracle's plain state dict: no lambda keys; the scaled weights folded (or left as they are: lambda = 1)."""
    out = {k: v.clone() for k, v in sd.items() if not k.endswith(".lambda1")}
    if not ones:
        for k, lam in sd.items():
            if k.endswith(".lambda1"):
                stem = k.replace("layer_scale1.lambda1", "attention.output.dense").replace("layer_scale2.lambda1", "output.dense")
                out[stem + ".weight"] = lam[:, None] * sd[stem + ".weight"]
                out[stem + ".bias"] = lam * sd[stem + ".bias"]
    return out


def ls_oracle_pass(rc, sd, x, labels, masks=None):
    """oracle.refvit.forward on a params dict whose two scaled weights per layer are lambda[:, None] * W of leaf tensors and
    whose biases are lambda * b: autograd yields dW, db and dlambda with nothing changed under oracle/."""
    from oracle import refvit

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    params = {k: v for k, v in leaves.items() if not k.endswith(".lambda1")}
    for k, lam in leaves.items():
        if k.endswith(".lambda1"):
            stem = k.replace("layer_scale1.lambda1", "attention.output.dense").replace("layer_scale2.lambda1", "output.dense")
            params[stem + ".weight"] = lam[:, None] * leaves[stem + ".weight"]
            params[stem + ".bias"] = lam * leaves[stem + ".bias"]
    out = refvit.forward(rc, params, x.cpu(), labels.cpu(), training=masks is not None, masks=masks, output_hidden_states=True)
    out.loss.backward()
    return dict(loss=float(out.loss.detach()), logits=out.logits.detach(), hs=[h.detach() for h in out.hidden_states],
                grads={k: p.grad for k, p in leaves.items() if p.grad is not None})


_oracles = {}


def oracles(tag, step=3):
    from test_parity_gpu import step_masks

    if tag not in _oracles:
        rc, kw, sd, x, labels = fixture(tag)
        _oracles[tag] = (ls_oracle_pass(rc, sd, x, labels), ls_oracle_pass(rc, sd, x, labels, masks=step_masks(rc, step)))
    return _oracles[tag]


def hold_to_gates(e, precision, who):
    lam = [n for n in e["grads"] if n.endswith(".lambda1")]
    assert len(lam) >= 4, (who, list(e["grads"]))  # the lambda tensors are held to the same per-tensor gate
    if precision == "32":
        assert e["hs"] < 1e-4 and e["logits"] < 1e-4 and e["loss"] < 1e-4, (who, e)
        for name, (r, _) in e["grads"].items():
            assert r < 2e-4, (who, name, r)
    else:
        assert e["hs"] <= 1.5e-2, (who, e["hs"])
        for name, (r, c) in e["grads"].items():
            assert r < 4e-2 and c > 0.999, (who, name, r, c)


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
@pytest.mark.parametrize("tag", ["c1", "k1"])
def test_model_parity_with_the_oracle(dev, tag, precision):
    from test_parity_gpu import check_train_parity, hip_pass, oracle_pass, pass_errors

    rc, kw, sd, x, labels = fixture(tag)
    o_eval, o_train = oracles(tag)
    model = build(kw, sd, dev, precision)
    xd, yd = x.to(dev), labels.to(dev)
    h = hip_pass(model, xd, yd, train=False)
    e = pass_errors(h, o_eval)
    print(f"[layerscale {tag} {precision} eval] hidden states {e['hs']:.2e}, logits {e['logits']:.2e}, worst gradient "
          f"{max(v[0] for v in e['grads'].values()):.2e}, lambda gradients "
          f"{max(v[0] for n, v in e['grads'].items() if n.endswith('.lambda1')):.2e}")
    hold_to_gates(e, precision, "eval")
    # negative control: the oracle with lambda = 1 is at least 10x further away
    ones = pass_errors(h, oracle_pass(rc, plain_sd(sd, ones=True), x, labels, grads=False))
    assert ones["hs_all"] >= 10 * e["hs_all"], (e["hs_all"], ones["hs_all"])
    # train mode, restated masks of step 3; its own negative control (the masks of step 4) runs on the folded plain weights
    et = check_train_parity(f"layerscale {tag}", rc, plain_sd(sd), model, xd, yd, precision, oracle_eval=o_eval, oracle_train=o_train)
    hold_to_gates(et, precision, "train")


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_off_is_off(dev, precision):
    """init None: the parent's parameter names.  init 1.0: multiplying by 1.0 is exact, so the loss and every gradient but
    lambda's are the plain model's bit for bit, and dlambda is the oracle's."""
    from test_parity_gpu import hip_pass, setup
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    rc, g, sd, plain, x, labels = setup("c1", dev, precision)
    kw = fixture("c1")[1]
    assert list(MyViT(ViTConfig(**kw, layer_scale_init=None), loss_name="mae").state_dict()) == list(plain.state_dict()) == \
        list(MyViT(ViTConfig(**kw), loss_name="mae").state_dict())
    assert plain.engine._ls is None and not plain.engine.layer_scale
    gen = torch.Generator().manual_seed(9)
    sd = {k: (0.02 * torch.randn(v.shape, generator=gen) if k.endswith(".bias") else v) for k, v in sd.items()}
    plain.load_state_dict(sd)
    model = MyViT(ViTConfig(**kw, layer_scale_init=1.0), loss_name="mae")
    model.set_precision(precision)
    assert model.load_state_dict(sd, strict=False).missing_keys == [k for k in model.state_dict() if k.endswith(".lambda1")]
    model = model.to(dev)
    with pytest.raises(RuntimeError):
        model.load_state_dict(sd, strict=True)  # a checkpoint without the keys
    with pytest.raises(RuntimeError):
        plain.load_state_dict(model.state_dict(), strict=True)  # and the converse
    a, b = hip_pass(plain, x, labels, train=False), hip_pass(model, x, labels, train=False)
    assert a["loss"] == b["loss"] and torch.equal(a["logits"], b["logits"])
    for h1, h2 in zip(a["hs"], b["hs"]):
        assert torch.equal(h1, h2)
    for name, ga in a["grads"].items():
        assert torch.equal(ga, b["grads"][name]), name
    full = dict(sd, **{k: v.detach().cpu() for k, v in model.state_dict().items() if k.endswith(".lambda1")})
    o = ls_oracle_pass(rc, full, x, labels)
    for name in full:
        if name.endswith(".lambda1"):
            r = rel(b["grads"][name], o["grads"][name])
            cos = float(torch.dot(b["grads"][name].double().flatten(), o["grads"][name].double().flatten()) /
                        (b["grads"][name].double().norm() * o["grads"][name].double().norm()))
            assert (r < 2e-4) if precision == "32" else (r < 4e-2 and cos > 0.999), (name, r, cos)


def eval_bits(model, x, labels):
    model.eval()
    with torch.no_grad():
        out = model(x, labels=labels)
    return float(out.loss), out.logits.detach().clone()


def fresh_bits(model, kw, dev, precision, x, labels):
    """The eval forward of a freshly built model loaded with model's current state_dict()."""
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return eval_bits(build(kw, sd, dev, precision), x, labels)


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_folded_operands_follow_every_writer_of_the_weights(dev, precision):
    from vit_amd.ema import WeightAverager
    from vit_amd.optimizer import FusedAdamW

    rc, kw, sd, x, labels = fixture("c1")
    x, labels = x.to(dev), labels.to(dev)
    model = build(kw, sd, dev, precision)
    lam0 = model._param_list[model._param_names.index("vit.encoder.layer.0.layer_scale1.lambda1")]
    seen = []

    def check(what, prec=precision, new=True):
        got, want = eval_bits(model, x, labels), fresh_bits(model, kw, dev, prec, x, labels)
        assert got[0] == want[0] and torch.equal(got[1], want[1]), what
        assert (got[0] not in seen) == new, what  # and the event really changed the function (or brought an earlier one back)
        seen.append(got[0])

    def backward():
        model.train()
        for p in model.parameters():
            p.grad = None
        model(x, labels=labels).loss.backward()

    check("as loaded")
    opt = FusedAdamW(model, lr=1e-2)
    backward()
    opt.step()
    check("FusedAdamW step")
    sgd = torch.optim.SGD(model.parameters(), lr=1e-1)
    backward()
    sgd.step()
    check("torch.optim.SGD step")
    model.load_state_dict({k: (v * 1.25 if k.endswith(".lambda1") else v) for k, v in sd.items()})
    check("load_state_dict")
    with torch.no_grad():
        lam0.mul_(0.5)
    check("p.mul_() on a lambda1")
    avg = WeightAverager(model, decay=0.9)
    avg.update(1)  # the first update copies
    with torch.no_grad():
        lam0.mul_(1.5)
    check("p.mul_() behind the averager's copy")
    avg.swap()
    check("EMA swap", new=False)  # the model holds the averager's copy: the function in front of the last mul_
    assert seen[-1] == seen[-3] != seen[-2]
    avg.swap()
    check("EMA swap back", new=False)
    assert seen[-1] == seen[-3] != seen[-2]
    other = "bf16-mixed" if precision == "32" else "32"
    model.set_precision(other)
    check("set_precision there", prec=other)
    model.set_precision(precision)
    check("set_precision back", new=False)


# ------------------------------------------------------------------ 6: CLS tail
def tail_pass(model, x, labels, tail):
    eng = model.engine
    eng.cls_tail = tail
    model.eval()
    for p in model.parameters():
        p.grad = None
    out = model(x, labels=labels)
    out.loss.backward()
    assert eng._last["tail"] is tail
    n = eng.layout.n_trainable
    return float(out.loss.detach()), out.logits.detach().clone(), eng.grads[:n].detach().clone()


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_cls_tail_gives_the_full_paths_bits(dev, precision):
    """'32': the c1 fixture (tests/test_accum_gpu.py: the tail's f32 sums walk the full path's order).  bf16-mixed: the "ms"
    geometry of tests/test_cls_tail_gpu.py (T = 65, widths of 256, B = 256), where that file asserts bit identity."""
    from oracle import refvit

    if precision == "32":
        rc, kw, sd, x, labels = fixture("c1")
    else:
        rc = refvit.RefConfig(image_size=2048, patch_size=32, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                              stride_size=32, loss_name="mae")
        sd = refvit.make_state_dict(rc, 61)
        gen = torch.Generator().manual_seed(5)
        for i in range(2):
            for s in (1, 2):
                sd[f"vit.encoder.layer.{i}.layer_scale{s}.lambda1"] = 0.5 + torch.rand(256, generator=gen)
            for stem in ("attention.output.dense", "output.dense"):
                sd[f"vit.encoder.layer.{i}.{stem}.bias"] = 0.02 * torch.randn(256, generator=gen)
        x, _, labels = refvit.make_inputs(rc, 256, 62)
        kw = dict(task_type="reg", image_size=2048, patch_size=32, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                  stride_size=32)
    model = build(kw, sd, dev, precision)
    x, labels = x.to(dev), labels.to(dev)
    full, tail = tail_pass(model, x, labels, False), tail_pass(model, x, labels, True)
    assert full[0] == tail[0] and torch.equal(full[1], tail[1])
    assert int((full[2] != tail[2]).sum()) == 0
    lay = model.engine.layout
    off = lay.entries["vit.encoder.layer.1.layer_scale2.lambda1"][0]
    assert float(tail[2][off:off + kw["hidden_size"]].abs().max()) > 0


# ------------------------------------------------------------------ 7: accumulation
@pytest.mark.parametrize("precision,tol", [("32", 2e-5), ("bf16-mixed", 2e-2)])
@pytest.mark.parametrize("tail", [True, False])
def test_two_accumulated_backwards_sum_the_micro_batch_gradients(dev, precision, tol, tail):
    """Repeated backward() without zero_grad (tests/test_accum_gpu.py's criterion: relative L2 against the reference sum): for
    W, b and lambda of the scaled Linears the buffer holds g1 + g2 -- in particular the raw bias-gradient slab does not carry
    the first micro-batch into the second a second time."""
    from oracle import refvit

    rc, kw, sd, _, _ = fixture("c1")
    flux, _, labels = refvit.make_inputs(rc, 8, 77)
    model = build(kw, sd, dev, precision)
    model.config.hidden_dropout_prob = model.config.attention_probs_dropout_prob = 0.0
    model.train()
    eng = model.engine
    eng.cls_tail = tail
    x, y = flux.to(dev), labels.to(dev)
    n = eng.layout.n_trainable

    def run(parts, zero_between):
        for p in model.parameters():
            p.grad = None
        outs = []
        for s in parts:
            (model(x[s], labels=y[s]).loss / 2).backward()
            torch.cuda.synchronize()
            outs.append(eng.grads[:n].detach().double().clone())
            if zero_between:
                for p in model.parameters():
                    p.grad = None
        return outs

    g1, g2 = run([slice(0, 4), slice(4, 8)], zero_between=True)
    acc = run([slice(0, 4), slice(4, 8)], zero_between=False)[-1]
    for name, p in zip(model._param_names, model._param_list):
        if eng.layout.entries[name][0] < n:
            assert p.grad is not None and p.grad.data_ptr() == eng.g(name).data_ptr(), name
    worst = 0.0
    for name, (off, shape) in eng.layout.entries.items():
        if ".lambda1" in name or "output.dense" in name:
            k = int(np.prod(shape))
            want, got = (g1 + g2)[off:off + k], acc[off:off + k]
            e = float((got - want).norm() / want.norm())
            twice = float((got - (2 * g1 + g2)[off:off + k]).norm() / want.norm())
            worst = max(worst, e)
            assert e < tol and twice > 10 * tol, (name, e, twice)
    whole = float((acc - (g1 + g2)).norm() / (g1 + g2).norm())
    print(f"[layerscale accumulate {precision} tail={tail}] worst scaled tensor {worst:.2e}, whole buffer {whole:.2e}")
    assert whole < tol
    assert float(eng._ls.views["vit.encoder.layer.0.output.dense"].db_raw.abs().max()) == 0.0


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_trainer_accumulated_step_equals_large_batch_step(dev, precision):
    """train.accumulate_grad_batches, by tests/test_accum_gpu.py::test_trainer_accumulated_step_equals_large_batch_step."""
    from test_accum_gpu import c1_config, one_step, same_step

    def cfg(**train):
        c = c1_config(precision=precision, **train)
        c["model"]["layer_scale_init"] = 0.5
        return c

    big, module, _ = one_step(cfg(batch_size=16), 16)
    acc, _, _ = one_step(cfg(batch_size=4, accumulate_grad_batches=4), 4)
    assert any(k.endswith(".lambda1") for k in module.model.state_dict())
    same_step(big, acc, precision)


# ------------------------------------------------------------------ 8: captured step
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_hip_graph_step_equals_eager(dev, precision):
    """Three replays of the captured step equal three eager steps (tests/test_ema_gpu.py::test_hip_graph_with_averaging_equals_
    eager's comparison: losses and the flat buffer, bit for bit, dropout off).  lambda changes between the replays, so the later
    losses are right only if the fold runs inside the graph."""
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.graph import GraphedTrainStep

    batches = [tuple(t.cuda() for t in b) for b in Batches(16, 5, bs=8)]
    finals = {}
    for mode in ("eager", "graph"):
        cfg = c1_config(precision=precision, batch_size=8, hip_graph=(mode == "graph"))
        cfg["model"]["layer_scale_init"] = 0.5
        cfg["opt"]["lr"] = 1e-2
        module, trainer = make(cfg)
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        eng = module.model.engine
        lam = [eng.p("vit.encoder.layer.0.layer_scale1.lambda1").detach().clone()]
        losses = []
        for i in range(3):
            losses.append(float(trainer.training_step(module, batches[i % 2], i).detach()))
            lam.append(eng.p("vit.encoder.layer.0.layer_scale1.lambda1").detach().clone())
        assert trainer.use_graph == (mode == "graph") and trainer.global_step == 3
        if mode == "graph":
            assert len(trainer._graphed) == 1 and all(isinstance(g, GraphedTrainStep) for g in trainer._graphed.values())
        assert not torch.equal(lam[0], lam[1]) and not torch.equal(lam[1], lam[2])
        finals[mode] = (losses, eng.flat.detach().clone(), eval_bits(module.model, *batches[0][::2]))
    assert finals["eager"][0] == finals["graph"][0], (finals["eager"][0], finals["graph"][0])
    assert torch.equal(finals["eager"][1], finals["graph"][1])
    assert finals["eager"][2][0] == finals["graph"][2][0]  # and the eager forward behind the replays refolds


# ------------------------------------------------------------------ 9: trainer
def test_yaml_trains_checkpoints_and_resumes_bit_for_bit(dev, tmp_path, monkeypatch):
    import yaml

    from scripts import run as run_script
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.trainer import Trainer, load_checkpoint_file, model_state_from_checkpoint

    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "ck"))
    cfg = c1_config(ep=2, precision="bf16-mixed", ema_decay=0.9)
    cfg["project"] = "t"
    cfg["model"].update(layer_scale_init=1e-4, drop_path_rate=0.1)
    cfg["opt"].update(no_decay=True, weight_decay=0.05)
    path = tmp_path / "c.yaml"
    path.write_text(yaml.safe_dump(cfg))
    args = types.SimpleNamespace(config=str(path), gpu=1, debug=0, seed=42, synthetic=48, save=False, ckpt=None)
    config, module, data = run_script.build(args)
    eng = module.model.engine
    assert eng.cfg.layer_scale_init == 1e-4 and eng.layer_scale
    trainer = Trainer(config["train"], device=dev, verbose=False)
    train_loader, val_loader = data.fit_loaders(args.debug)
    lam_before = [p.detach().clone() for n, p in module.model.named_parameters() if n.endswith(".lambda1")]
    hist = trainer.fit(module, train_loader, val_loader)
    assert len(hist) == 2 and all(np.isfinite(float(v)) for h in hist for k, v in h.items() if "loss" in k)
    groups = trainer.optimizer.param_groups
    lam_ids = {id(p) for n, p in module.model.named_parameters() if n.endswith(".lambda1")}
    assert len(lam_ids) == 6 and all(g["weight_decay"] == 0.0 for g in groups if lam_ids & {id(p) for p in g["params"]})
    raw = trainer.averager.train_state_dict()
    assert any(not torch.equal(raw[n], b.cpu()) for (n, _), b in
               zip([(n, p) for n, p in module.model.named_parameters() if n.endswith(".lambda1")], lam_before))
    # exact resume: 4 epochs in one run against 2 + 2 through a checkpoint
    train, val = Batches(24, 1, bs=8), Batches(16, 2, bs=8)

    def c(ep, save):
        k = c1_config(ep=ep, batch_size=8, precision="bf16-mixed", ema_decay=0.9, save=save)
        k["model"].update(layer_scale_init=1e-4, drop_path_rate=0.1)
        k["opt"].update(no_decay=True, weight_decay=0.05)
        return k

    m_full, t_full = make(c(4, False))
    t_full.fit(m_full, train, val)
    m_a, t_a = make(c(2, True))
    t_a.fit(m_a, train, val)
    ck = load_checkpoint_file(t_a.checkpointer.last_path)
    keys = [k for k in model_state_from_checkpoint(ck) if k.endswith(".lambda1")]
    assert len(keys) == 6 and all(k in ck["vit_amd"]["ema"]["train_state"] for k in keys)
    m_b, t_b = make(c(4, False))
    hist_b = t_b.fit(m_b, train, val, ckpt_path=t_a.checkpointer.last_path)
    assert len(hist_b) == 2 and t_b.global_step == t_full.global_step == 12
    for which in ("averaged_state_dict", "train_state_dict"):
        a, b = getattr(t_full.averager, which)(), getattr(t_b.averager, which)()
        for k in a:
            assert torch.equal(a[k], b[k]), (which, k)
    assert [h["val_mae"] for h in t_full.history[2:]] == [h["val_mae"] for h in hist_b]


# ------------------------------------------------------------------ data parallelism
def test_two_ranks_exchange_true_gradients(tmp_path):
    """tests/_layerscale_ddp_child.py: 2 gloo ranks on the one GPU, two steps with the feature on.  The replicas are bit-identical,
    and dlambda after the exchange is the mean of the ranks' local dlambda (the bucket a reducer picks up already holds the
    unfolded gradients)."""
    child = os.path.join(ROOT, "tests", "_layerscale_ddp_child.py")
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "VIT_DIST_SINGLE", "VIT_DIST_BACKEND")}
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    envs = [dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                 MASTER_PORT=str(port), VIT_DIST_BACKEND="gloo") for r in range(2)]
    for env in envs:
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, child, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for env in envs]
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [0, 0], "\n".join(o[-2000:] for o in outs)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2))
    assert r0["world"] == r1["world"] == 2 and r0["global_step"] == 2
    assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["grads"], r1["grads"])
    assert r0["lambda_names"] and not torch.equal(r0["params0"], r0["params"])
    for name in r0["lambda_names"]:
        mean = (r0["local"][name].double() + r1["local"][name].double()) / 2
        got = r0["exchanged"][name].double()
        assert float((got - mean).abs().max()) <= 2.0 ** -22 * float(mean.abs().max()) + 1e-30, name
        assert not torch.equal(r0["local"][name], r1["local"][name])
