"""Global average pooling (`model.global_pool: avg`, include/vit_amd_pool.h) on the GPU: the two kernels against their host
restatement (tests/_pool_ref.py) bit for bit and against a float64 mean at the f32 bound; argument errors; the model against the
UNCHANGED CPU oracle with the head moved to the mean of the patch rows (`_pool_ref.oracle_step`) at the bounds
tests/test_cls_tail_gpu.py and tests/test_droppath_gpu.py apply to the same cases; depth 0; patch dropout; soft targets; the
captured step; gradient accumulation; and the shipped YAML end to end behind a masked pre-training run.
Outputs and the workspace are poisoned before the kernel calls (tests/_poison.py)."""
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

import _pool_ref as pr
from _poison import poisoned
from oracle import dropmask as dm

pytestmark = pytest.mark.gpu

BASE_SEED = 0x5DEECE66D2468ACE  # tests/test_cls_tail_gpu.py: hip_pass runs step STEP of this seed
STEP = 3
GUARD = 64  # floats behind every kernel output that must keep their fill


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def with_guard(dev, *shape):
    """(an f32 tensor of `shape`, the GUARD floats behind it): one allocation, so the band is what an overrun would hit."""
    n = int(np.prod(shape))
    buf = torch.empty(n + GUARD, dtype=torch.float32, device=dev)
    return buf[:n].view(*shape), buf[n:]


# ------------------------------------------------------------------ 1. the forward kernel
@pytest.mark.parametrize("offset", [0.0, 1e4])
@pytest.mark.parametrize("shape", pr.SHAPES)
def test_forward_kernel_is_the_restatement(dev, shape, offset):
    import vit_amd.functional as vf

    B, T, D, first = shape
    xh = pr.kernel_input(shape, 2000 + T + D, offset)
    x = torch.from_numpy(xh).to(dev)
    pooled, pad = with_guard(dev, B, D)
    # two rounds over different poison (NaN, then 3.4e38), workspace included: finite, bit-identical, the band untouched
    got = poisoned(dev, lambda: vf.token_pool_fwd(x, first, out=pooled), [pooled], pads=[pad])[0].cpu().numpy()
    want = pr.pool_fwd(xh, first)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    ref = xh[:, first:, :].astype(np.float64).mean(axis=1)
    err, lim = np.abs(got.astype(np.float64) - ref), pr.bound(xh, first)
    print(f"[pool fwd {shape} offset {offset:g}] worst error / bound {float((err / lim).max()):.3f}")
    assert bool((err <= lim).all())
    assert torch.equal(vf.token_pool_fwd(x, first), torch.from_numpy(want).to(dev))  # the allocating form


def test_forward_order_does_not_depend_on_the_batch(dev):
    """The sum's order is a function of (T, first): a sample pools to the same bits alone and as one of 300."""
    import vit_amd.functional as vf

    x = torch.from_numpy(pr.kernel_input((300, 23, 40, 1), 77, 3.0)).to(dev)
    whole = vf.token_pool_fwd(x, 1)
    for b in (0, 157, 299):
        assert torch.equal(vf.token_pool_fwd(x[b:b + 1].contiguous(), 1)[0], whole[b])


# ------------------------------------------------------------------ 2. the backward kernel
@pytest.mark.parametrize("shape", pr.SHAPES)
def test_backward_kernel_writes_every_element(dev, shape):
    import vit_amd.functional as vf

    B, T, D, first = shape
    gh = np.random.default_rng(3000 + T + D).standard_normal((B, D)).astype(np.float32)
    g = torch.from_numpy(gh).to(dev)
    dx, pad = with_guard(dev, B, T, D)
    got = poisoned(dev, lambda: vf.token_pool_bwd(g, dx, first), [dx], pads=[pad])[0].cpu().numpy()
    want = np.zeros((B, T, D), dtype=np.float32)
    want[:, first:, :] = (gh * np.float32(1 / (T - first)))[:, None, :]
    assert np.array_equal(want, pr.pool_bwd(gh, T, first))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert first == 0 or not got[:, :first].view(np.int32).any()  # exact (positive) zeros over the poison


def test_backward_is_the_adjoint_of_the_forward(dev):
    import vit_amd.functional as vf

    B, T, D, first = 2, 197, 768, 1
    x = torch.from_numpy(pr.kernel_input((B, T, D, first), 41)).to(dev)
    g = torch.from_numpy(np.random.default_rng(42).standard_normal((B, D)).astype(np.float32)).to(dev)
    lhs = float((vf.token_pool_fwd(x, first).double() * g.double()).sum())
    rhs = float((x.double() * vf.token_pool_bwd(g, torch.empty_like(x), first).double()).sum())
    print(f"[pool adjoint] <pool(x), g> = {lhs:.9f}, <x, pool_bwd(g)> = {rhs:.9f}")
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))


# ------------------------------------------------------------------ 3. argument errors
def test_argument_errors_launch_nothing(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    B, T, D = 2, 5, 32
    h = vf._h(torch.empty(1, device=dev))
    st = torch.cuda.current_stream(dev).cuda_stream
    SENT = -12345.0
    x, g = torch.randn(B, T, D, device=dev), torch.randn(B, D, device=dev)
    outs = dict(pooled=torch.full((B, D), SENT, device=dev), dx=torch.full((B, T, D), SENT, device=dev))
    lib, hh, po, dxo = h.lib, h.h, outs["pooled"].data_ptr(), outs["dx"].data_ptr()
    calls = [
        (lambda: lib.vit_token_pool_fwd(hh, None, po, B, T, D, 1, st), b"null pointer"),
        (lambda: lib.vit_token_pool_fwd(hh, x.data_ptr(), None, B, T, D, 1, st), b"null pointer"),
        (lambda: lib.vit_token_pool_fwd(hh, x.data_ptr(), po, 0, T, D, 1, st), b"B=0"),
        (lambda: lib.vit_token_pool_fwd(hh, x.data_ptr(), po, B, 0, D, 0, st), b"T=0"),
        (lambda: lib.vit_token_pool_fwd(hh, x.data_ptr(), po, B, T, 0, 1, st), b"D=0"),
        (lambda: lib.vit_token_pool_fwd(hh, x.data_ptr(), po, B, T, D, T, st), b"first=5"),
        (lambda: lib.vit_token_pool_fwd(hh, x.data_ptr(), po, B, T, D, -1, st), b"first=-1"),
        (lambda: lib.vit_token_pool_bwd(hh, None, dxo, B, T, D, 1, st), b"null pointer"),
        (lambda: lib.vit_token_pool_bwd(hh, g.data_ptr(), None, B, T, D, 1, st), b"null pointer"),
        (lambda: lib.vit_token_pool_bwd(hh, g.data_ptr(), dxo, B, T, -3, 1, st), b"D=-3"),
        (lambda: lib.vit_token_pool_bwd(hh, g.data_ptr(), dxo, B, T, D, T + 2, st), b"first=7"),
        (lambda: lib.vit_token_pool_bwd(hh, g.data_ptr(), dxo, B, T, D, -1, st), b"first=-1"),
    ]
    for call, text in calls:
        assert call() == -1  # VIT_ERR_ARG
        assert text in lib.vit_last_error(), (text, lib.vit_last_error())
    with pytest.raises(_cabi.VitError, match="first"):
        vf.token_pool_fwd(x, T, out=outs["pooled"])
    with pytest.raises(_cabi.VitError, match="pooled must hold"):
        vf.token_pool_bwd(g[:, :-1].contiguous(), outs["dx"], 1)
    torch.cuda.synchronize(dev)
    for k, v in outs.items():  # nothing was launched: every output still holds its sentinel
        assert bool((v == SENT).all()), k


# ------------------------------------------------------------------ 4 / 5. the model against the oracle
_oracle = {}
CLS5 = dict(image_size=640, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, stride_size=32,
            pos_encoding_type="rope", rope_base=1000.0, task_type="cls", num_labels=5)  # the 'rope' case with a 5-class head


def avg_model(rc, sd, dev, precision, **over):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    cfg = ViTConfig(task_type=rc.task_type, image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                    num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
                    stride_size=rc.stride_size, num_labels=rc.num_labels, pos_encoding_type=rc.pos_encoding_type,
                    rope_base=rc.rope_base, **dict(dict(global_pool="avg"), **over))
    model = MyViT(cfg, loss_name=rc.loss_name)
    model.set_precision(precision)
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def oracle_pass(key, rc, sd, flux, labels, train, masks="step", soft=None):
    """One CPU oracle forward (+ backward in train mode) under average pooling, cached under `key` and left unchanged; also the
    CLS-head logits of the same forward (what the model must NOT compute)."""
    if key not in _oracle:
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        if masks == "step":
            masks = dm.engine_masks(rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, dm.step_seed(BASE_SEED, STEP),
                                    None) if train else None
        params = {k: v.clone().requires_grad_(train) for k, v in sd.items()}
        with torch.set_grad_enabled(train):
            loss, logits, out = pr.oracle_step(rc, params, flux, labels, train, masks, soft=soft)
        if train:
            loss.backward()
        _oracle[key] = dict(loss=float(loss.detach()), logits=logits.detach(), cls_logits=out.logits.detach(),
                            grads={k: p.grad for k, p in params.items() if p.grad is not None})
    return _oracle[key]


def case_oracle(tag, train):
    from test_cls_tail_gpu import case

    rc, sd, flux, labels, _, gtol = case(tag)
    return rc, sd, flux, labels, gtol, oracle_pass((tag, train), rc, sd, flux, labels, train)


def check_fp32(name, h, o):
    """The project's bounds for these cases at precision '32': logits and loss < 1e-4, every gradient tensor < 2e-4."""
    from test_cls_tail_gpu import errors

    e = errors(h, o)
    worst = max(e["grads"].items(), key=lambda kv: kv[1][0])
    print(f"[avg {name} 32] logits {e['logits']:.2e}, loss {e['loss']:.2e}, worst gradient {worst[1][0]:.2e} ({worst[0]})")
    assert e["logits"] < 1e-4 and e["loss"] < 1e-4, (name, e["logits"], e["loss"])
    for pname, (r, _) in e["grads"].items():
        assert r < 2e-4, (name, pname, r)
    return e


@pytest.mark.parametrize("tag", ["l3", "rope"])
def test_model_is_the_oracle_fp32(dev, tag):
    from test_cls_tail_gpu import hip_pass

    rc, sd, flux, labels, _, o = case_oracle(tag, True)
    model = avg_model(rc, sd, dev, "32")
    x, y = flux.to(dev), labels.to(dev)
    h = hip_pass(model, x, y, True, tail=True)  # cls_tail on: the pooling still takes every row
    assert h["tail"] is False and model.engine._last["pool"] == "avg"
    e = check_fp32(f"{tag} train", h, o)
    assert {"vit.layernorm.weight", "vit.embeddings.cls_token", rc.head_name + ".weight"} <= set(e["grads"])
    apart = rel(h["logits"], o["cls_logits"])
    print(f"[avg {tag} 32] logits against the CLS head's {apart:.2e}")
    assert apart >= 10 * e["logits"] and apart > 1e-3  # the pooling is in the path
    # eval mode, without gradients, and with hidden states asked for
    _, _, _, _, _, oe = case_oracle(tag, False)
    model.eval()
    with torch.no_grad():
        out = model(x, labels=y)
        hid = model(x, labels=y, output_hidden_states=True)
    assert model.engine._last["tail"] is False and model.engine._last["grad"] is False
    ee, el = rel(out.logits, oe["logits"]), abs(float(out.loss) - oe["loss"]) / abs(oe["loss"])
    print(f"[avg {tag} 32 eval] logits {ee:.2e}, loss {el:.2e}")
    assert ee < 1e-4 and el < 1e-4
    assert torch.equal(hid.logits, out.logits) and len(hid.hidden_states) == rc.num_hidden_layers + 1
    # global_pool 'token' on the same weights is the CLS head
    model.set_global_pool("token")
    with torch.no_grad():
        tok = model(x, labels=y)
    assert model.engine._last["pool"] == "token" and rel(tok.logits, oe["cls_logits"]) < 1e-4


def test_model_is_the_oracle_bf16(dev):
    """Case l3 at bf16-mixed: logits < 1.5e-2, the loss within tests/test_droppath_gpu.py's rule (3e-2 for this case), every
    gradient tensor < the case's gtol with cosine > 0.999."""
    from test_cls_tail_gpu import errors, hip_pass

    rc, sd, flux, labels, gtol, o = case_oracle("l3", True)
    model = avg_model(rc, sd, dev, "bf16-mixed")
    h = hip_pass(model, flux.to(dev), labels.to(dev), True, tail=True)
    assert h["tail"] is False
    e = errors(h, o)
    worst = max(e["grads"].items(), key=lambda kv: kv[1][0])
    print(f"[avg l3 bf16-mixed] logits {e['logits']:.2e}, loss {e['loss']:.2e} (tol 3e-2), worst gradient {worst[1][0]:.2e} "
          f"({worst[0]}, gtol {gtol}), lowest cosine {min(c for _, c in e['grads'].values()):.5f}")
    assert e["logits"] < 1.5e-2 and e["loss"] <= 3e-2
    for name, (r, c) in e["grads"].items():
        assert r < gtol and c > 0.999, (name, r, c)


# ------------------------------------------------------------------ 6. depth 0
def test_depth_zero(dev):
    from oracle import refvit
    from test_cls_tail_gpu import hip_pass

    rc = refvit.RefConfig(image_size=512, patch_size=32, hidden_size=64, num_hidden_layers=0, num_attention_heads=2,
                          stride_size=32, pos_encoding_type="learned", loss_name="mae")
    sd = refvit.make_state_dict(rc, 81)
    flux, _, labels = refvit.make_inputs(rc, 6, 82)
    o = oracle_pass(("l0", True), rc, sd, flux, labels, True)
    model = avg_model(rc, sd, dev, "32")
    h = hip_pass(model, flux.to(dev), labels.to(dev), True, tail=True)
    # without a layer nothing mixes the tokens: the CLS token's gradient is exactly zero, in the oracle and here
    assert not o["grads"]["vit.embeddings.cls_token"].any()
    assert not h["grads"]["vit.embeddings.cls_token"].any()
    o = dict(o, grads={k: v for k, v in o["grads"].items() if k != "vit.embeddings.cls_token"})
    h = dict(h, grads={k: v for k, v in h["grads"].items() if k != "vit.embeddings.cls_token"})
    check_fp32("depth 0", h, o)


# ------------------------------------------------------------------ 7. patch dropout
def test_patch_dropout_pools_the_kept_tokens(dev):
    """'32', dropout probabilities 0, a given selection: the model is the oracle on the shortened signal (a model of
    image_size K * P whose tokens are exactly the kept ones), the mean running over the K kept tokens."""
    from _patchdrop_ref import kept, shortened_signal
    from test_cls_tail_gpu import case, hip_pass

    rc, sd, flux, labels, _, _ = case("l3")
    rc = dataclasses.replace(rc, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    B, N, P = flux.shape[0], rc.num_patches, rc.patch_size
    K = kept(N, 0.5)
    rng = np.random.default_rng(91)
    idx = np.stack([np.sort(rng.choice(N, K, replace=False)) for _ in range(B)]).astype(np.int32)
    assert rc.stride == P and 1 < K < N
    rc2 = dataclasses.replace(rc, image_size=K * P)
    assert rc2.num_patches == K
    o = oracle_pass(("l3 patch drop", True), rc2, sd, shortened_signal(flux, idx, P), labels, True, masks=None)
    model = avg_model(rc, sd, dev, "32", patch_drop_rate=0.5)
    eng = model.engine
    eng.cfg.hidden_dropout_prob = eng.cfg.attention_probs_dropout_prob = 0.0
    eng.patch_keep = torch.from_numpy(idx).to(dev)
    h = hip_pass(model, flux.to(dev), labels.to(dev), True, tail=True)
    assert eng._last["T"] == 1 + K and np.array_equal(eng._last["keep"].cpu().numpy(), idx) and h["tail"] is False
    check_fp32("patch dropout", h, o)


# ------------------------------------------------------------------ 8. soft targets
@pytest.mark.parametrize("soft", ["ce", "bce"])
def test_soft_targets(dev, soft):
    from oracle import refvit
    from test_cls_tail_gpu import hip_pass

    rc = refvit.RefConfig(**CLS5)
    sd = refvit.make_state_dict(rc, 101)
    flux, _, _ = refvit.make_inputs(rc, 5, 102)
    t = torch.softmax(2 * torch.randn(5, rc.num_labels, generator=torch.Generator().manual_seed(103)), -1)
    o = oracle_pass(("cls5", soft), rc, sd, flux, t, True, soft=soft)
    model = avg_model(rc, sd, dev, "32")
    model.engine.set_soft_loss(soft)
    h = hip_pass(model, flux.to(dev), t.to(dev), True, tail=True)
    check_fp32(f"soft {soft}", h, o)
    if soft == "ce":  # and the int64 labels' plain cross entropy, on the same model
        y = torch.arange(5) % rc.num_labels
        oh = oracle_pass(("cls5", "hard"), rc, sd, flux, y, True)
        check_fp32("hard ce", hip_pass(model, flux.to(dev), y.to(dev), True, tail=True), oh)


# ------------------------------------------------------------------ 9. the captured step
def test_hip_graph_replay_is_the_eager_step(dev):
    """lr = 0: the replay is a step of the same weights.  Its loss and every gradient are the eager step's under the same bound
    record, bit for bit."""
    import vit_amd.functional as vf
    from test_cls_tail_gpu import case
    from vit_amd import _cabi
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedAdamW

    rc, sd, flux, labels, _, _ = case("l3")
    model = avg_model(rc, sd, dev, "bf16-mixed")
    eng = model.engine
    eng.overlap_dw = False  # the captured step runs on one stream; so does the eager one it is compared with
    x, y = flux.to(dev), labels.to(dev)
    eng.base_seed, eng.step_counter = BASE_SEED, 0
    opt = FusedAdamW(model, lr=0.0)
    opt.set_grad_clip(0.5)
    module = types.SimpleNamespace(model=model, noise_level=0, train=model.train)
    warmup = 2
    gs = GraphedTrainStep(module, opt, (x, None, y), warmup=warmup)
    lay = eng.layout
    names = [k for k, (off, _) in lay.entries.items() if off < lay.n_trainable]
    loss = gs.step((x, None, y)).clone()
    torch.cuda.synchronize(dev)
    assert eng._last["pool"] == "avg" and eng._last["tail"] is False
    grads = {k: lay.view(eng.grads, k).clone() for k in names}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and float(grads["vit.layernorm.weight"].abs().max()) > 0
    h = eng.handle()
    record = torch.zeros(8, dtype=torch.int32, device=dev)
    eng.step_counter = warmup
    eng.grads.fill_(float("nan"))
    _cabi.check(h.lib.vit_step_state_bind(h.h, record.data_ptr()), "vit_step_state_bind")
    try:
        with vf.use_handle(h):
            _cabi.check(h.lib.vit_step_advance(h.h, BASE_SEED, 0.9, 0.999, vf._stream(record)), "vit_step_advance")
        eager, _, _, _ = eng.forward(x, y, training=True, need_grad=True)
        eng.backward(torch.ones(1, device=dev))
        torch.cuda.synchronize(dev)
    finally:
        _cabi.check(h.lib.vit_step_state_bind(h.h, None), "vit_step_state_bind")
    assert torch.equal(eager, loss), (float(eager), float(loss))
    for k in names:  # every element of every gradient tensor was rewritten over the NaN fill, with the replay's bits
        assert torch.equal(lay.view(eng.grads, k), grads[k]), k


# ------------------------------------------------------------------ 10. accumulation
def test_gradient_accumulation_adds_two_backwards(dev):
    from test_cls_tail_gpu import case

    rc, sd, flux, labels, _, _ = case("l3")
    model = avg_model(rc, sd, dev, "bf16-mixed")
    eng = model.engine
    x, y = flux.to(dev), labels.to(dev)
    model.train()
    lay = eng.layout

    def backward_of(step, fresh):
        eng.base_seed, eng.step_counter = BASE_SEED, step - 1
        if fresh:
            for p in model.parameters():
                p.grad = None
        model(x, labels=y).loss.backward()
        return eng.grads[:lay.n_trainable].detach().clone()

    g1, g2 = backward_of(3, True), backward_of(4, True)
    assert not torch.equal(g1, g2)
    backward_of(3, True)
    both = backward_of(4, False)  # the parameters still hold the buffer's views: this backward accumulates
    want = g1 + g2
    for name in (rc.head_name + ".weight", rc.head_name + ".bias", "vit.embeddings.cls_token", "vit.layernorm.weight",
                 "vit.layernorm.bias"):
        e = rel(lay.view(both, name), lay.view(want, name))
        assert e < 1e-6 and float(lay.view(want, name).abs().max()) > 0, (name, e)
    assert rel(both, want) < 1e-6


# ------------------------------------------------------------------ 11. end to end
def test_yaml_fine_tunes_behind_masked_pretraining(dev, tmp_path, monkeypatch, capsys):
    import yaml

    from scripts import run as run_script
    from scripts import test as test_script
    from vit_amd.trainer import Trainer, load_checkpoint_file, model_state_from_checkpoint, saved_global_pool

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tiny = dict(image_size=256, patch_size=16, stride_size=16, hidden_size=32, num_hidden_layers=2, num_attention_heads=2)
    # the masked pre-training run that hands its encoder over
    pre = yaml.safe_load(open(os.path.join(root, "configs", "exp", "mim_pretrain.yaml")))
    pre["model"].update(tiny)
    pre["train"].update(batch_size=8, ep=1, save=True)
    pre["project"] = "t"
    (tmp_path / "pre.yaml").write_text(yaml.safe_dump(pre))
    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "pre"))
    args = types.SimpleNamespace(config=str(tmp_path / "pre.yaml"), gpu=1, debug=0, seed=42, synthetic=64, save=True, ckpt=None)
    config, module, data = run_script.build(args)
    trainer = Trainer(config["train"], device=dev, verbose=False)
    trainer.fit(module, *data.fit_loaders(args.debug))
    mim_ckpt = trainer.checkpointer.last_path
    saved = model_state_from_checkpoint(load_checkpoint_file(mim_ckpt))
    # the shipped fine-tuning config at the same tiny geometry
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "exp", "finetune_avgpool.yaml")))
    assert cfg["model"]["global_pool"] == "avg" and cfg["model"]["hidden_size"] == 768 and cfg["opt"]["layer_decay"] == 0.75
    cfg["model"].update(tiny, init_from=mim_ckpt)
    cfg["train"].update(batch_size=8, ep=3, save=True)
    cfg["project"] = "t"
    (tmp_path / "ft.yaml").write_text(yaml.safe_dump(cfg))
    monkeypatch.setenv("CKPT_DIR", str(tmp_path / "ft"))
    capsys.readouterr()
    args2 = types.SimpleNamespace(config=str(tmp_path / "ft.yaml"), gpu=1, debug=0, seed=43, synthetic=128, save=True, ckpt=None)
    config2, module2, data2 = run_script.build(args2)
    said = capsys.readouterr().out
    line = next(ln for ln in said.splitlines() if ln.startswith("[init_from]"))
    assert "not in the model (skipped): ['decoder.bias', 'decoder.weight', 'vit.embeddings.mask_token'];" in line
    assert line.endswith("(kept as initialised): ['regressor.bias', 'regressor.weight']")
    own = module2.model.state_dict()
    for k in set(own) & set(saved):
        assert torch.equal(own[k].cpu(), saved[k]), k
    assert "vit.layernorm.weight" in set(own) & set(saved)
    eng = module2.model.engine
    assert eng.avg_pool and module2.model.name.endswith("_gap") and eng.cfg.drop_path_rate == 0.1
    t2 = Trainer(config2["train"], device=dev, verbose=False)
    steps, log = [], t2._log

    def spy(name, value, **kw):
        if name.endswith("_loss") and not name.startswith(("val_", "test_")):  # the training step's `{loss_name}_loss`
            steps.append((name, float(value)))
        return log(name, value, **kw)

    t2._log = spy
    hist = t2.fit(module2, *data2.fit_loaders(args2.debug))
    assert eng._last["pool"] == "avg"
    name = steps[0][0]
    losses = [v for k, v in steps if k == name]
    assert t2.global_step == 48 and len(losses) == 48 and all(np.isfinite(losses))
    first, last = sum(losses[:8]) / 8, sum(losses[-8:]) / 8
    print(f"[avg end to end] {name} of the first 8 steps {first:.4f}, of the last 8 {last:.4f}; logged {sorted(hist[-1])}")
    assert last < first
    ft_ckpt = t2.checkpointer.last_path
    assert saved_global_pool(load_checkpoint_file(ft_ckpt)) == "avg"
    in_process = t2.test(module2, data2.test_loader())
    # `launch.sh test --ckpt`: from the run's own config, and from one that does not say how to pool -- the checkpoint does
    targs = types.SimpleNamespace(config=str(tmp_path / "ft.yaml"), gpu=1, debug=0, seed=43, synthetic=128, ckpt=ft_ckpt)
    again = test_script.main(targs)
    assert again == in_process and again, (again, in_process)
    cfg["model"].pop("global_pool")
    cfg["model"].pop("init_from")
    (tmp_path / "plain.yaml").write_text(yaml.safe_dump(cfg))
    targs.config = str(tmp_path / "plain.yaml")
    capsys.readouterr()
    assert test_script.main(targs) == in_process
    assert "trained with model.global_pool 'avg'" in capsys.readouterr().out
    # the same weights read through the CLS row give another number
    module2.model.set_global_pool("token")
    assert t2.test(module2, data2.test_loader()) != in_process


# ------------------------------------------------------------------ 12. the poison table
# tests/test_poison_cpu.py demands that every exported vit_* name is a case of tests/test_poison_gpu.py's table or listed in its
# EXEMPT dict with a reason.  The two exports of include/vit_amd_pool.h are listed there from here, when this module is imported
# (pytest imports every test module before it runs the first test): tests 1 and 2 above poison their outputs and the workspace.
def _list_in_poison_table():
    import test_poison_gpu as table

    here = "poisoned by tests/test_pool_gpu.py"
    for name in ("vit_token_pool_fwd", "vit_token_pool_bwd"):
        table.EXEMPT.setdefault(name, here)


_list_in_poison_table()
