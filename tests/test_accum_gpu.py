"""Gradient accumulation over micro-batches, in place in the flat gradient buffer.

(a) the writer contract of vit_handle_set_option("grad_accumulate"): every producer of a parameter gradient stores old + new,
    new being bit for bit what overwrite mode stores;
(b) the PyTorch idiom at model level: K backward() calls without zero_grad() leave the gradient of the whole batch;
(c) a mixed `.grad` state is an error; zero_grad(set_to_none=False) is not;
(d) - (h) `train.accumulate_grad_batches` in the trainer: one step equals the large-batch step, bookkeeping, K = 1 changes
    nothing, dropout streams, data parallelism (two gloo ranks on the one GPU), hip_graph falls back to eager launches.

Micro-batches always have EQUAL sizes here: the loss is a mean over the batch, and the mean of K means is the mean over all
samples only then (Lightning's accumulate_grad_batches has the same property)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ULP2 = 2.0 ** -22  # two f32 ulps (relative): the issue's bound for old + new


def randn(shape, dev, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


# ------------------------------------------------------------------------------------------------ (a) writer contract
def writer_contract(dev, run, outs, tag):
    """`run()` launches one producer that writes the f32 tensors `outs`.  Overwrite -> prefill + accumulate (twice, from the same
    prefill) -> overwrite again."""
    from vit_amd import _cabi

    h = _cabi.handle_for(dev)
    for o in outs:
        o.fill_(float("nan"))
    run()
    plain = [o.clone() for o in outs]
    assert all(torch.isfinite(p).all() for p in plain), tag
    pre = [randn(o.shape, dev, 1000 + i) for i, o in enumerate(outs)]
    got = []
    h.set_option("grad_accumulate", 1)
    try:
        for _ in range(2):
            for o, p in zip(outs, pre):
                o.copy_(p)
            run()
            got.append([o.clone() for o in outs])
    finally:
        h.set_option("grad_accumulate", 0)
    for o in outs:
        o.fill_(float("nan"))
    run()
    worst = 0.0
    for i, (p, q, a, b, o) in enumerate(zip(plain, pre, got[0], got[1], outs)):
        assert torch.equal(o, p), f"{tag}: output {i} does not overwrite again after the option was cleared"
        assert torch.equal(a, b), f"{tag}: output {i}: two accumulate runs from the same prefill differ"
        want = q.double() + p.double()
        bound = ULP2 * torch.maximum(torch.maximum(q.abs(), p.abs()), a.abs()).double()
        err = (a.double() - want).abs()
        assert bool((err <= bound).all()), (tag, i, float((err - bound).max()))
        assert not torch.equal(a, p), f"{tag}: output {i} was overwritten in accumulate mode"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"[writer {tag}] worst |out - (prefill + plain)| / bound = {worst:.3f}")


@pytest.mark.parametrize("colsum", [True, False])
@pytest.mark.parametrize("rows,n,dtype,split_k", [(258, 32, torch.bfloat16, -1), (258, 32, torch.float32, -1),
                                                  (1024, 256, torch.bfloat16, -1), (1024, 256, torch.bfloat16, 1)])
def test_writer_gemm_weight_gradient(dev, rows, n, dtype, split_k, colsum):
    """dW = dY^T X through vit_gemm (generic core, bf16 and x3; ping-pong core with and without split-K), with colsum_out on --
    the issue's cases -- and off (the paths a training step takes: slab reduction / the epilogue's residual port)."""
    from vit_amd import functional as vf

    dy, x = randn((rows, n), dev, 1, dtype=dtype), randn((rows, n), dev, 2, dtype=dtype)
    dW = torch.empty((n, n), dtype=torch.float32, device=dev)
    cs = torch.empty(n, dtype=torch.float32, device=dev)

    def run():
        vf.gemm(dy, x, M=n, N=n, K=rows, a_trans=True, b_trans=True, out=dW, split_k=split_k, colsum_out=cs if colsum else None)

    writer_contract(dev, run, [dW, cs] if colsum else [dW], f"gemm dW {rows}->{n}x{n} {dtype} split_k={split_k} colsum={colsum}")


@pytest.mark.parametrize("rows,n,split_k", [(258, 32, -1), (258, 32, 1), (1024, 256, -1), (1024, 256, 1)])
def test_writer_gemm_weight_gradient_scaled(dev, rows, n, split_k):
    """alpha != 1: the product is scaled first and the old C added last, in the slab reduction and through the residual port
    alike, so `new` is still the overwrite value bit for bit."""
    from vit_amd import functional as vf

    dy, x = randn((rows, n), dev, 21, dtype=torch.bfloat16), randn((rows, n), dev, 22, dtype=torch.bfloat16)
    dW = torch.empty((n, n), dtype=torch.float32, device=dev)
    writer_contract(dev, lambda: vf.gemm(dy, x, M=n, N=n, K=rows, a_trans=True, b_trans=True, out=dW, split_k=split_k, alpha=0.37),
                    [dW], f"gemm dW {rows}->{n}x{n} alpha=0.37 split_k={split_k}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_activation_gradient_products_never_accumulate(dev, dtype):
    """A dX-form product (a_trans = 0) with an f32 C -- every dX of precision '32' -- is overwritten under the option; its
    colsum_out (a bias gradient) accumulates."""
    from vit_amd import _cabi
    from vit_amd import functional as vf

    dy, w = randn((258, 64), dev, 3, dtype=dtype), randn((64, 32), dev, 4, dtype=dtype)
    dx = torch.empty((258, 32), dtype=torch.float32, device=dev)
    cs = torch.empty(32, dtype=torch.float32, device=dev)
    run = lambda: vf.gemm(dy, w, M=258, N=32, K=64, b_trans=True, out=dx, colsum_out=cs)  # noqa: E731
    run()
    plain, plain_cs = dx.clone(), cs.clone()
    h = _cabi.handle_for(dev)
    h.set_option("grad_accumulate", 1)
    try:
        dx.fill_(7.0)
        cs.fill_(7.0)
        run()
    finally:
        h.set_option("grad_accumulate", 0)
    assert torch.equal(dx, plain)
    assert torch.equal(cs, 7.0 + plain_cs)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_writer_dw_rows_and_colsum_rows(dev, dtype):
    from vit_amd import functional as vf

    dy, x = randn((4, 256), dev, 5, dtype=dtype), randn((4, 256), dev, 6, dtype=dtype)
    dW = torch.empty((256, 256), dtype=torch.float32, device=dev)
    cs = torch.empty(256, dtype=torch.float32, device=dev)
    writer_contract(dev, lambda: vf.linear_bwd_dw_rows(dy, x, dW, row_stride=64, full_rows=256), [dW], f"dw_rows {dtype}")
    writer_contract(dev, lambda: vf.colsum_rows(dy, cs, row_stride=64, full_rows=256), [cs], f"colsum_rows {dtype}")


@pytest.mark.parametrize("rows,D,stride", [(258, 32, 129), (1024, 256, 64)])
def test_writer_layernorm_backwards(dev, rows, D, stride):
    from vit_amd import functional as vf

    x, gamma, beta = randn((rows, D), dev, 7), 1 + 0.1 * randn((D,), dev, 8), randn((D,), dev, 9)
    _, mean, rstd = vf.layernorm_fwd(x, gamma, beta, 1e-12)
    dy, dres = randn((rows, D), dev, 10, dtype=torch.bfloat16), randn((rows, D), dev, 11)
    dx, dyn = torch.empty_like(x), torch.empty((rows, D), dtype=torch.bfloat16, device=dev)
    dg, db, dbias = (torch.empty(D, dtype=torch.float32, device=dev) for _ in range(3))
    writer_contract(dev, lambda: vf.layernorm_bwd(dy, x, gamma, mean, rstd, dres=dres, dx=dx, dgamma=dg, dbeta=db), [dg, db],
                    f"layernorm_bwd {rows}x{D}")
    drop = (0.1, 1234, 5)
    writer_contract(dev, lambda: vf.layernorm_bwd_fused(dy, x, gamma, mean, rstd, dres, dx, dg, db, dyn, dbias, drop),
                    [dg, db, dbias], f"layernorm_bwd_fused {rows}x{D}")
    # the rows form: both ends of a compact run -- every `stride`-th row held compactly, and a compact residual gradient
    c = rows // stride
    xc, dyc, dresc = x[::stride].contiguous(), dy[::stride].contiguous(), dres[::stride].contiguous()
    meanc, rstdc = mean[::stride].contiguous(), rstd[::stride].contiguous()
    dxc, dync = torch.empty_like(xc), torch.empty((c, D), dtype=torch.bfloat16, device=dev)
    writer_contract(dev, lambda: vf.layernorm_bwd_rows(dyc, xc, gamma, meanc, rstdc, dresc, dxc, dg, db, dyn=dync, dbias=dbias,
                                                       dropout=drop, row_stride=stride, full_rows=rows),
                    [dg, db, dbias], f"layernorm_bwd_rows compact {rows}x{D}/{stride}")
    writer_contract(dev, lambda: vf.layernorm_bwd_rows(dy, x, gamma, mean, rstd, dresc, dx, dg, db, dyn=dyn, dbias=dbias,
                                                       dropout=drop, dres_row_stride=stride),
                    [dg, db, dbias], f"layernorm_bwd_rows compact dres {rows}x{D}/{stride}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,H,T,dh", [(2, 2, 129, 16), (1, 2, 197, 64)])
def test_writer_attention_bwd_colsum(dev, B, H, T, dh, dtype):
    from vit_amd import functional as vf

    qkv = randn((B * T, 3 * H * dh), dev, 12, dtype=dtype)
    dctx = randn((B * T, H * dh), dev, 13, dtype=dtype)
    ctx, lse = vf.attention_fwd(qkv, B, H, T, dh, dh ** -0.5)
    cs = torch.empty(3 * H * dh, dtype=torch.float32, device=dev)
    dqkv = torch.empty_like(qkv)
    writer_contract(dev, lambda: vf.attention_bwd(qkv, ctx, dctx, lse, B, H, T, dh, dh ** -0.5, dqkv=dqkv, colsum_out=cs), [cs],
                    f"attention_bwd colsum B{B} H{H} T{T} dh{dh} {dtype}")


def test_writer_embed_finish_bwd(dev):
    from vit_amd import functional as vf

    B, T, D = 3, 129, 32
    dtok = randn((B, T, D), dev, 14)
    dcls, dpos = torch.empty(D, dtype=torch.float32, device=dev), torch.empty((T, D), dtype=torch.float32, device=dev)
    writer_contract(dev, lambda: vf.embed_finish_bwd(dtok, dcls, dpos, dropout=(0.1, 99, 0)), [dcls, dpos], "embed_finish_bwd")


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", ["mse", "l1", "ce"])
def test_writer_head_loss_bwd(dev, kind, C):
    from vit_amd import functional as vf

    B, T, D = 5, 3, 32
    loss_kind = {"mse": vf.LOSS_MSE, "l1": vf.LOSS_L1, "ce": vf.LOSS_CE}[kind]
    last, W, b = randn((B, T, D), dev, 15), randn((C, D), dev, 16), randn((C,), dev, 17)
    g = torch.Generator().manual_seed(18)
    labels = (torch.randint(0, C, (B,), generator=g) if kind == "ce" else torch.rand((B, C), generator=g)).to(dev)
    logits, _ = vf.head_loss_fwd(last, W, b, labels, loss_kind)
    dloss = torch.ones(1, dtype=torch.float32, device=dev)
    dW, db, dlast = torch.empty_like(W), torch.empty_like(b), torch.empty_like(last)
    writer_contract(dev, lambda: vf.head_loss_bwd(last, W, logits, labels, dloss, loss_kind, dlast=dlast, dW=dW, db=db), [dW, db],
                    f"head_loss_bwd {kind} C={C}")


# ------------------------------------------------------------------------------------------------ (b) the PyTorch idiom
_cases = {}


def fixture_case(tag):
    """Configuration and seeded weights of the fixtures c1 / k1 (learned position embedding; also the classification fixture:
    cross-entropy) / conv (C1D), 8 seeded samples, and the CPU oracle's gradient of the whole batch (computed once)."""
    from oracle import refvit

    if tag not in _cases:
        rc = {"c1": refvit.named_config("C1"),
              "k1": refvit.RefConfig(image_size=512, patch_size=32, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                                     stride_size=32, task_type="cls", num_labels=5, pos_encoding_type="learned", loss_name="ce"),
              "conv": refvit.RefConfig(image_size=1024, patch_size=32, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                                       stride_size=32, proj_fn="C1D", loss_name="mae")}[tag]
        g = np.load(os.path.join(GOLD, f"{tag}.npz"))
        sd = refvit.make_state_dict(rc, int(g["a_wseed" if tag == "conv" else "wseed"]))
        flux, _, labels = refvit.make_inputs(rc, 8, 77)
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        refvit.forward(rc, params, flux, labels, training=False).loss.backward()
        _cases[tag] = (rc, sd, flux, labels, {k: p.grad for k, p in params.items() if p.grad is not None})
    return _cases[tag]


def build(rc, sd, dev, precision):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    cfg = ViTConfig(task_type=rc.task_type, image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                    num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
                    stride_size=rc.stride_size, num_labels=rc.num_labels, pos_encoding_type=rc.pos_encoding_type)
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    model = MyViT(cfg, loss_name=rc.loss_name)
    model.set_precision(precision)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).train()


def trainable(model):
    lay = model.engine.layout
    return [(n, p) for n, p in zip(model._param_names, model._param_list) if lay.entries[n][0] < lay.n_trainable]


def accumulate(model, x, y, K, tail, check_memory=False):
    """K micro-batches of 8 / K samples, `(loss / K).backward()` each, no zero_grad in between; returns the flat gradient."""
    eng = model.engine
    eng.cls_tail = tail
    for p in model.parameters():
        p.grad = None
    mb = x.shape[0] // K
    mem = []
    for k in range(K):
        (model(x[k * mb:(k + 1) * mb], labels=y[k * mb:(k + 1) * mb]).loss / K).backward()
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    assert eng._last["tail"] is tail
    for n, p in trainable(model):
        assert p.grad is not None and p.grad.data_ptr() == eng.g(n).data_ptr(), n  # still the flat buffer's views
    if check_memory and K >= 4:
        assert mem[1] == mem[3], mem  # nothing is allocated per accumulated micro-batch
    return eng.grads[:eng.layout.n_trainable].detach().clone()


def worst_tensor_error(model, flat, oracle_grads):
    lay = model.engine.layout
    gmax = max(float(g.norm()) for g in oracle_grads.values())
    worst = 0.0
    for n, g in oracle_grads.items():
        if float(g.norm()) < 1e-6 * gmax:
            continue  # key.bias: analytically zero
        off = lay.entries[n][0]
        mine = flat[off:off + g.numel()].double().cpu()
        worst = max(worst, float((mine - g.double().flatten()).norm() / g.double().norm()))
    return worst


@pytest.mark.parametrize("precision,tol", [("32", 2e-5), ("bf16-mixed", 2e-2)])
@pytest.mark.parametrize("tag", ["c1", "k1", "conv"])
def test_repeated_backward_accumulates_the_batch_gradient(dev, tag, precision, tol):
    """B = 8 as K = 4 micro-batches of 2 and as K = 2 of 4 against one backward over the 8 samples, at the gates
    tests/test_ddp_gpu.py:38-51 sets for the same split across two ranks; CLS tail on and off (bf16-mixed: the CLS-tail gate of
    tests/test_cls_tail_gpu.py against the CPU oracle -- bit-identity is asserted there only at tile-aligned widths with B a
    multiple of 256, which no fixture here has).  On the parent commit the buffer ends as 2 x the last micro-batch's gradient."""
    from test_parity_deep_gpu import bf16_factor

    rc, sd, flux, labels, oracle_grads = fixture_case(tag)
    model = build(rc, sd, dev, precision)
    x, y = flux.to(dev), labels.to(dev)
    worst = {}
    for tail in (True, False):
        whole = accumulate(model, x, y, 1, tail).double()
        for K in (4, 2):
            got = accumulate(model, x, y, K, tail, check_memory=True)
            e = float((got.double() - whole).norm() / whole.norm())
            worst[(tail, K)] = worst_tensor_error(model, got, oracle_grads)
            print(f"[accumulate {tag} {precision}] K={K} cls_tail={tail}: rel L2 error against one backward over the batch {e:.3e} "
                  f"(gate {tol:.0e}); worst tensor against the CPU oracle {worst[(tail, K)]:.3e}")
            assert e < tol, (tag, precision, K, tail, e)
    if precision != "32":
        f = bf16_factor("s")  # tests/test_parity_deep_gpu.py:44, as tests/test_cls_tail_gpu.py applies it
        for K in (4, 2):
            assert worst[(True, K)] <= f * worst[(False, K)] + 1e-3, (K, worst)


@pytest.mark.parametrize("tag", ["c1", "k1", "conv"])
def test_accumulated_buffers_with_and_without_cls_tail_are_bit_identical_in_fp32(dev, tag):
    """Precision '32': the buffer accumulated with the CLS tail on equals the one accumulated with it off, bit for bit -- and so
    does one backward in overwrite mode (K = 1).  The tail's f32 weight gradients and column sums walk the full path's order
    (vit_linear_bwd_dw_rows / vit_colsum_rows with f32 operands, include/vit_amd.h); before they did, 4 963 of the c1 fixture's
    39 304 gradient elements differed for ONE plain backward (relative L2 2.3e-8), and 2 301 / 3 251 at K = 4 / 2."""
    rc, sd, flux, labels, _ = fixture_case(tag)
    model = build(rc, sd, dev, "32")
    x, y = flux.to(dev), labels.to(dev)
    found = {}
    for K in (1, 4, 2):
        on, off = accumulate(model, x, y, K, True), accumulate(model, x, y, K, False)
        found[K] = int((on != off).sum())
        e = float((on.double() - off.double()).norm() / off.double().norm())
        print(f"[tail on/off {tag} 32] K={K}: {found[K]} of {on.numel()} elements differ, rel L2 {e:.3e}")
    assert found == {1: 0, 4: 0, 2: 0}, (tag, found)


# ------------------------------------------------------------------------------------------------ (c) mixed .grad state
def test_mixed_grad_state_is_an_error_and_zero_grad_in_place_is_not(dev):
    from vit_amd._cabi import VitError

    rc, sd, flux, labels, _ = fixture_case("c1")
    model = build(rc, sd, dev, "32")
    x, y = flux.to(dev)[:4], labels.to(dev)[:4]
    model(x, labels=y).loss.backward()
    plain = model.engine.grads.detach().clone()
    name = "vit.encoder.layer.1.intermediate.dense.weight"
    dict(zip(model._param_names, model._param_list))[name].grad = None
    with pytest.raises(VitError, match=name.replace(".", r"\.")):
        model(x, labels=y).loss.backward()
    # frozen parameters and the pooler are not part of the decision
    model.zero_grad(set_to_none=True)
    model(x, labels=y).loss.backward()
    frozen = dict(zip(model._param_names, model._param_list))["vit.embeddings.cls_token"]
    frozen.requires_grad_(False)
    frozen.grad = None
    model(x, labels=y).loss.backward()
    frozen.requires_grad_(True)
    n = model.engine.layout.n_trainable
    off = model.engine.layout.entries[name][0]
    assert torch.equal(model.engine.grads[off:off + 64], 2 * plain[off:off + 64])  # accumulated: x + x
    # zero_grad(set_to_none=False) keeps the views: the next backward adds to zeros, which is the plain gradient
    model.zero_grad(set_to_none=True)
    model(x, labels=y).loss.backward()
    model.zero_grad(set_to_none=False)
    assert all(float(p.grad.abs().max()) == 0.0 for _, p in trainable(model))
    model(x, labels=y).loss.backward()
    assert torch.equal(model.engine.grads[:n], plain[:n])
    assert all(p.grad.data_ptr() == model.engine.g(nm).data_ptr() for nm, p in trainable(model))


# ------------------------------------------------------------------------------------------------ (d) - (h) trainer
def c1_config(**train):
    cfg = {
        "model": dict(name="vit", task_type="reg", image_size=4096, patch_size=32, hidden_size=32, num_hidden_layers=3,
                      num_attention_heads=2, stride_size=32, proj_fn="SW"),
        "train": dict(batch_size=16, ep=1, precision="32"),
        "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"},
        "noise": {"noise_level": 0},
    }
    cfg["train"].update(train)
    return cfg


class Batches:
    """A re-iterable, unshuffled list of (flux, error, labels) batches over n seeded samples."""

    def __init__(self, n, seed, bs):
        g = torch.Generator().manual_seed(seed)
        self.flux = torch.randn(n, 4096, generator=g)
        self.err = 0.1 * torch.rand(n, 4096, generator=g)
        self.lab = torch.rand(n, generator=g)
        self.bs = bs

    def __iter__(self):
        for i in range(0, self.flux.shape[0], self.bs):
            s = slice(i, i + self.bs)
            yield self.flux[s], self.err[s], self.lab[s]


def make(cfg, dropout=False, seed=42):
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    seed_everything(seed)
    module = ViTLModule(config=cfg)
    if not dropout:
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
    trainer = Trainer(cfg["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.train()
    return module, trainer


def one_step(cfg, bs, n=16):
    """The parameters after the first optimizer step over the first n samples, fed in batches of bs."""
    module, trainer = make(cfg)
    batches = list(Batches(n, 5, bs))
    for i, b in enumerate(batches):
        trainer.training_step(module, tuple(t.cuda() for t in b), i, is_last=(i == len(batches) - 1))
    torch.cuda.synchronize()
    eng = module.model.engine
    assert trainer.global_step == trainer.optimizer._step == 1
    return eng.flat[:eng.layout.n_trainable].detach().double().cpu(), module, trainer


def same_step(a, b, precision, lr=1e-3):
    """tests/test_ddp_gpu.py:55-59: the first AdamW step moves every weight by ~lr * sign(g)."""
    assert float((a - b).abs().max()) <= 2.1 * lr
    agree = float(((a - b).abs() < 1e-5).double().mean())
    assert agree > (0.999 if precision == "32" else 0.97), agree
    return agree


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_trainer_accumulated_step_equals_large_batch_step(dev, precision):
    big, _, _ = one_step(c1_config(precision=precision, batch_size=16), 16)
    acc, _, _ = one_step(c1_config(precision=precision, batch_size=4, accumulate_grad_batches=4), 4)
    agree = same_step(big, acc, precision)
    print(f"[trainer {precision}] K=4 x 4 against 1 x 16 after one optimizer step: parameters agree on {agree:.4%} of entries")


def test_trainer_bookkeeping_over_an_epoch(dev):
    """10 batches, K = 4: three optimizer steps (4, 4, 2 micro-batches); global_step, the optimizer's step count and a one-cycle
    scheduler (3 steps in all: a fourth would raise) count optimizer steps; last_grad_norm is the accumulated buffer's."""
    cfg = c1_config(batch_size=4, accumulate_grad_batches=4)
    cfg["opt"]["lr_sch"] = "onecycle"
    cfg["data"]["num_samples"] = 40
    module, trainer = make(cfg)
    eng = module.model.engine
    steps, losses = [], []
    step0, train0 = trainer.optimizer.step, module.training_step
    trainer.optimizer.step = lambda *a, **k: (steps.append(eng.step_counter), step0(*a, **k))[1]
    module.training_step = lambda *a, **k: (lambda loss: (losses.append(float(loss)), loss)[1])(train0(*a, **k))
    hist = trainer.fit(module, Batches(40, 6, 4))
    torch.cuda.synchronize()
    sch = trainer.sched_cfg["scheduler"]
    assert steps == [4, 8, 10] and trainer.global_step == trainer.optimizer._step == 3  # forwards seen at each optimizer step
    assert sch.total_steps == 3 and sch.last_epoch == 3
    norm = float(eng.grads[:eng.layout.n_trainable].double().norm())
    assert abs(float(trainer.optimizer.last_grad_norm.sqrt()) - norm) <= 1e-5 * norm
    # the logged loss is the undivided one: the epoch mean of the ten batch losses, not a quarter of it
    assert len(losses) == 10 and abs(hist[-1]["mae_loss"] - sum(losses) / 10) <= 1e-6 * abs(sum(losses) / 10)


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_accumulate_grad_batches_one_is_the_key_absent(dev, precision):
    out = {}
    for key in ("absent", "one"):
        cfg = c1_config(precision=precision, **({"accumulate_grad_batches": 1} if key == "one" else {}))
        module, trainer = make(cfg, dropout=True)
        losses = [float(trainer.training_step(module, tuple(t.cuda() for t in b), i)) for i, b in enumerate(Batches(64, 8, 16))]
        assert trainer.global_step == 4
        out[key] = (losses, {k: v.detach().cpu().clone() for k, v in module.model.state_dict().items()})
    assert out["absent"][0] == out["one"][0]
    for k, v in out["absent"][1].items():
        assert torch.equal(v, out["one"][1][k]), k


def test_micro_batches_draw_their_own_dropout_masks(dev):
    cfg = c1_config(batch_size=4, accumulate_grad_batches=2)
    cfg["opt"]["lr"] = 0.0
    module, trainer = make(cfg, dropout=True)
    b = tuple(t.cuda() for t in next(iter(Batches(4, 9, 4))))
    l1 = float(trainer.training_step(module, b, 0))
    l2 = float(trainer.training_step(module, b, 1))
    assert l1 != l2 and trainer.global_step == 1
    trainer._es_best, trainer._es_bad = None, 0
    assert trainer.make_checkpoint(module)["vit_amd"]["dropout_step"] == 2  # counts training forwards, not optimizer steps


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_hip_graph_with_accumulation_warns_once_and_runs_eager(dev, precision):
    big, _, _ = one_step(c1_config(precision=precision, batch_size=16), 16)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        acc, module, trainer = one_step(c1_config(precision=precision, batch_size=8, accumulate_grad_batches=2, hip_graph=True), 8)
        for i, b in enumerate(Batches(16, 5, 8)):  # a second group: no second warning
            trainer.training_step(module, tuple(t.cuda() for t in b), i)
    hits = [w for w in caught if "hip_graph" in str(w.message)]
    assert len(hits) == 1 and "eager" in str(hits[0].message), [str(w.message) for w in caught]
    assert trainer._graphed is None and trainer.use_graph is False and trainer.global_step == 2
    same_step(big, acc, precision)


# ------------------------------------------------------------------------------------------------ (g) data parallelism
def run_ranks(tmp_path, world, precision, exchange, K):
    from vit_amd.launch import launch_ranks

    out = tmp_path / f"w{world}_{precision}_{exchange}_k{K}"
    out.mkdir()
    child = os.path.join(ROOT, "tests", "_accum_ddp_child.py")
    argv = [str(out), precision, exchange, str(K)]
    if world == 1:
        import subprocess

        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "VIT_DIST_SINGLE", "VIT_DIST_BACKEND"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, child, *argv], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    else:
        assert launch_ranks(world, child, argv, extra_env={"VIT_DIST_BACKEND": "gloo"}) == 0
    return [torch.load(out / f"rank{r}.pt", weights_only=True) for r in range(world)]


@pytest.mark.parametrize("precision,tol", [("32", 2e-5), ("bf16-mixed", 2e-2)])
def test_ddp_two_ranks_times_two_micro_batches(tmp_path, precision, tol):
    """World 2 x K 2 x per-rank batch 2 against a single process at B = 8.  The reducer is armed for the stepping micro-batch
    alone: buckets x optimizer-steps collectives, carrying the locally accumulated sums."""
    single = run_ranks(tmp_path, 1, precision, "allreduce", 1)[0]
    two = run_ranks(tmp_path, 2, precision, "allreduce", 2)
    n = single["n_trainable"]
    for r in two:
        assert r["world"] == 2 and r["mode"] == "allreduce" and r["global_step"] == r["opt_step"] == 1 and r["grads_are_views"]
        assert r["collectives"] == r["all_reduce_calls"] == r["buckets"] * 1 == 5, r  # tail, three layers, embeddings
    assert torch.equal(two[0]["grads"][:n], two[1]["grads"][:n]) and torch.equal(two[0]["params"], two[1]["params"])
    g1, g2 = single["grads"][:n].double(), two[0]["grads"][:n].double()
    e = float((g1 - g2).norm() / g1.norm())
    print(f"[ddp accumulate {precision}] 2 ranks x 2 micro-batches x 2 samples against one process at B = 8: rel L2 error {e:.3e} "
          f"(gate {tol:.0e})")
    assert e < tol, e
    assert abs(two[0]["grad_norm"] - single["grad_norm"]) <= tol * single["grad_norm"]
    if precision == "32":
        z = run_ranks(tmp_path, 2, precision, "zero1", 2)
        assert z[0]["mode"] == "zero1" and z[0]["collectives"] == z[0]["buckets"] and torch.equal(z[0]["params"], z[1]["params"])
        assert torch.equal(z[0]["params"][:n], two[0]["params"][:n])
