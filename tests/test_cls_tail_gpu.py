"""The last encoder layer's CLS tail (ViTEngine.cls_tail): behind the last layer's attention the head
consumes one row per image (specvit.py:78-81), so unless hidden states are asked for that part of the layer runs over the
B CLS rows only, forward and backward.  `engine.cls_tail = False` forces the full path on the same engine.

The yardstick is the CPU oracle (oracle/refvit.py; train mode: with the masks oracle/dropmask.py restates), not either
path.  In general the two paths are not bitwise equal (another GEMM core may serve M = B, and a sum over B instead of B*T rows
may run in another rounding order); in bf16-mixed at tile-aligned widths with T >= 64 and B a multiple of 256 -- the
benchmarked geometry -- the tail runs the full path's GEMM core, sums its rows in the full passes' order and IS bitwise equal:
the multi-slice `ms` case and test_same_bits_at_the_benchmarked_geometry assert it.
  precision '32': both paths meet the gates tests/test_parity_gpu.py:774-777 applies in that precision (check_train_parity:
    logits and loss < 1e-4, every gradient tensor < 2e-4; eval mode: the same figures, tests/test_parity_deep_gpu.py:13-14,
    126-127, 143).
  bf16-mixed: the CLS-tail path's error against the oracle is at most bf16_factor x the full path's error against the
    oracle + 1e-3 (tests/test_parity_deep_gpu.py:44-49: what that file allows between two bf16 evaluations of one quantity;
    1.15 at the C3 geometry, 1.5 for the few-sample small configurations), on the logits, the loss and the worst gradient
    tensor -- worst against worst, because per tensor the ratio of two bf16 rounding draws is not a stable quantity where
    a gradient is a cancelling sum (tests/test_parity_gpu.py:789-794) -- and every tensor stays under that file's absolute
    bf16 gates (tests/test_parity_gpu.py:781-783: 4e-2 with cosine > 0.999; RoPE 8e-2, :824).
A dropout mask keyed by the compact row instead of the original row b*T is an O(1) error in train mode under either gate.
"""
import ctypes
import os
import re

import pytest
import torch

BASE_SEED = 0x5DEECE66D2468ACE
STEP = 3

# tag -> (RefConfig keywords or a named config, batch, weight seed, input seed, bf16_factor tag, bf16 absolute gradient gate)
CASES = {
    # the last layer is also the first: LN-before's backward is the plain form taking the compact residual gradient
    "l1": (dict(image_size=512, patch_size=32, hidden_size=64, num_hidden_layers=1, num_attention_heads=2, stride_size=32,
                loss_name="mae"), 6, 11, 12, "s", 4e-2),
    "l3": ("C1", 4, 21, 22, "s", 4e-2),
    "rope": (dict(image_size=640, patch_size=32, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, stride_size=32,
                  pos_encoding_type="rope", rope_base=1000.0, loss_name="mae"), 5, 31, 32, "s", 8e-2),
    # B = 256 at widths of 256: the tail's products are tile-aligned (M = 256) and run the ping-pong core, as at the
    # benchmarked shape -- strided A operand, dropout keyed by row b*T in its generic epilogue, K = 256 weight gradients
    "pp": (dict(image_size=288, patch_size=32, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, stride_size=32,
                loss_name="mae"), 256, 41, 42, "s", 4e-2),
    "vitb": ("C3", 4, 51, 52, "c3", 4e-2),  # ViT-B/16 geometry (T 197, D 768, 12 layers)
    # T = 65, B = 256, 16 640 token rows: the full weight-gradient products split K into 32 slices, the column sums into 130
    # wave blocks (two CLS rows in most of them) -- the multi-slice form of the bitwise claim
    "ms": (dict(image_size=2048, patch_size=32, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, stride_size=32,
                loss_name="mae"), 256, 61, 62, "s", 4e-2),
}
_oracle = {}


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def case(tag):
    from oracle import refvit

    spec, B, wseed, xseed, ftag, gtol = CASES[tag]
    rc = refvit.named_config(spec) if isinstance(spec, str) else refvit.RefConfig(**spec)
    sd = refvit.make_state_dict(rc, wseed)
    flux, _, labels = refvit.make_inputs(rc, B, xseed)
    return rc, sd, flux, labels, ftag, gtol


def build(rc, sd, dev, precision):
    from vit_amd.config import ViTConfig
    from vit_amd.specvit import MyViT

    cfg = ViTConfig(task_type=rc.task_type, image_size=rc.image_size, patch_size=rc.patch_size, hidden_size=rc.hidden_size,
                    num_hidden_layers=rc.num_hidden_layers, num_attention_heads=rc.num_attention_heads, proj_fn=rc.proj_fn,
                    stride_size=rc.stride_size, num_labels=rc.num_labels, pos_encoding_type=rc.pos_encoding_type,
                    rope_base=rc.rope_base)
    model = MyViT(cfg, loss_name=rc.loss_name)
    model.set_precision(precision)
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def oracle(tag, rc, sd, flux, labels, train):
    """One CPU oracle forward + backward per (case, mode), shared by the precisions."""
    from oracle import dropmask as dm
    from oracle import refvit

    key = (tag, train)
    if key not in _oracle:
        if len(_oracle) >= 2:
            _oracle.clear()
        torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
        masks = dm.engine_masks(rc.hidden_dropout_prob, rc.attention_probs_dropout_prob, dm.step_seed(BASE_SEED, STEP),
                                None) if train else None
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        out = refvit.forward(rc, params, flux, labels, training=train, masks=masks)
        out.loss.backward()
        _oracle[key] = dict(loss=float(out.loss.detach()), logits=out.logits.detach(),
                            grads={k: p.grad for k, p in params.items() if p.grad is not None})
    return _oracle[key]


def hip_pass(model, x, labels, train, tail, **kw):
    """Forward + backward with the masks of step STEP; returns loss, logits and EVERY trainable slice of eng.grads."""
    eng = model.engine
    eng.cls_tail = tail
    model.train(train)
    eng.base_seed, eng.step_counter = BASE_SEED, STEP - 1
    for p in model.parameters():
        p.grad = None
    out = model(x, labels=labels, **kw)
    out.loss.backward()
    lay = eng.layout
    grads = {n: lay.view(eng.grads, n).detach().clone().cpu() for n, (off, _) in lay.entries.items() if off < lay.n_trainable}
    return dict(loss=float(out.loss.detach()), logits=out.logits.detach().cpu(), grads=grads, out=out,
                tail=eng._last["tail"])


def errors(h, o):
    gmax = max(float(g.norm()) for g in o["grads"].values())
    e = dict(logits=rel(h["logits"], o["logits"]), loss=abs(h["loss"] - o["loss"]) / abs(o["loss"]), grads={})
    assert set(h["grads"]) == set(o["grads"])  # every trainable slice has an oracle gradient, and the other way round
    for name, g in o["grads"].items():
        mine = h["grads"][name].double().flatten()
        r = g.double().flatten()
        if float(r.norm()) < 1e-6 * gmax:  # key.bias: analytically zero
            assert float(mine.norm()) < 2e-3 * gmax, name
            continue
        e["grads"][name] = (float((mine - r).norm() / r.norm()), float(torch.dot(mine, r) / (mine.norm() * r.norm() + 1e-30)))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])  # varies fastest: one oracle run per (case, mode)
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("tag", list(CASES))
def test_cls_tail_against_full_path_and_oracle(dev, tag, train, precision):
    from test_parity_deep_gpu import bf16_factor

    rc, sd, flux, labels, ftag, gtol = case(tag)
    o = oracle(tag, rc, sd, flux, labels, train)
    model = build(rc, sd, dev, precision)
    x, y = flux.to(dev), labels.to(dev)
    full = hip_pass(model, x, y, train, tail=False)
    tail = hip_pass(model, x, y, train, tail=True)
    assert full["tail"] is False and tail["tail"] is True
    ef, et = errors(full, o), errors(tail, o)
    wf, wt = max(ef["grads"].items(), key=lambda kv: kv[1][0]), max(et["grads"].items(), key=lambda kv: kv[1][0])
    between = max(rel(tail["grads"][n], full["grads"][n]) for n in et["grads"])
    mode = "train" if train else "eval"
    print(f"[{tag} {precision} {mode}] against the oracle, full / CLS tail: logits {ef['logits']:.2e} / {et['logits']:.2e}, "
          f"loss {ef['loss']:.2e} / {et['loss']:.2e}, worst gradient {wf[1][0]:.2e} ({wf[0]}) / {wt[1][0]:.2e} ({wt[0]}); "
          f"ratios tail / full: logits {et['logits'] / max(ef['logits'], 1e-30):.2f}, worst gradient "
          f"{wt[1][0] / max(wf[1][0], 1e-30):.2f}; tail against full: logits {rel(tail['logits'], full['logits']):.2e}, "
          f"worst gradient {between:.2e}")
    if precision != "32" and rc.seq_len >= 64 and rc.hidden_size % 256 == 0 and x.shape[0] % 256 == 0:
        # the tail's products run the core the full path's run (B a multiple of 256), and it sums its B rows in the order of
        # the full-size ping-pong passes, whose other rows are exact zeros (include/vit_amd.h: vit_linear_bwd_dw_rows,
        # vit_layernorm_bwd_rows): the same bits, not only the same error
        assert tail["loss"] == full["loss"] and torch.equal(tail["logits"], full["logits"])
        for n in full["grads"]:
            assert torch.equal(tail["grads"][n], full["grads"][n]), n
    if precision == "32":
        for name, e in (("full", ef), ("tail", et)):  # tests/test_parity_gpu.py:774-777
            assert e["logits"] < 1e-4 and e["loss"] < 1e-4, (name, e["logits"], e["loss"])
            for pname, (r, _) in e["grads"].items():
                assert r < 2e-4, (name, pname, r)
        return
    f = bf16_factor(ftag)  # tests/test_parity_deep_gpu.py:44
    assert et["logits"] <= f * ef["logits"] + 1e-3, (et["logits"], ef["logits"])
    assert et["loss"] <= f * ef["loss"] + 1e-3, (et["loss"], ef["loss"])
    assert wt[1][0] <= f * wf[1][0] + 1e-3, (wt, wf)
    for pname, (r, c) in et["grads"].items():  # tests/test_parity_gpu.py:781-783
        assert r < gtol and c > 0.999, (pname, r, c)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
@pytest.mark.parametrize("tag", ["l1", "l3"])
def test_hidden_states_and_attentions_take_the_full_path(dev, tag, precision):
    """output_hidden_states=True runs the full path whatever `cls_tail` says: with and without labels / grad the outputs
    are bit for bit the forced full path's, and the backward behind such a forward leaves the full path's gradients."""
    rc, sd, flux, labels, _, _ = case(tag)
    model = build(rc, sd, dev, precision)
    x, y = flux.to(dev), labels.to(dev)
    kw = dict(output_hidden_states=True, output_attentions=True)
    for train in (False, True):
        a = hip_pass(model, x, y, train, tail=False, **kw)
        b = hip_pass(model, x, y, train, tail=True, **kw)
        assert a["tail"] is False and b["tail"] is False
        assert len(b["out"].hidden_states) == rc.num_hidden_layers + 1 and len(b["out"].attentions) == rc.num_hidden_layers
        assert a["loss"] == b["loss"] and torch.equal(a["logits"], b["logits"])
        for u, v in zip(a["out"].hidden_states + a["out"].attentions, b["out"].hidden_states + b["out"].attentions):
            assert torch.equal(u, v)
        for n in a["grads"]:
            assert torch.equal(a["grads"][n], b["grads"][n]), n
        # the gradients behind the full-path forward are the plain full path's (no hidden states asked for)
        c = hip_pass(model, x, y, train, tail=False)
        for n in a["grads"]:
            assert torch.equal(a["grads"][n], c["grads"][n]), n
    # no labels / no grad: the evaluation arena
    model.eval()
    outs = []
    for tail in (False, True):
        model.engine.cls_tail = tail
        with torch.no_grad():
            outs.append(model(x, **kw))
        assert model.engine._last["tail"] is False
    for u, v in zip(outs[0].hidden_states + outs[0].attentions + (outs[0].logits,),
                    outs[1].hidden_states + outs[1].attentions + (outs[1].logits,)):
        assert torch.equal(u, v)
    # attention maps alone do not need the last layer's token rows: the tail runs, the maps are the full path's bit for bit
    model.engine.cls_tail = True
    with torch.no_grad():
        o2 = model(x, output_attentions=True)
    assert model.engine._last["tail"] is True
    for u, v in zip(o2.attentions, outs[0].attentions):
        assert torch.equal(u, v)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_switching_paths_reuses_the_arena(dev, precision):
    """tail, full, tail, full on one engine (one arena): the step after a switch equals the same path's earlier step bit for
    bit (the kernels are deterministic), in train mode; then an evaluation forward without grad takes the tail too and
    meets the oracle at the eval gates of test_cls_tail_against_full_path_and_oracle."""
    from test_parity_deep_gpu import bf16_factor

    rc, sd, flux, labels, ftag, _ = case("l3")
    model = build(rc, sd, dev, precision)
    x, y = flux.to(dev), labels.to(dev)
    runs = [hip_pass(model, x, y, True, tail=t) for t in (True, False, True, False)]
    for first, again in ((runs[0], runs[2]), (runs[1], runs[3])):
        assert first["loss"] == again["loss"] and torch.equal(first["logits"], again["logits"])
        for n in first["grads"]:
            assert torch.equal(first["grads"][n], again["grads"][n]), n
    o = oracle("l3", rc, sd, flux, labels, False)
    model.eval()
    logits = {}
    for tail in (False, True):
        model.engine.cls_tail = tail
        with torch.no_grad():
            out = model(x, labels=y)
        assert model.engine._last["tail"] is tail and model.engine._last["grad"] is False
        logits[tail] = (rel(out.logits, o["logits"]), abs(float(out.loss) - o["loss"]) / abs(o["loss"]))
    print(f"[l3 {precision} eval, no grad] logits / loss against the oracle: full {logits[False]}, CLS tail {logits[True]}")
    if precision == "32":
        assert max(logits[False] + logits[True]) < 1e-4
    else:
        f = bf16_factor(ftag)
        assert logits[True][0] <= f * logits[False][0] + 1e-3 and logits[True][1] <= f * logits[False][1] + 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("train", [False, True])
def test_same_bits_at_the_benchmarked_geometry(dev, train):
    """ViT-B/16 widths and token count (T 197, D 768, 12 heads, MLP 3072) at the benchmark's B = 256, two layers deep (no
    oracle: the CPU cannot run this batch): 50 432 token rows, the full weight gradients in 7 / 7 / 28 K slices, 394 wave
    blocks of column sums.  Loss, logits and every gradient of the CLS tail equal the forced full path's bit for bit."""
    from oracle import refvit

    rc = refvit.RefConfig(image_size=50176, patch_size=256, hidden_size=768, num_hidden_layers=2, num_attention_heads=12,
                          stride_size=256, loss_name="mae")
    sd = refvit.make_state_dict(rc, 71)
    flux, _, labels = refvit.make_inputs(rc, 256, 72)
    model = build(rc, sd, dev, "bf16-mixed")
    x, y = flux.to(dev), labels.to(dev)
    full = hip_pass(model, x, y, train, tail=False)
    tail = hip_pass(model, x, y, train, tail=True)
    assert full["tail"] is False and tail["tail"] is True
    assert tail["loss"] == full["loss"] and torch.equal(tail["logits"], full["logits"])
    for n in full["grads"]:
        assert torch.equal(tail["grads"][n], full["grads"][n]), n


@pytest.mark.gpu
def test_dctx_cls_rows_between_the_cls_rows_are_never_written(dev):
    """The tail's dctx buffer is zero from allocation and only its rows b*T are written (engine.py: INVARIANT).  Fill the rows
    in between with a marker after a first step: a second step must leave every marker in place (nobody rewrites them)."""
    rc, sd, flux, labels, _, _ = case("l3")
    model = build(rc, sd, dev, "bf16-mixed")
    x, y = flux.to(dev), labels.to(dev)
    hip_pass(model, x, y, True, tail=True)
    eng, T = model.engine, rc.seq_len
    buf = eng.tmp["dctx_cls"]
    rows = torch.arange(buf.shape[0], device=dev)
    other = rows[rows % T != 0]
    assert float(buf[other].abs().max()) == 0.0
    buf[other] = 3.0
    hip_pass(model, x, y, True, tail=True)
    assert bool((buf[other] == 3.0).all())
    buf[other] = 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("tag", ["l3", "ms"])
def test_one_stream_and_two_streams_give_the_same_bits(dev, tag, tail):
    """engine.overlap_dw moves the weight-gradient products (and nothing else) to a second HIP stream with a workspace of its
    own: the kernels and their arguments are the same and each is deterministic, so a train-mode step in bf16-mixed leaves the
    same loss, logits and gradient bits with one stream and with two.  `l3` is off the 256-aligned GEMM core; at `ms` the
    weight gradients are multi-slice split-K products in the second handle's workspace, and with two layers every scratch
    buffer of the backward is rewritten while a reader of it on the second stream may still exist."""
    rc, sd, flux, labels, _, _ = case(tag)
    model = build(rc, sd, dev, "bf16-mixed")
    x, y = flux.to(dev), labels.to(dev)
    eng, runs = model.engine, []
    for overlap in (False, True):
        eng.overlap_dw = overlap
        runs.append(hip_pass(model, x, y, True, tail=tail))
        assert runs[-1]["tail"] is tail
        assert (eng.side_stream is not None) is overlap
    one, two = runs
    assert one["loss"] == two["loss"] and torch.equal(one["logits"], two["logits"])
    for n in one["grads"]:
        assert torch.equal(one["grads"][n], two["grads"][n]), n


# ------------------------------------------------------------------ no GPU needed
# every export of the parent's header with its parameter count: the CLS tail ADDS entry points and one descriptor field
_EXPORTS = {
    'vit_version': 0, 'vit_last_error': 0, 'vit_create': 2, 'vit_destroy': 1, 'vit_set_workspace': 3, 'vit_set_option': 2,
    'vit_handle_set_option': 3, 'vit_step_state_bind': 2, 'vit_step_advance': 5, 'vit_gemm': 3,
    'vit_last_gemm_kernel': 0, 'vit_linear_fwd': 16, 'vit_linear_bwd_dx': 10, 'vit_linear_bwd_dw': 9, 'vit_layernorm_fwd': 12,
    'vit_layernorm_fwd_residual': 15, 'vit_layernorm_bwd': 14, 'vit_layernorm_bwd_fused': 20, 'vit_attention_fwd': 15,
    'vit_attention_bwd': 19, 'vit_attention_probs': 10, 'vit_unfold_cast': 10, 'vit_fold_add': 9, 'vit_add_noise': 8,
    'vit_rope_qk': 12, 'vit_embed_finish': 11, 'vit_embed_finish_bwd': 14, 'vit_dropout_bwd_cast': 10, 'vit_colsum': 9,
    'vit_cast_f32_bf16': 5, 'vit_cast_bf16_f32': 6, 'vit_head_loss_fwd': 13, 'vit_head_loss_bwd': 16, 'vit_grad_sqnorm': 5,
    'vit_grad_sqnorm_acc': 5, 'vit_adamw_step': 16,
}
_NEW = {'vit_layernorm_fwd_residual_rows': 16, 'vit_layernorm_bwd_rows': 22, 'vit_linear_bwd_dw_rows': 13, 'vit_colsum_rows': 10,
        'vit_workspace_needed': 0}
_DESC_FIELDS = ["M", "N", "K", "a_trans", "b_trans", "ab_dtype", "A", "lda", "B", "ldb", "C", "ldc", "c_dtype", "alpha", "bias",
                "act", "aux_out", "aux_in", "ldaux", "dropout_p", "seed", "site", "residual", "ldres", "rows_per_batch",
                "out_batch_rows", "out_row_offset", "split_k", "accumulate", "colsum_out", "rope_cos", "rope_sin", "rope_T",
                "rope_dh", "rope_cols"]


def test_exports_added_and_existing_signatures_kept():
    from vit_amd import _cabi

    text = re.sub(r"/\*.*?\*/", "", open(_cabi.HEADER_PATH).read(), flags=re.S)
    decl = {}
    for name, args in re.findall(r"\b(vit_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = args.strip()
        decl[name] = 0 if args in ("", "void") else args.count(",") + 1
    assert decl == {**_EXPORTS, **_NEW}
    lib = _cabi.load()
    for name, n in {**_EXPORTS, **_NEW}.items():
        assert hasattr(lib, name), name
        assert len(_cabi._PROTOS[name]) == n, name
    # the descriptor grew at its END: every earlier field keeps its place, and a zeroed new field means today's behaviour
    names = [f[0] for f in _cabi.GemmDesc._fields_]
    assert names == _DESC_FIELDS + ["drop_row_stride"]
    assert _cabi.GemmDesc.drop_row_stride.offset >= _cabi.GemmDesc.rope_cols.offset + ctypes.sizeof(ctypes.c_int)
    assert _cabi.GemmDesc().drop_row_stride == 0
    # argument errors of the new entry points come back as a status, without a GPU
    assert lib.vit_layernorm_fwd_residual_rows(None, None, 1, None, 1, None, None, None, None, 1, None, None, 4, 32, 1e-12,
                                               None) == -1
    assert b"null pointer" in lib.vit_last_error()
    assert lib.vit_layernorm_bwd_rows(None, None, 1, None, None, None, None, None, 0, None, None, None, 4, 32, None, 1, None,
                                      0.0, 0, 0, 1, None) == -1
    assert b"null pointer" in lib.vit_last_error()
