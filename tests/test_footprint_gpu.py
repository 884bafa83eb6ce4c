"""Every kernel call with the inputs OUTSIDE a target's footprint overwritten (tests/_footprint.py): each case runs one entry point
once for a baseline, compares every target region with an fp64 reference at the tolerance the kernel's own test asserts, and
then, per target, three more times -- a fresh Gaussian draw, a draw times 2^12 and the NaN byte fill over everything the header
says the target does not depend on -- and demands the target bit for bit.  The footprints are the headers' (include/*.h), not
the kernels'.  Targets sit where indexing goes wrong: the first and last slice, one in the middle, the last partial tile, one
that straddles a tile boundary, and the two sides of a sample boundary of the token-major layouts.

CASES is the table; tests/test_footprint_cpu.py checks that every exported vit_* name is a case's entry point or in NO_FOOTPRINT,
that every input view the table names exists, and that every region is large enough for its tolerance (rounding_room).

Measured on an MI355X: 332 cases, 4472 target groups, 16.7 s of pytest wall time for the file (tests/test_poison_gpu.py: 271 cases
in 7.0 s); no case takes a second."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _footprint import Case, IntIn, footprint, others

F32, BF16 = torch.float32, torch.bfloat16
CASES = []
ALL = slice(None)

# exported names no case calls, each with the reason in one line
NO_FOOTPRINT = {
    "vit_version": "no input",
    "vit_last_error": "no input",
    "vit_create": "set-up only",
    "vit_destroy": "set-up only",
    "vit_set_workspace": "set-up only",
    "vit_workspace_needed": "no input",
    "vit_set_option": "set-up only",
    "vit_handle_set_option": "set-up only",
    "vit_step_state_bind": "set-up only",
    "vit_step_advance": "set-up only: the record is a function of the scalars alone",
    "vit_last_gemm_kernel": "no input",
    "vit_optim_groups_write": "set-up only: writes a table from kernel arguments",
    "vit_layer_scale_table_write": "set-up only: writes a table from kernel arguments",
    "vit_mix_plan_write": "set-up only: writes a table from kernel arguments",
    "vit_grad_sqnorm": "the one output depends on every input",
    "vit_grad_sqnorm_acc": "the one output depends on every input",
    "vit_sam_sqnorm": "the one output depends on every input",
    "vit_mim_loss_fwd": "the scalar loss and count depend on every input",
    "vit_patch_select": "no tensor input; that sample b's draw does not depend on B is test_patch_select_is_per_sample below",
}


def add(cid, entries, make, run, targets, outside, **kw):
    CASES.append(Case(cid, entries, make, run, targets, outside, **kw))


def bf(t):
    return t.to(BF16)


def randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def rand(shape, dev, seed):
    return torch.rand(shape, generator=torch.Generator(device="cpu").manual_seed(seed)).to(dev)


def E(dev, *s, dt=F32):
    return torch.empty(s, dtype=dt, device=dev)


def dn(dt):
    return "bf16" if dt == BF16 else "f32"


def sl(a, b, c=None):
    return slice(a, b, c)


def drop_mult(drop, rows, cols, dev="cpu", stride=1):
    """The dropout multiplier of every element of a [rows, cols] tensor keyed by row * stride, restated on the host."""
    from oracle import dropmask as dm

    m = dm.multiplier(dm.drop_cfg(*drop), (rows - 1) * stride + 1, cols)[::stride]
    return torch.from_numpy(np.ascontiguousarray(m)).to(dev)


@contextlib.contextmanager
def options(dev, reserve=False, **opts):
    """Process-wide kernel-selection options for the block (name -> (value, default)), and optionally a handle of its own with
    reserve_cus = 8: the one-workgroup-per-CU kernels launch fewer workgroups."""
    from test_poison_gpu import option, reserved

    with contextlib.ExitStack() as st:
        for name, (value, default) in opts.items():
            st.enter_context(option(name, value, default))
        if reserve:
            st.enter_context(reserved(dev))
        yield


def ctx_of(reserve=False, **opts):
    return functools.partial(options, reserve=reserve, **opts) if (reserve or opts) else None


# =================================================================================================== GEMM
# vit_gemm_desc (include/vit_amd.h): C rows in S depend on A's rows in S, all of B, bias, and aux_in / residual / old C at rows
# S; C columns in S depend on B's rows in S and bias[S] (and aux_in / residual / old C at columns S).  The generic core works
# in 128 x 128 tiles, the ping-pong core in 256 x 256 tiles of two 128-row wave blocks.
PAD = 8


def gemm_tol(ab, cdt):
    return 3e-5 if ab == F32 else 2e-5 if cdt == F32 else 4e-3


def gemm_targets(M, N):
    """(row slices, column slices): first, last, middle, the last partial tile, straddling a 128 / 256 boundary."""
    def pick(n):
        s = [sl(0, 1), sl(n - 1, n), sl(n // 2 - 1, n // 2 + 2)]
        if n > 128:
            s.append(sl(250, 262) if n > 256 and n % 256 == 0 else sl(120, 136))
            if n % 128:
                s.append(sl(n - n % 128, n))
        elif n % 16:
            s.append(sl(n - n % 16, n))
        return s

    return pick(M), pick(N)


def gemm_case(cid, M, N, K, layout="nt", cdt=BF16, ab=BF16, core=None, split_k=0, reserve=False, epi=None, wide=False,
              entries="vit_gemm"):
    from vit_amd._cabi import ACT_DGELU, ACT_GELU, ACT_MUL_AUX

    a_t, b_t = layout in ("tn", "tt"), layout in ("nn", "tn")
    pad = PAD if wide else 0
    drop = (0.1, 77, 5)
    s_rows = 3  # drop_row_stride
    has_bias = epi in ("gelu_aux", "drop_res", "row_map", "drop_row_stride")
    aux_in = epi in ("dgelu", "mul_aux")
    has_res = epi == "drop_res"
    Bn, rpb = 4, M // 4  # row_map: 4 samples

    def store(t, tr, seed, dev):  # the operand as the layout stores it, inside a wider tensor when `wide`
        t = t.t() if tr else t
        w = randn((t.shape[0], t.shape[1] + pad), dev, seed).to(t.dtype)
        w[:, :t.shape[1]] = t
        return w

    def make(dev):
        A, Bm = randn((M, K), dev, 1).to(ab), randn((N, K), dev, 2, 0.1 if epi else 1.0).to(ab)
        d = {"B": store(Bm, b_t, 12, dev)}
        if epi == "drop_row_stride":
            full = randn((M * s_rows, K), dev, 13).to(ab)
            full[::s_rows] = A
            d["A"] = full
        else:
            d["A"] = store(A, a_t, 11, dev)
        if has_bias:
            d["bias"] = randn((N,), dev, 5)
        if aux_in:
            d["aux"] = bf(randn((M, N + pad), dev, 8))
        if has_res:
            d["res"] = randn((M, N + pad), dev, 6)
        if epi == "accumulate":
            d["C0"] = randn((M, N + pad), dev, 9)
        return d

    def logical(d):
        A, Bm = d["A"].double(), d["B"].double()
        A = A[::s_rows] if epi == "drop_row_stride" else A[:, :M].t() if a_t else A[:, :K]
        return A, Bm[:, :N].t() if b_t else Bm[:, :K]

    def ref(d):
        A, Bm = logical(d)
        v = A @ Bm.t()
        out = {}
        if has_bias:
            v = v + d["bias"].double()
        if epi == "gelu_aux":
            out["aux"] = v
            v = F.gelu(v)
        elif epi == "dgelu":
            u = d["aux"][:, :N].double().requires_grad_(True)
            F.gelu(u).backward(v)
            v = u.grad
        elif epi == "mul_aux":
            v = v * d["aux"][:, :N].double()
        if epi in ("drop_res", "drop_row_stride"):
            v = v * drop_mult(drop, M, N, v.device, s_rows if epi == "drop_row_stride" else 1).double()
        if has_res:
            v = v + d["res"][:, :N].double()
        if epi == "accumulate":
            v = v + d["C0"][:, :N].double()
        if epi == "row_map":
            full = torch.zeros((Bn, rpb + 1, N), dtype=torch.float64, device=v.device)
            full[:, 1:] = v.view(Bn, rpb, N)
            v = full.view(Bn * (rpb + 1), N)
        out["C"] = v
        return out

    def run(d):
        import vit_amd.functional as vf

        A, Bs = d["A"], d["B"]
        dev = A.device
        kw = {}
        if epi == "row_map":
            buf = torch.zeros((Bn * (rpb + 1), N + pad), dtype=cdt, device=dev)
            kw["row_map"] = (rpb, rpb + 1, 1)
        elif epi == "accumulate":
            buf = d["C0"]  # a clone: the call adds into it
            kw["accumulate"] = True
        else:
            buf = E(dev, M, N + pad, dt=cdt)
        out = {"C": buf[:, :N]}
        if epi == "gelu_aux":
            auxb = E(dev, M, N + pad, dt=BF16)
            kw.update(act=ACT_GELU, aux_out=auxb, ldaux=N + pad)
            out["aux"] = auxb[:, :N]
        elif aux_in:
            kw.update(act=ACT_DGELU if epi == "dgelu" else ACT_MUL_AUX, aux_in=d["aux"], ldaux=N + pad)
        if epi in ("drop_res", "drop_row_stride"):
            kw["dropout"] = drop
        if has_res:
            kw.update(residual=d["res"], ldres=N + pad)
        if epi == "drop_row_stride":
            kw["drop_row_stride"] = s_rows
        lda = s_rows * K if epi == "drop_row_stride" else A.shape[1]
        vf.gemm(A, Bs, M=M, N=N, K=K, a_trans=a_t, b_trans=b_t, lda=lda, ldb=Bs.shape[1], out=buf, ldc=N + pad, split_k=split_k,
                bias=d.get("bias"), **kw)
        if core is not None:  # the plan falls back to the generic core silently: the label of the case must stay true
            from vit_amd import _cabi

            sym = _cabi.load().vit_last_gemm_kernel().decode()
            assert sym.startswith("gemm3_kernel") == (core == 5), f"gemm_core={core} ran {sym}"
        return out

    # the operands' pad columns (wide) and, for drop_row_stride, the rows of A between the strided ones: outside every footprint
    always = []
    if wide:
        always += [("A", (ALL, sl((M if a_t else K), None))), ("B", (ALL, sl((N if b_t else K), None)))]
        always += [(k, (ALL, sl(N, None))) for k, on in (("aux", aux_in), ("res", has_res), ("C0", epi == "accumulate")) if on]
    if epi == "drop_row_stride":
        always.append(("A", others(M * s_rows, sl(0, None, s_rows))))
    row_sets, col_sets = gemm_targets(M, N)
    if epi == "row_map":  # the rows on either side of every sample boundary: the skipped rows lie between them
        row_sets = [sl(b * rpb - 2, b * rpb + 2) for b in range(1, Bn)] + [sl(0, 1), sl(M - 1, M)]
    targets, outside = [], []
    for S in row_sets:
        o = list(always)
        if epi == "drop_row_stride":
            o.append(("A", others(M, S) * s_rows))
        else:
            o.append(("A", (ALL, others(M, S)) if a_t else others(M, S)))
        o += [(k, others(M, S)) for k, on in (("aux", aux_in), ("res", has_res), ("C0", epi == "accumulate")) if on]
        if epi == "row_map":
            m = torch.arange(M)[S]
            S = m // rpb * (rpb + 1) + m % rpb + 1
        targets.append([("C", S), ("aux", S)] if epi == "gelu_aux" else ("C", S))
        outside.append(o)
    for S in col_sets:
        o = list(always) + [("B", (ALL, others(N, S)) if b_t else others(N, S))]
        if has_bias:
            o.append(("bias", others(N, S)))
        o += [(k, (ALL, others(N + pad, S))) for k, on in (("aux", aux_in), ("res", has_res), ("C0", epi == "accumulate")) if on]
        targets.append(("C", (ALL, S)))
        outside.append(o)
    tol = gemm_tol(ab, cdt)
    # tests/test_kernels_gpu.py::test_gemm_epilogues: 5e-3 for the GELU output, 8e-3 for the MUL_AUX product, 4e-3 for aux
    tols = {"C": {"gelu_aux": 5e-3, "mul_aux": 8e-3}.get(epi, tol) if cdt == BF16 else tol, "aux": 4e-3}
    opts = {"gemm_core": (core, 1)} if core is not None else {}
    add(cid, entries, make, run, targets, outside, ref=ref, tol=tols, context=ctx_of(reserve, **opts))


for cdt in (BF16, F32):
    for lay in ("nt", "nn", "tn", "tt"):
        for shape in ((104, 40, 72), (264, 136, 72)):
            gemm_case(f"gemm generic {shape} {lay} {dn(cdt)}", *shape, layout=lay, cdt=cdt)
for lay in ("nt", "nn", "tn", "tt"):
    for shape in ((104, 40, 72), (264, 136, 72)):
        gemm_case(f"gemm x3 {shape} {lay}", *shape, layout=lay, cdt=F32, ab=F32)
for shape in ((256, 256, 64), (512, 512, 192)):
    for lay in ("nt", "nn", "tn"):
        for cdt in (BF16, F32):
            gemm_case(f"gemm ping-pong {shape} {lay} {dn(cdt)}", *shape, layout=lay, cdt=cdt, core=5)
gemm_case("gemm ping-pong (512, 512, 192) nt bf16 reserve_cus=8", 512, 512, 192, core=5, reserve=True)
gemm_case("gemm split_k=5 (96, 64, 4096)", 96, 64, 4096, cdt=F32, split_k=5)
gemm_case("gemm split_k=-1 (96, 64, 4096)", 96, 64, 4096, cdt=F32, split_k=-1)
gemm_case("gemm ping-pong split_k=5 (256, 256, 4096) tn", 256, 256, 4096, layout="tn", cdt=F32, core=5, split_k=5)
gemm_case("gemm ping-pong split_k=-1 (256, 256, 4096) tn", 256, 256, 4096, layout="tn", cdt=F32, core=5, split_k=-1)
# the epilogues, each on both cores (the ping-pong core takes GELU with nt and DGELU / MUL_AUX with nn operands: pp_plan)
for epi, lay, cdt in (("gelu_aux", "nt", BF16), ("dgelu", "nn", BF16), ("mul_aux", "nn", BF16), ("drop_res", "nt", F32),
                      ("drop_res", "nt", BF16), ("row_map", "nt", F32), ("accumulate", "tn", F32)):
    gemm_case(f"gemm generic epilogue {epi} (264, 136, 72) {lay} {dn(cdt)}", 264, 136, 72, layout=lay, cdt=cdt, epi=epi, core=0)
    gemm_case(f"gemm ping-pong epilogue {epi} (512, 256, 64) {lay} {dn(cdt)}", 512, 256, 64, layout=lay, cdt=cdt, epi=epi, core=5)
gemm_case("gemm epilogue drop_row_stride=3 (104, 40, 72) lda=3K", 104, 40, 72, cdt=BF16, epi="drop_row_stride")
gemm_case("gemm epilogue drop_row_stride=3 (256, 256, 64) lda=3K", 256, 256, 64, cdt=F32, epi="drop_row_stride")
# every leading dimension wider than its row, once per core and operand kind
for epi, lay, cdt in ((None, "nt", BF16), (None, "tn", F32), ("gelu_aux", "nt", BF16), ("dgelu", "nn", BF16), ("drop_res", "nt", F32),
                      ("accumulate", "tn", F32)):
    gemm_case(f"gemm generic wide ld {epi} (264, 136, 72) {lay} {dn(cdt)}", 264, 136, 72, layout=lay, cdt=cdt, epi=epi, core=0, wide=True)
    gemm_case(f"gemm ping-pong wide ld {epi} (256, 256, 64) {lay} {dn(cdt)}", 256, 256, 64, layout=lay, cdt=cdt, epi=epi, core=5, wide=True)


# =================================================================================================== LayerNorm
# include/vit_amd.h: a row's y, xsum, mean, rstd, dx and dyn depend on that row's inputs and on gamma / beta.  dgamma / dbeta
# depend on all rows: their columns in S depend on columns S of dy and x (mean and rstd are inputs of the backward).  dbias =
# colsum(mask * dx) depends on whole rows and is no column target.
EPS = 1e-12
LN_SHAPES = ((37, 32), (129, 1024), (33, 2048))
PATH_SITE = 4 + 4 * 5


def affine(D, dev):
    return randn((D,), dev, 21) * 0.1 + 1, randn((D,), dev, 22) * 0.1


def row_picks(n, edge=32):
    """first, last, middle, and the rows around the last multiple of `edge` (a block or sample boundary)."""
    s = [sl(0, 1), sl(n - 1, n), sl(n // 2 - 1, n // 2 + 2)]
    m = (n - 1) // edge * edge
    if m > 0:
        s.append(sl(m - 1, min(n, m + 2)))
    return s


def col_picks(D):
    s = [sl(0, 1), sl(D - 1, D), sl(D // 2 - 1, D // 2 + 2)]
    if D > 256:
        s.append(sl(252, 260))
    return s


def stats(x):
    """(mean, rstd) in f32 from an fp64 pass: inputs of the backward forms."""
    xd = x.double()
    mean = xd.mean(-1)
    return mean.float(), (1.0 / torch.sqrt(xd.var(-1, unbiased=False) + EPS)).float()


def ln_ref(x, g, b):
    return F.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), EPS)


def ln_bwd_ref(dy, x, g, mean, rstd):
    """dx, dgamma, dbeta in fp64 from the operands as the kernel consumes them (mean / rstd are inputs)."""
    dy, g = dy.double(), g.double()
    xhat = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    a = dy * g
    dx = rstd.double()[:, None] * (a - a.mean(-1, keepdim=True) - xhat * (a * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).sum(0), dy.sum(0)


def ln_fwd_case(rows, D, odt):
    def make(dev):
        g, b = affine(D, dev)
        return {"x": randn((rows, D), dev, 20) * 3 + 0.5, "g": g, "b": b}

    def run(d):
        import vit_amd.functional as vf

        y, mean, rstd = vf.layernorm_fwd(d["x"], d["g"], d["b"], EPS, out_dtype=odt)
        return {"y": y, "mean": mean, "rstd": rstd}

    def ref(d):
        return {"y": ln_ref(d["x"], d["g"], d["b"]), "mean": d["x"].double().mean(-1)}

    targets, outside = [], []
    for S in row_picks(rows):
        targets.append([(name, S) for name in ("y", "mean", "rstd")])
        outside.append([("x", others(rows, S))])
    add(f"vit_layernorm_fwd ({rows}, {D}) {dn(odt)}", "vit_layernorm_fwd", make, run, targets, outside, ref=ref,
        tol={"y": 1e-6 if odt == F32 else 4e-3, "mean": 1e-6})


def ln_fwd_residual_case(rows, D, ddt, odt, stride=1, path=False):
    B, T, p, br = 6, 17, 0.5, 0  # the drop-path form: rows = B * T, one gate per sample

    def path_of(dev):
        from test_poison_gpu import path_rows

        return path_rows(p, B, T, br, dev)

    def make(dev):
        g, b = affine(D, dev)
        return {"x": randn((rows * stride, D), dev, 90) * 2 + 0.3, "delta": randn((rows, D), dev, 91).to(ddt), "g": g, "b": b}

    def run(d):
        import vit_amd.functional as vf

        xs = E(d["x"].device, rows, D)
        kw = dict(path=(p, PATH_SITE, T, br), seed=path_of(xs.device)[0]) if path else {}
        y, mean, rstd = vf.layernorm_fwd_residual(d["x"], d["delta"], xs, d["g"], d["b"], EPS, out_dtype=odt, x_row_stride=stride, **kw)
        return {"xsum": xs, "y": y, "mean": mean, "rstd": rstd}

    def ref(d):
        delta = d["delta"].float()
        if path:  # p = 0.5: the kept scale 2 is exact
            delta = delta * path_of(d["x"].device)[1]
        xs = d["x"][::stride] + delta  # one f32 add: exact
        return {"xsum": xs.double(), "y": ln_ref(xs, d["g"], d["b"]), "mean": xs.double().mean(-1)}

    between = [("x", others(rows * stride, sl(0, None, stride)))] if stride > 1 else []
    targets, outside = [], []
    for S in row_picks(rows, T if path else 32):
        targets.append([(name, S) for name in ("xsum", "y", "mean", "rstd")])
        outside.append(between + [("x", others(rows, S) * stride), ("delta", others(rows, S))])
    entry = "vit_layernorm_fwd_residual" + ("_path" if path else "_rows" if stride > 1 else "")
    add(f"{entry} ({rows}, {D}) delta {dn(ddt)} y {dn(odt)}" + (f" x_row_stride={stride}" if stride > 1 else ""), entry, make, run,
        targets, outside, ref=ref, tol={"xsum": 0, "y": 1e-6 if odt == F32 else 4e-3, "mean": 1e-6})


def ln_bwd_case(rows, D, dydt, form, ndt=BF16, drop=(0.0, 0, 0), with_dres=True):
    """form: 'plain' (vit_layernorm_bwd), 'fused', 'row_stride' / 'dres_row_stride' (+ '_fused') of vit_layernorm_bwd_rows, 'path'."""
    fused = form in ("fused", "path") or form.endswith("_fused")
    s = 17
    compact = form.startswith("row_stride")      # the tensors hold rows 0, 17, .. of `full` rows
    dres_compact = form.startswith("dres_row_stride")
    full = rows * s if compact else rows
    B, T, p, br = 6, 17, 0.5, 1                  # the drop-path form (rows = B * T)

    def path_of(dev):
        from test_poison_gpu import path_rows

        return path_rows(p, B, T, br, dev)

    def make(dev):
        x = randn((rows, D), dev, 80) * 2 + 0.3
        g, _ = affine(D, dev)
        mean, rstd = stats(x)
        d = {"x": x, "g": g, "mean": mean, "rstd": rstd, "dy": randn((rows, D), dev, 83).to(dydt)}
        if with_dres:
            d["dres"] = randn((-(-rows // s) if dres_compact else rows, D), dev, 84)
        return d

    def run(d):
        import vit_amd.functional as vf

        dev = d["x"].device
        dx, dg, db = E(dev, rows, D), E(dev, D), E(dev, D)
        out = {"dx": dx, "dgamma": dg, "dbeta": db}
        if fused:
            out["dyn"], out["dbias"] = E(dev, rows, D, dt=ndt), E(dev, D)
        args = (d["dy"], d["x"], d["g"], d["mean"], d["rstd"], d.get("dres"), dx, dg, db)
        if form == "plain":
            vf.layernorm_bwd(d["dy"], d["x"], d["g"], d["mean"], d["rstd"], dres=d.get("dres"), dx=dx, dgamma=dg, dbeta=db)
        elif form == "fused":
            vf.layernorm_bwd_fused(*args, out["dyn"], out["dbias"], drop)
        elif form == "path":
            vf.layernorm_bwd_path(*args, out["dyn"], out["dbias"], (p, PATH_SITE, T, br), dropout=(drop[0], path_of(dev)[0], drop[2]))
        else:
            kw = dict(row_stride=s, full_rows=full) if compact else dict(dres_row_stride=s)
            vf.layernorm_bwd_rows(*args, dyn=out.get("dyn"), dbias=out.get("dbias"), dropout=drop, **kw)
        return out

    def ref(d):
        dx, dg, db = ln_bwd_ref(d["dy"], d["x"], d["g"], d["mean"], d["rstd"])
        if with_dres and dres_compact:
            dx[::s] += d["dres"].double()
        elif with_dres:
            dx = dx + d["dres"].double()
        return {"dx": dx, "dgamma": dg, "dbeta": db}

    targets, outside = [], []
    picks = row_picks(rows, T if form == "path" or dres_compact else 32)
    if dres_compact:
        picks.append(others(rows, sl(0, None, s)))  # the rows without a residual gradient: independent of all of dres
    for S in picks:
        o = [(k, others(rows, S)) for k in ("dy", "x", "mean", "rstd")]
        if with_dres and dres_compact:
            has = torch.zeros(rows, dtype=torch.bool)
            has[S] = True
            o.append(("dres", others(-(-rows // s), has[::s].nonzero().view(-1))))
        elif with_dres:
            o.append(("dres", others(rows, S)))
        if torch.is_tensor(S):
            o = [o[-1]]  # dres alone: the other rows are this target's own
        targets.append([(name, S) for name in (("dx", "dyn") if fused else ("dx",))])
        outside.append(o)
    for S in col_picks(D):
        targets.append([("dgamma", S), ("dbeta", S)])
        outside.append([("dy", (ALL, others(D, S))), ("x", (ALL, others(D, S)))])
    entry = {"plain": "vit_layernorm_bwd", "fused": "vit_layernorm_bwd_fused", "path": "vit_layernorm_bwd_path"}.get(form, "vit_layernorm_bwd_rows")
    cid = f"{entry} ({rows}, {D}) dy {dn(dydt)}" + ("" if form in ("plain", "fused", "path") else f" {form}={s}") + \
        (f" dyn {dn(ndt)} p={drop[0]}" if fused else "") + ("" if with_dres else " no dres")
    add(cid, entry, make, run, targets, outside, ref=ref, tol={"dx": 1e-5, "dgamma": 1e-5, "dbeta": 1e-5})


for rows, D in LN_SHAPES:
    for dt in (BF16, F32):
        ln_fwd_case(rows, D, dt)
        ln_fwd_residual_case(rows, D, dt, BF16)
        ln_bwd_case(rows, D, dt, "plain")
        if D <= 1024:  # the fused form keeps a row block in the LDS: D = 2048 is refused by the library
            ln_bwd_case(rows, D, dt, "fused", ndt=dt, drop=(0.1, 321, 9))
    ln_fwd_residual_case(rows, D, BF16, F32)
    ln_bwd_case(rows, D, BF16, "plain", with_dres=False)
    if D <= 1024:
        ln_bwd_case(rows, D, BF16, "fused", drop=(0.0, 0, 0))
for ddt in (BF16, F32):
    ln_fwd_residual_case(6, 192, ddt, BF16, stride=17)
    ln_fwd_residual_case(37, 1024, ddt, F32, stride=3)
    ln_fwd_residual_case(102, 192, ddt, BF16, path=True)
for form, rows in (("row_stride", 6), ("dres_row_stride", 102)):
    for fused in (False, True):
        ln_bwd_case(rows, 192, BF16, form + ("_fused" if fused else ""), drop=(0.1, 321, 9))
ln_bwd_case(35, 1024, F32, "dres_row_stride")
for ph in (0.0, 0.1):
    ln_bwd_case(102, 192, BF16, "path", drop=(ph, 0, 1 + 4 * 5 + 2))


# =================================================================================================== attention
# include/vit_amd.h: the outputs of slice (b, h) depend on the qkv columns of head h in the rows of sample b; the backward adds
# ctx, ctx_lo, dctx and lse of that slice.  Inside a slice, ctx / lse / probs row q depend on Q row q and on all K, V; dQ row q
# and delta row q additionally on dctx, ctx, ctx_lo and lse row q.  dK and dV depend on the whole slice.
@functools.lru_cache(maxsize=None)
def attn_oracle(B, H, T, dh, drop, dt):
    """Inputs and the fp64 forward / autograd backward of one (shape, dropout, dtype), on the host, shared by every case of it."""
    from oracle import dropmask as dm

    D, scale = H * dh, dh ** -0.5
    qkv = randn((B * T, 3 * D), "cpu", 30).to(dt)
    dctx = randn((B * T, D), "cpu", 31).to(dt)
    mask = torch.from_numpy(dm.attn_multiplier(dm.drop_cfg(*drop), B, H, T)).double() if drop[0] else None
    q64 = qkv.double().requires_grad_(True)
    q, k, v = q64.view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    p = s.softmax(-1)
    pd = p if mask is None else p * mask
    ctx = (pd @ v).permute(0, 2, 1, 3).reshape(B * T, D)
    ctx.backward(dctx.double())
    # the documented rounding points of the bf16 forward: P to bf16 before PV, the context to bf16
    pr = pd.detach().to(dt).double()
    ctx_r = (pr @ v.detach()).permute(0, 2, 1, 3).reshape(B * T, D).to(dt).double()
    ctx = ctx.detach()
    c = ctx.to(dt)
    return dict(qkv=qkv, dctx=dctx, ctx64=ctx, ctx_rounded=ctx_r, p64=p.detach(), lse64=torch.logsumexp(s.detach(), -1).reshape(B * H, T),
                grad64=q64.grad, ctx=c, ctx_lo=(ctx - c.double()).to(dt), lse=torch.logsumexp(s.detach(), -1).reshape(B * H, T).float())


def q_picks(T, dh):
    """Query-row ranges inside a slice: the first rows, the last rows (the last partial 64-row tile or its end), the rows around
    a tile boundary.  n rows each, n * dh >= 512 elements: a single bf16 context row is too small a region for the 6e-3 gate
    (rounding P and the context alone gives 3.7e-3 on 16 elements and still 3.06e-3 on 256; tests/test_footprint_cpu.py checks the 2 x room)."""
    n = max(8, -(-512 // dh))
    if T <= 2 * n:
        return [sl(0, T // 2), sl(T // 2, T)] if (T // 2) * dh >= 512 else [sl(0, T)]  # too short to halve: the whole slice's rows
    s = [sl(0, n), sl(T - n, T)]
    if T > 64 + n:
        s.append(sl(64 - n // 2, 64 + n // 2))
    if T % 64 > n and T > 64:
        s.append(sl(T - T % 64, T))
    return s


def slice_picks(B, H, which=None):
    n = B * H
    # the first and the last slice, one in the middle, and the last head of the first sample: the slice whose padded keys are
    # followed in memory by the next sample's first token (the last sample has no such neighbour)
    ids = which if which is not None else sorted({0, H - 1, n // 2, n - 1})
    return [(i // H, i % H) for i in ids]


def attn_case(kind, shape, drop=(0.0, 0, 0), dt=BF16, slices=None, with_lo=True, **opt):
    """kind 'fwd': vit_attention_fwd (+ vit_attention_probs without dropout); 'bwd': vit_attention_bwd on the forward's results as
    inputs (ctx, ctx_lo, lse formed on the host from the fp64 forward, rounded as the forward stores them)."""
    B, H, T, dh = shape
    D, scale = H * dh, dh ** -0.5
    b16 = dt == BF16
    lo = b16 and with_lo
    probs = kind == "fwd" and not drop[0]

    def make(dev):
        o = attn_oracle(B, H, T, dh, drop, dt)
        keys = ("qkv",) if kind == "fwd" else ("qkv", "dctx", "ctx", "lse") + (("ctx_lo",) if lo else ())
        return {k: o[k].to(dev) for k in keys}

    def run(d):
        import vit_amd.functional as vf

        dev = d["qkv"].device
        if kind == "fwd":
            out = {"ctx": E(dev, B * T, D, dt=dt), "lse": E(dev, B * H, T)}
            if lo:
                out["ctx_lo"] = E(dev, B * T, D, dt=dt)
            vf.attention_fwd(d["qkv"], B, H, T, dh, scale, dropout=drop, ctx=out["ctx"], lse=out["lse"], ctx_lo=out.get("ctx_lo"))
            if probs:
                out["probs"] = vf.attention_probs(d["qkv"], B, H, T, dh, scale)
            return out
        out = {"dqkv": E(dev, B * T, 3 * D, dt=dt), "delta": E(dev, B * H, T)}
        vf.attention_bwd(d["qkv"], d["ctx"], d["dctx"], d["lse"], B, H, T, dh, scale, dropout=drop, dqkv=out["dqkv"], delta=out["delta"],
                         ctx_lo=d.get("ctx_lo"))
        return out

    def ref(d):
        o = attn_oracle(B, H, T, dh, drop, dt)
        if kind == "fwd":
            return {"ctx": o["ctx64"], "lse": o["lse64"], "probs": o["p64"]}
        full = d["ctx"].double() + (d["ctx_lo"].double() if lo else 0.0)
        delta = (d["dctx"].double() * full).view(B, T, H, dh).sum(-1).permute(0, 2, 1).reshape(B * H, T)
        return {"dqkv": o["grad64"], "delta": delta}

    def rounded(d):
        return {"ctx": attn_oracle(B, H, T, dh, drop, dt)["ctx_rounded"]}

    def hc(h, parts=(0, 1, 2)):
        return torch.cat([torch.arange(part * D + h * dh, part * D + (h + 1) * dh) for part in parts])

    side = ("ctx", "dctx") + (("ctx_lo",) if lo else ()) if kind == "bwd" else ()
    targets, outside = [], []
    for b, h in slice_picks(B, H, slices):
        rows, hcols = sl(b * T, (b + 1) * T), sl(h * dh, (h + 1) * dh)
        o = [("qkv", others(B * T, rows)), ("qkv", (rows, others(3 * D, hc(h))))]
        for k in side:
            o += [(k, others(B * T, rows)), (k, (rows, others(D, hcols)))]
        if kind == "bwd":
            o.append(("lse", others(B * H, [b * H + h])))
            targets.append([("dqkv", (rows, hc(h))), ("delta", b * H + h)])
        else:
            targets.append([("ctx", (rows, hcols)), ("lse", b * H + h)] + ([("ctx_lo", (rows, hcols))] if lo else []) +
                           ([("probs", (b, h))] if probs else []))
        outside.append(o)
        # single query rows take part in the bit-equality rounds alone (they need no tolerance): a leak between neighbouring
        # rows inside one of the larger regions, which the reference check needs, shows here
        singles = sorted({0, T - 1} | ({63, 64} if T > 64 else set()) | ({T - T % 64} if T % 64 and T > 64 else set()))
        for Q, checked in [(Q, True) for Q in q_picks(T, dh)] + [(sl(q, q + 1), False) for q in singles if T > 1]:
            qrows, rest = sl(b * T + Q.start, b * T + Q.stop), b * T + others(T, Q)
            oq = o + [("qkv", (rest, hcols))] + [(k, (rest, hcols)) for k in side]
            if kind == "bwd":
                oq.append(("lse", (b * H + h, others(T, Q))))
                views = [("dqkv", (qrows, hcols)), ("delta", (b * H + h, Q))]
            else:
                views = [("ctx", (qrows, hcols)), ("lse", (b * H + h, Q))] + ([("ctx_lo", (qrows, hcols))] if lo else []) + \
                    ([("probs", (b, h, Q))] if probs else [])
            targets.append([v + (checked,) for v in views])
            outside.append(oq)
    # tests/test_kernels_gpu.py::test_attention_fwd_bwd and tests/test_poison_gpu.py: 6e-3 / 1.5e-2 in bf16, 1e-5 / 2e-5 in f32
    tol = {"ctx": 6e-3 if b16 else 1e-5, "lse": 1e-5 if b16 else 1e-6, "probs": 1e-5, "dqkv": 1.5e-2 if b16 else 2e-5, "delta": 1e-5}
    entries = ("vit_attention_bwd",) if kind == "bwd" else ("vit_attention_fwd",) + (("vit_attention_probs",) if probs else ())
    names = {"split": ("attn_split", 2), "fused": ("attn_bwd_fused", 4)}
    reserve = opt.pop("reserve", False)
    cid = f"attention {kind} {shape} {dn(dt)} p={drop[0]}" + "".join(f" {k}={v}" for k, v in opt.items()) + \
        (" reserve_cus=8" if reserve else "") + ("" if with_lo or not b16 else " no ctx_lo")
    add(cid, entries, make, run, targets, outside, ref=ref, tol=tol, rounded=rounded if kind == "fwd" and b16 else None,
        context=ctx_of(reserve, **{names[k][0]: (v, names[k][1]) for k, v in opt.items()}))


ATT_DROP = ((0.0, 0, 0), (0.1, 9, 3))
MANY = (0, 255, 256, 299)  # more slices than CUs: consecutive heads of one persistent workgroup
#           shape             slices  forward options     backward options
ATT_BF16 = (((2, 2, 129, 16), None, ({}, {"split": 1}), ({}, {"split": 1})),
            ((2, 3, 5, 64), None, ({}, {"split": 1}), ({},)),
            ((2, 2, 120, 32), None, ({}, {"split": 1}), ({},)),
            ((2, 3, 197, 64), None, ({"split": 1}, {"split": 2}), ({}, {"fused": 0, "split": 1}, {"fused": 0, "split": 2})),
            ((2, 12, 197, 64), (0, 11, 12, 23), ({},), ({}, {"fused": 0})),
            ((3, 2, 65, 64), None, ({},), ({"fused": 4}, {"fused": 0})),
            ((2, 3, 208, 64), None, ({},), ({"fused": 4}, {"fused": 0})),
            ((300, 1, 64, 64), MANY, ({}, {"reserve": True}), ({"fused": 4}, {"fused": 0}, {"reserve": True})),
            ((300, 1, 96, 64), MANY, ({},), ({"fused": 4}, {"fused": 0})),
            ((150, 2, 75, 64), MANY, ({},), ({"fused": 4}, {"fused": 0})),
            ((1, 2, 640, 64), None, ({},), ({},)),
            ((1, 2, 1025, 16), None, ({},), ({},)),
            ((2, 8, 122, 4), None, ({},), ({},)),
            ((2, 3, 130, 12), None, ({},), ({},)),
            ((1, 2, 70, 128), None, ({},), ({},)))
for shape, slices, fopts, bopts in ATT_BF16:
    for drop in ATT_DROP:
        for o in fopts:
            attn_case("fwd", shape, drop, slices=slices, **o)
        for o in bopts:
            attn_case("bwd", shape, drop, slices=slices, **o)
attn_case("fwd", (2, 12, 197, 64), with_lo=False, slices=(0, 11, 12, 23))
attn_case("bwd", (2, 12, 197, 64), with_lo=False, slices=(0, 11, 12, 23))
for shape in ((2, 2, 130, 64), (2, 2, 129, 16)):
    for drop in ATT_DROP:
        attn_case("fwd", shape, drop, dt=F32)
        attn_case("bwd", shape, drop, dt=F32)


# =================================================================================================== GEMM: rope, convenience forms, rows
def gemm_rope_case(cid, M, K, H, dh, T, ncols, core=None):
    """The cos / sin tables belong to every row's footprint (the rotating epilogue steps by a recurrence over table row 8): only
    A's other rows are perturbed."""
    D = H * dh
    N = ncols * D

    def make(dev):
        inv = 1.0 / (10000.0 ** (torch.arange(0, dh, 2).float() / dh))
        fr = torch.outer(torch.arange(T).float(), inv)
        return {"A": bf(randn((M, K), dev, 300, 0.5)), "B": bf(randn((N, K), dev, 301, 0.1)), "bias": randn((N,), dev, 302),
                "cos": fr.cos().contiguous().to(dev), "sin": fr.sin().contiguous().to(dev)}

    def run(d):
        import vit_amd.functional as vf

        return {"C": vf.gemm(d["A"], d["B"], M=M, N=N, K=K, bias=d["bias"], rope=(d["cos"], d["sin"], T, dh, 2 * D))}

    def ref(d):
        from test_poison_gpu import rope_ref

        return {"C": rope_ref(d["A"].double() @ d["B"].double().t() + d["bias"].double(), d["cos"], d["sin"], T, H, dh)}

    picks = row_picks(M, T) + gemm_targets(M, N)[0][3:]
    add(cid, "vit_gemm", make, run, [("C", S) for S in picks], [[("A", others(M, S))] for S in picks], ref=ref, tol={"C": 4e-3},
        context=ctx_of(gemm_core=(core, 1)) if core is not None else None)


gemm_rope_case("gemm rope q/k only (104, 64, 72) generic, pass behind", M=104, K=72, H=2, dh=16, T=13, ncols=2)
gemm_rope_case("gemm rope q/k only (256, 256, 64) ping-pong rotating epilogue", M=256, K=64, H=2, dh=64, T=32, ncols=2, core=5)
gemm_rope_case("gemm rope (1024, 768, 64) ping-pong rotating epilogue", M=1024, K=64, H=4, dh=64, T=197, ncols=3)


def linear_export_case(which):
    """The three convenience exports themselves (vit_amd.functional reaches the same kernels through vit_gemm)."""
    M, N, K = 104, 40, 72

    def make(dev):
        return {"x": bf(randn((M, K), dev, 3)), "W": bf(randn((N, K), dev, 4, 0.1)), "dy": bf(randn((M, N), dev, 7)), "bias": randn((N,), dev, 5)}

    def run(d):
        import vit_amd.functional as vf
        from _poison import active_handle
        from vit_amd._cabi import ACT_NONE, VIT_BF16, VIT_F32

        x, W, dy = d["x"], d["W"], d["dy"]
        dev = x.device
        h, st = active_handle(dev), vf._stream(x)
        if which == "fwd":
            y = E(dev, M, N, dt=BF16)
            h.call("vit_linear_fwd", x.data_ptr(), W.data_ptr(), d["bias"].data_ptr(), y.data_ptr(), VIT_BF16, M, N, K, ACT_NONE, None, 0.0,
                   0, 0, None, st)
        elif which == "bwd_dx":
            y = E(dev, M, K)
            h.call("vit_linear_bwd_dx", dy.data_ptr(), W.data_ptr(), y.data_ptr(), VIT_F32, M, N, K, None, st)
        else:
            y = E(dev, N, K)
            h.call("vit_linear_bwd_dw", dy.data_ptr(), x.data_ptr(), y.data_ptr(), M, N, K, 0, st)
        return {"y": y}

    def ref(d):
        x, W, dy = d["x"].double(), d["W"].double(), d["dy"].double()
        return {"y": x @ W.t() + d["bias"].double() if which == "fwd" else dy @ W if which == "bwd_dx" else dy.t() @ x}

    # y = L R^T-like: rows of y follow `lhs` (its rows, or its columns when it enters transposed), columns follow `rhs`
    lhs, lhs_cols, n_l, rhs, rhs_cols, n_r = {"fwd": ("x", False, M, "W", False, N), "bwd_dx": ("dy", False, M, "W", True, K),
                                              "bwd_dw": ("dy", True, N, "x", True, K)}[which]
    rows, cols = gemm_targets(n_l, n_r)
    targets = [("y", S) for S in rows] + [("y", (ALL, S)) for S in cols]
    outside = [[(lhs, (ALL, others(n_l, S)) if lhs_cols else others(n_l, S))] for S in rows] + \
              [[(rhs, (ALL, others(n_r, S)) if rhs_cols else others(n_r, S))] + ([("bias", others(N, S))] if which == "fwd" else [])
               for S in cols]
    add(f"vit_linear_{which} (104, 40, 72)", f"vit_linear_{which}", make, run, targets, outside, ref=ref,
        tol={"y": 4e-3 if which == "fwd" else 2e-5})


for which in ("fwd", "bwd_dx", "bwd_dw"):
    linear_export_case(which)


def rows_forms_case(which, held, stride, cols, dt=BF16, pad_rows=0):
    """vit_colsum_rows / vit_linear_bwd_dw_rows: compact row j stands for row j * stride of a tensor of full_rows rows; the rows
    between do not exist in the compact form, so what the header promises is tested: a leading dimension wider than the row with
    the gap outside every footprint, and (f32: the full product's route) bit equality with the call over the full tensors of
    full_rows rows, at full_rows = held * stride and at a full_rows padded past it."""
    full = held * stride + pad_rows
    K = 256 if cols % 256 == 0 else 64

    def make(dev):
        d = {"dy": randn((held, cols + (PAD if which == "colsum_rows" else 0)), dev, 32).to(dt)}
        if which != "colsum_rows":
            d["x"] = randn((held, K + PAD), dev, 33).to(dt)
        return d

    def run(d):
        import vit_amd.functional as vf

        if which == "colsum_rows":
            return {"out": vf.colsum_rows(d["dy"][:, :cols], E(d["dy"].device, cols), row_stride=stride, full_rows=full)}
        return {"out": vf.linear_bwd_dw_rows(d["dy"], d["x"], E(d["dy"].device, cols, K), row_stride=stride, full_rows=full, ldx=K + PAD)}

    def ref(d):
        if which == "colsum_rows":
            return {"out": d["dy"][:, :cols].double().sum(0)}
        return {"out": d["dy"].double().t() @ d["x"][:, :K].double()}

    def is_the_full_product(d, out):
        """include/vit_amd.h: f32 operands run the full product's own kernel and split-K plan over full_rows rows, the absent
        rows read as zero (vit_colsum_rows: vit_colsum's order over the full tensor): bit for bit the call over the full tensors,
        at this full_rows -- padded past held * stride or not.  The plan is a function of full_rows, so the header does not
        promise the same bits at two different paddings, and none are asserted."""
        import vit_amd.functional as vf
        from _footprint import _same_bits

        dev = d["dy"].device
        dy_full = torch.zeros((full, cols), dtype=dt, device=dev)
        dy_full[:held * stride:stride] = d["dy"][:, :cols]
        if which == "colsum_rows":
            want = vf.colsum(dy_full)
        else:
            x_full = randn((full, K), dev, 34).to(dt)  # x's other rows are irrelevant: they meet zero rows of dy
            x_full[:held * stride:stride] = d["x"][:, :K]
            want = vf.linear_bwd_dw(dy_full, x_full)
        diff = _same_bits(out["out"], want)
        assert diff == 0, f"{diff} of {want.numel()} elements differ from the call over the full tensors of {full} rows"

    targets, outside = [], []
    for S in col_picks(cols):
        targets.append(("out", S))
        if which == "colsum_rows":
            outside.append([("dy", (ALL, others(cols + PAD, S)))])
        else:
            outside.append([("dy", (ALL, others(cols, S))), ("x", (ALL, sl(K, None)))])
    if which != "colsum_rows":
        for S in col_picks(K):
            targets.append(("out", (ALL, S)))
            outside.append([("x", (ALL, others(K + PAD, S)))])
    add(f"vit_{which} {dn(dt)} held={held} row_stride={stride} full_rows={full} cols={cols} wide ld", f"vit_{which}", make, run, targets,
        outside, ref=ref, tol={"out": 1e-5 if which == "colsum_rows" else gemm_tol(dt, F32)},
        extra=is_the_full_product if dt == F32 and stride > 1 else None)


for which in ("colsum_rows", "linear_bwd_dw_rows"):
    rows_forms_case(which, 16, 64, 256)
    rows_forms_case(which, 6, 17, 192)
    rows_forms_case(which, 16, 64, 256, dt=F32)
    rows_forms_case(which, 16, 64, 256, dt=F32, pad_rows=192)


# =================================================================================================== embedding side
def windows(L, P, S):
    return math.ceil((L - P) / S) + 1


def unfold_case(odt, gather=False):
    """patch (b, n) depends on x[b, n * S : n * S + P]; the ragged tail window is all zero and depends on nothing."""
    B, L, P, S = 3, 1000, 64, 48
    N = windows(L, P, S)
    Kk = 5

    def idx_of():
        from test_patchdrop_gpu import random_idx

        return random_idx(B, N, Kk, 302, must=N - 1)  # the ragged last window is selected

    def make(dev):
        d = {"x": randn((B, L), dev, 40)}
        if gather:
            d["idx"] = idx_of().to(dev)
        return d

    def run(d):
        import vit_amd.functional as vf

        if gather:
            return {"out": vf.unfold_gather_cast(d["x"], d["idx"], P, S, N, out_dtype=odt)}
        return {"out": vf.unfold_cast(d["x"], P, S, N, out_dtype=odt)}

    def ref(d):
        full = d["x"].unfold(1, P, S)
        full = torch.cat([full, torch.zeros(B, N - full.size(1), P, device=full.device)], 1)
        if gather:
            full = torch.gather(full, 1, d["idx"].long()[:, :, None].expand(B, Kk, P))
        return {"out": full.reshape(-1, P).to(odt).double()}

    idx = idx_of()
    per = Kk if gather else N
    picks = [(0, 0), (1, per // 2), (B - 1, per - 2), (B - 1, per - 1)]
    targets, outside = [], []
    for b, k in picks:
        n = int(idx[b, k]) if gather else k
        win = sl(n * S, n * S + P) if n * S + P <= L else sl(0, 0)
        o = [("x", others(B, [b])), ("x", (b, others(L, win)))]
        if gather:
            keep = torch.zeros(B * Kk, dtype=torch.bool)
            keep[b * Kk + k] = True
            o.append(IntIn("idx", (~keep).view(B, Kk), 0, N))
        targets.append(("out", b * per + k))
        outside.append(o)
    name = "vit_unfold_gather_cast" if gather else "vit_unfold_cast"
    add(f"{name} B=3 L=1000 P=64 S=48 {dn(odt)}", name, make, run, targets, outside, ref=ref, tol={"out": 0})


def fold_case(L, P, S, gather=False):
    """dx[b, l] depends on the windows of sample b that cover l and lie inside the signal: the ragged window's row of dpatches,
    and the rows of windows that do not reach the target, are outside."""
    B = 3
    N = windows(L, P, S)
    Kk = N // 2

    def idx_of():
        from test_patchdrop_gpu import random_idx

        return random_idx(B, N, Kk, 351, must=N - 1)

    def slot_of_idx():
        from _patchdrop_ref import slot_of

        return torch.from_numpy(slot_of(idx_of().numpy(), N))

    def make(dev):
        d = {"dp": randn((B * (Kk if gather else N), P), dev, 45)}
        if gather:
            d["slot"] = slot_of_idx().to(dev)
        return d

    def run(d):
        import vit_amd.functional as vf

        if gather:
            return {"dx": vf.fold_add_gather(d["dp"], d["slot"], L, P, S)}
        return {"dx": vf.fold_add(d["dp"], B, L, P, S, N)}

    def ref(d):
        dev = d["dp"].device
        dp = d["dp"].double()
        if gather:
            full = torch.zeros(B, N, P, dtype=torch.float64, device=dev)
            full[torch.arange(B, device=dev)[:, None].expand(B, Kk), idx_of().long().to(dev)] = dp.view(B, Kk, P)
            dp = full
        x = torch.zeros((B, L), dtype=torch.float64, device=dev, requires_grad=True)
        u = x.unfold(1, P, S)
        u = torch.cat([u, torch.zeros(B, N - u.size(1), P, dtype=torch.float64, device=dev)], 1)
        u.backward(dp.view(B, N, P))
        return {"dx": x.grad}

    slot = slot_of_idx() if gather else torch.arange(N).expand(B, N)
    per = Kk if gather else N
    targets, outside = [], []
    for b, (l0, l1) in ((0, (0, 3)), (1, (L // 2 - 3, L // 2 + 4)), (B - 1, (L - 5, L)), (B - 1, ((N - 2) * S - 2, (N - 2) * S + 3))):
        hit = [n for n in range(N) if n * S < l1 and n * S + P > l0 and n * S + P <= L and int(slot[b, n]) >= 0]
        rows = [b * per + int(slot[b, n]) for n in hit]
        targets.append(("dx", (b, sl(l0, l1))))
        outside.append([("dp", others(B * per, rows))])
    name = "vit_fold_add_gather" if gather else "vit_fold_add"
    add(f"{name} B=3 L={L} P={P} S={S}", name, make, run, targets, outside, ref=ref, tol={"dx": 1e-6})


for odt in (BF16, F32):
    unfold_case(odt)
    unfold_case(odt, gather=True)
fold_case(1000, 64, 48)
fold_case(250, 16, 8)
fold_case(250, 16, 8, gather=True)


def embed_case(form, bwd, B=4, N=12, D=32, p=0.1):
    """vit_embed_finish / _gather / _masked / _reg (in place) and their backwards.  form: 'plain', 'gather', 'masked', 'reg'
    (registers, no mask), 'reg_masked'.  Token row (b, t) depends on its own row and on cls / pos[its position] / reg /
    mask_token -- and not even on its own row where that row is replaced (CLS, a register, a masked patch).  dpatch row (b, n)
    depends on dtokens row (b, 1 + R + n), dpos row t on rows t of every sample, dcls on rows 0, dreg on the register rows,
    dmask_token on the masked patch rows."""
    R = 3 if form.startswith("reg") else 0
    masked = form in ("masked", "reg_masked")
    gather = form == "gather"
    T = 1 + R + N
    T_full = 1 + 2 * N if gather else 1 + N  # gather: N of 2N patches are kept
    drop = (p, 5, 1)

    @functools.lru_cache(maxsize=None)
    def idx_of():
        from test_patchdrop_gpu import random_idx

        return random_idx(B, 2 * N, N, 321)

    @functools.lru_cache(maxsize=None)
    def mask_of():
        m = (rand((B, N), "cpu", 77) < 0.5).to(torch.int32) * 7
        m[0, 0], m[-1, -1] = 7, 0
        return m

    def posrow(b, t):  # the row of pos a token takes, None for a register
        if t == 0:
            return 0
        if t <= R:
            return None
        return 1 + int(idx_of()[b, t - 1]) if gather else t - R

    def make(dev):
        d = {"tok": randn((B * T, D), dev, 44)}
        if not bwd:
            d.update(cls=randn((D,), dev, 45), pos=randn((T_full, D), dev, 46))
            if R:
                d["reg"] = randn((R, D), dev, 47)
            if masked:
                d["mt"] = randn((D,), dev, 48)
        return d

    def run(d):
        import vit_amd.functional as vf
        from _patchdrop_ref import slot_of

        tok = d["tok"].view(B, T, D)
        dev = tok.device
        mask = mask_of().to(dev) if masked else None
        if not bwd:
            if gather:
                vf.embed_finish_gather(tok, d["cls"], idx_of().to(dev), T_full, pos=d["pos"], dropout=drop)
            elif form == "plain":
                vf.embed_finish(tok, d["cls"], pos=d["pos"], dropout=drop)
            elif form == "masked":
                vf.embed_finish_masked(tok, d["cls"], mask, d["mt"], pos=d["pos"], dropout=drop)
            else:
                vf.embed_finish_reg(tok, R, d["cls"], d["reg"], pos=d["pos"], mask=mask, mask_token=d.get("mt"), dropout=drop)
            return {"tok": d["tok"]}
        out = {"dcls": E(dev, D), "dpos": E(dev, T_full, D)}
        if masked:
            out["dmt"] = E(dev, D)
        if R:
            out["dreg"] = E(dev, R, D)
        if gather:
            slot = torch.from_numpy(slot_of(idx_of().numpy(), 2 * N)).to(dev)
            out["dpatch"] = vf.embed_finish_gather_bwd(tok, slot, out["dcls"], out["dpos"], dropout=drop)
        elif form == "plain":
            out["dpatch"] = vf.embed_finish_bwd(tok, out["dcls"], out["dpos"], dropout=drop)
        elif form == "masked":
            out["dpatch"] = vf.embed_finish_masked_bwd(tok, mask, out["dcls"], out["dmt"], dpos=out["dpos"], dropout=drop)
        else:
            out["dpatch"] = vf.embed_finish_reg_bwd(tok, R, out["dcls"], out["dreg"], dpos=out["dpos"], mask=mask, dmask_token=out.get("dmt"),
                                                    dropout=drop)
        return out

    def ref(d):
        dev = d["tok"].device
        mult = drop_mult(drop, B * T, D, dev).view(B, T, D)
        pr = torch.tensor([[-1 if posrow(b, t) is None else posrow(b, t) for t in range(T)] for b in range(B)], device=dev)
        mask = mask_of().to(dev) != 0 if masked else torch.zeros(B, N, dtype=torch.bool, device=dev)
        if not bwd:
            v = d["tok"].view(B, T, D).clone()
            v[:, 0] = d["cls"]
            if R:
                v[:, 1:1 + R] = d["reg"]
            if masked:
                v[:, 1 + R:] = torch.where(mask[:, :, None], d["mt"].view(1, 1, D), v[:, 1 + R:])
            v = v + torch.where((pr >= 0)[:, :, None], d["pos"][pr.clamp(min=0)], torch.zeros((), device=dev))  # one f32 add
            return {"tok": (v * mult).view(B * T, D).double()}  # one f32 multiply: the kernel's own two roundings
        g = d["tok"].view(B, T, D).double() * mult.double()
        gp = g[:, 1 + R:]
        out = {"dpatch": torch.where(mask[:, :, None], torch.zeros((), dtype=torch.float64, device=dev), gp).reshape(B * N, D),
               "dcls": g[:, 0].sum(0), "dmt": torch.where(mask[:, :, None], gp, torch.zeros((), dtype=torch.float64, device=dev)).sum((0, 1))}
        dpos = torch.zeros(T_full, D, dtype=torch.float64, device=dev)
        for b in range(B):
            for t in range(T):
                if posrow(b, t) is not None:
                    dpos[posrow(b, t)] += g[b, t]
        out["dpos"] = dpos
        if R:
            out["dreg"] = g[:, 1:1 + R].sum(0)
        return out

    flat = lambda b, t: b * T + t
    replaced = [flat(b, t) for b in range(B) for t in range(T)
                if t <= R or (masked and int(mask_of()[b, t - 1 - R]) != 0)]  # input rows the forward never reads
    targets, outside = [], []
    if not bwd:
        for S in ([flat(0, 0)], [flat(B - 1, T - 1)], [flat(1, T - 1), flat(2, 0), flat(2, 1)], [flat(0, 1 + R)],
                  [flat(b, t) for b in range(B) for t in range(1, 1 + R)] or [flat(B // 2, T // 2)]):
            used = {posrow(r // T, r % T) for r in S} - {None}
            o = [("tok", others(B * T, [r for r in S if r not in replaced])), ("pos", others(T_full, sorted(used)))]
            if R and not any(1 <= r % T <= R for r in S):
                o.append(("reg", ALL))
            if masked and not any(r in replaced and r % T > R for r in S):
                o.append(("mt", ALL))
            if not any(r % T == 0 for r in S):
                o.append(("cls", ALL))
            targets.append(("tok", torch.tensor(S)))
            outside.append(o)
    else:
        for S in ([0], [B * N - 1], [N - 1, N, N + 1]):
            src = [flat(n // N, 1 + R + n % N) for n in S if not (masked and int(mask_of()[n // N, n % N]) != 0)]
            targets.append(("dpatch", torch.tensor(S)))
            outside.append([("tok", others(B * T, src))])
        if masked:  # the masked rows are exact zeros and depend on nothing; dmask_token depends on the masked patch rows alone
            zero_rows = mask_of().view(-1).nonzero().view(-1)
            targets.append(("dpatch", zero_rows))
            outside.append([("tok", ALL)])
            targets.append(("dmt", ALL))
            outside.append([("tok", others(B * T, [flat(int(n) // N, 1 + R + int(n) % N) for n in zero_rows]))])
        targets.append(("dcls", ALL))
        outside.append([("tok", others(B * T, [flat(b, 0) for b in range(B)]))])
        if R:
            targets.append(("dreg", ALL))
            outside.append([("tok", others(B * T, [flat(b, t) for b in range(B) for t in range(1, 1 + R)]))])
        for prow in (0, 1, T_full - 1, T_full // 2):
            targets.append(("dpos", prow))
            outside.append([("tok", others(B * T, [flat(b, t) for b in range(B) for t in range(T) if posrow(b, t) == prow]))])
    entry = {"plain": "vit_embed_finish", "gather": "vit_embed_finish_gather", "masked": "vit_embed_finish_masked"}.get(form, "vit_embed_finish_reg")
    entry += "_bwd" if bwd else ""
    add(f"{entry} ({B}, {T}, {D}) p={p}" + (" with a mask" if form == "reg_masked" else ""), entry, make, run, targets, outside, ref=ref,
        tol={"tok": 0, "dpatch": 4e-3, "dcls": 1e-6, "dpos": 1e-6, "dmt": 1e-6, "dreg": 1e-6})


for form in ("plain", "gather", "masked", "reg", "reg_masked"):
    for bwd in (False, True):
        embed_case(form, bwd)
embed_case("plain", False, B=3, N=128, D=32, p=0.0)
embed_case("plain", True, B=20, N=16, D=64, p=0.0)


def rows_gather_case():
    B, N, Kk, W = 3, 40, 17, 8

    def idx_of():
        from test_patchdrop_gpu import random_idx

        return random_idx(B, N, Kk, 341)

    def make(dev):
        return {"table": randn((N + 1, W), dev, 343), "idx": idx_of().to(dev)}

    def run(d):
        import vit_amd.functional as vf

        return {"out": vf.rows_gather(d["table"], d["idx"])}

    def ref(d):
        from _patchdrop_ref import positions

        pos = torch.from_numpy(positions(idx_of().numpy())).to(d["table"].device)
        return {"out": d["table"][pos].view(B * (Kk + 1), W).double()}

    targets, outside = [], []
    for b, t in ((0, 0), (0, 1), (1, Kk // 2), (B - 1, Kk)):
        keep = torch.zeros(B, Kk, dtype=torch.bool)
        if t:
            keep[b, t - 1] = True
        targets.append(("out", b * (Kk + 1) + t))
        outside.append([("table", others(N + 1, [0 if t == 0 else 1 + int(idx_of()[b, t - 1])])), IntIn("idx", ~keep, 0, N)])
    add("vit_rows_gather (3, 17) of 41 rows", "vit_rows_gather", make, run, targets, outside, ref=ref, tol={"out": 0})


rows_gather_case()


def patch_slot_case():
    B, N, Kk = 4, 13, 3

    def make(dev):
        from test_patchdrop_gpu import random_idx

        return {"idx": random_idx(B, N, Kk, 305).to(dev)}

    def run(d):
        import vit_amd.functional as vf

        return {"slot": vf.patch_slot(d["idx"], torch.empty((B, N), dtype=torch.int32, device=d["idx"].device))}

    def ref(d):
        from _patchdrop_ref import slot_of

        return {"slot": torch.from_numpy(slot_of(d["idx"].cpu().numpy(), N)).double()}

    add("vit_patch_slot (4, 13, 3)", "vit_patch_slot", make, run, [("slot", b) for b in range(B)],
        [[IntIn("idx", others(B, [b]), 0, N)] for b in range(B)], ref=ref, tol={"slot": 0})


patch_slot_case()


def mim_mask_case():
    B, N, span = 4, 29, 4
    Nb = -(-N // span)

    def make(dev):
        g = torch.Generator().manual_seed(9)
        return {"slot": (torch.randint(0, 3, (B, Nb), generator=g) - 1).to(torch.int32).to(dev)}  # -1: masked, else a slot number

    def run(d):
        import vit_amd.functional as vf

        return {"mask": vf.mim_mask(d["slot"], span, torch.empty((B, N), dtype=torch.int32, device=d["slot"].device))}

    def ref(d):
        return {"mask": (d["slot"][:, torch.arange(N) // span] < 0).double()}

    targets, outside = [], []
    for b, (n0, n1) in ((0, (0, 1)), (1, (3, 5)), (2, (14, 16)), (B - 1, (N - 1, N))):
        keep = torch.zeros(B, Nb, dtype=torch.bool)
        keep[b, n0 // span:(n1 - 1) // span + 1] = True
        targets.append(("mask", (b, sl(n0, n1))))
        outside.append([IntIn("slot", ~keep, -1, 2)])
    add("vit_mim_mask (4, 29) span=4", "vit_mim_mask", make, run, targets, outside, ref=ref, tol={"mask": 0})


mim_mask_case()


def mim_loss_bwd_case(kind, pdt, norm):
    """dpred row (b, 1 + n) of a masked window depends on pred's row, the window of x, and the scalars count / dloss; the CLS rows
    and the rows of unmasked windows are exact zeros whatever pred and x hold.  The mask is held fixed (count depends on all of it)."""
    B, L, P, S = 3, 250, 16, 8
    N = windows(L, P, S)
    T = N + 1

    def mask_of():
        m = (rand((B, N), "cpu", 78) < 0.5).to(torch.int32)
        m[0, 0], m[1, 5], m[-1, -1], m[-1, -2], m[0, 1] = 1, 1, 1, 1, 0
        return m

    def make(dev):
        return {"x": randn((B, L), dev, 60), "pred": randn((B * T, P), dev, 61).to(pdt)}

    def run(d):
        import vit_amd.functional as vf
        from vit_amd._cabi import LOSS_L1, LOSS_MSE

        dev = d["x"].device
        m = mask_of().to(dev)
        count = m.sum().to(torch.int32).reshape(())
        dloss = torch.full((1,), 1.7, device=dev)
        return {"dpred": vf.mim_loss_bwd(d["x"], d["pred"], m, count, dloss, P, S, LOSS_L1 if kind == "l1" else LOSS_MSE, norm_target=norm,
                                         out_dtype=pdt)}

    def ref(d):
        dev = d["x"].device
        m = mask_of().to(dev)
        x = d["x"].double()
        t = torch.zeros(B, N, P, dtype=torch.float64, device=dev)
        for n in range(N):
            if n * S + P <= L:
                t[:, n] = x[:, n * S:n * S + P]
        if norm:
            t = (t - t.mean(-1, keepdim=True)) / torch.sqrt(t.var(-1, unbiased=True, keepdim=True) + 1e-6)
        dd = d["pred"].double().view(B, T, P)[:, 1:] - t
        g = (torch.sign(dd) if kind == "l1" else 2 * dd) * (1.7 / (max(1, int(m.sum())) * P)) * (m != 0)[:, :, None]
        out = torch.zeros(B, T, P, dtype=torch.float64, device=dev)
        out[:, 1:] = g
        return {"dpred": out.view(B * T, P)}

    m = mask_of()
    targets, outside = [], []
    for b, n in ((0, 0), (1, 5), (B - 1, N - 2), (B - 1, N - 1)):  # the last one is the ragged window: its reconstruction target is all zero, whatever x holds
        win = sl(n * S, n * S + P) if n * S + P <= L else sl(0, 0)
        targets.append(("dpred", b * T + 1 + n))
        outside.append([("pred", others(B * T, [b * T + 1 + n])), ("x", others(B, [b])), ("x", (b, others(L, win)))])
    zero = torch.tensor([b * T + t for b in range(B) for t in range(T) if t == 0 or int(m[b, t - 1]) == 0])
    targets.append(("dpred", zero))
    outside.append([("pred", ALL), ("x", ALL)])
    add(f"vit_mim_loss_bwd (3, 250) P=16 S=8 {kind} pred {dn(pdt)}" + (" norm_target" if norm else ""), "vit_mim_loss_bwd", make, run,
        targets, outside, ref=ref, tol={"dpred": 1e-5 if pdt == F32 else 4e-3})


for kind, pdt, norm in (("l1", F32, False), ("mse", F32, False), ("mse", BF16, True), ("l1", BF16, False)):
    mim_loss_bwd_case(kind, pdt, norm)


def rope_qk_case(dt):
    """In place on [rows, 3 * H * dh]: row r and head h of the q and k thirds depend on themselves and on table row r % T; the v
    third is outside every footprint and stays unwritten."""
    B, T, H, dh = 3, 13, 2, 16
    D, rows = H * dh, B * T

    def make(dev):
        inv = 1.0 / (10000.0 ** (torch.arange(0, dh, 2).float() / dh))
        fr = torch.outer(torch.arange(T).float(), inv)
        return {"qkv": randn((rows, 3 * D), dev, 70).to(dt), "cos": fr.cos().contiguous().to(dev), "sin": fr.sin().contiguous().to(dev)}

    def run(d):
        import vit_amd.functional as vf

        v_in = d["qkv"][:, 2 * D:].clone()
        vf.rope_qk(d["qkv"], d["cos"], d["sin"], T, H, dh)
        return {"qkv": d["qkv"], "v_in": v_in}

    def v_untouched(out):
        from _footprint import _same_bits

        assert _same_bits(out["qkv"][:, 2 * D:], out["v_in"]) == 0, "vit_rope_qk wrote the v third"

    def ref(d):
        from test_poison_gpu import rope_ref

        return {"qkv": rope_ref(d["qkv"].double(), d["cos"], d["sin"], T, H, dh)}

    targets, outside = [], []
    for S, h in ((sl(0, 1), 0), (sl(rows - 1, rows), H - 1), (sl(T - 1, T + 2), 0), (sl(rows // 2, rows // 2 + 2), 1)):
        cols = torch.cat([torch.arange(part * D + h * dh, part * D + (h + 1) * dh) for part in (0, 1)])
        used = sorted({r % T for r in range(rows)[S]})
        targets.append(("qkv", (S, cols)))
        outside.append([("qkv", others(rows, S)), ("qkv", (S, others(3 * D, cols))), ("cos", others(T, used)), ("sin", others(T, used))])
    add(f"vit_rope_qk (39, 96) T=13 {dn(dt)}", "vit_rope_qk", make, run, targets, outside, ref=ref, tol={"qkv": 4e-3 if dt == BF16 else 2e-5},
        every_round=v_untouched)


for dt in (BF16, F32):
    rope_qk_case(dt)


def token_pool_case(bwd, first):
    B, T, D = 3, 19, 36

    def make(dev):
        return {"dp": randn((B, D), dev, 81)} if bwd else {"x": randn((B * T, D), dev, 80)}

    def run(d):
        import vit_amd.functional as vf

        if bwd:
            return {"dx": vf.token_pool_bwd(d["dp"], E(d["dp"].device, B, T, D), first).view(B * T, D)}
        return {"pooled": vf.token_pool_fwd(d["x"].view(B, T, D), first)}

    def ref(d):
        if bwd:
            out = (d["dp"].double() / (T - first))[:, None].expand(B, T, D).clone()
            out[:, :first] = 0
            return {"dx": out.reshape(B * T, D)}
        return {"pooled": d["x"].double().view(B, T, D)[:, first:].mean(1)}

    def front_is_zero(out):
        assert bool((out["dx"].view(B, T, D)[:, :first] == 0).all()), "rows in front of `first` are not exact zeros"

    targets, outside = [], []
    for b in range(B):
        if bwd:
            targets.append(("dx", sl(b * T, (b + 1) * T)))
            outside.append([("dp", others(B, [b]))])
        else:  # rows in front of `first` (CLS, the registers) are outside every footprint
            targets.append(("pooled", b))
            outside.append([("x", others(B * T, sl(b * T + first, (b + 1) * T)))])
    for S in col_picks(D)[:3]:
        targets.append(("dx", (ALL, S)) if bwd else ("pooled", (ALL, S)))
        outside.append([("dp" if bwd else "x", (ALL, others(D, S)))])
    add(f"vit_token_pool_{'bwd' if bwd else 'fwd'} (3, 19, 36) first={first}", f"vit_token_pool_{'bwd' if bwd else 'fwd'}", make, run, targets,
        outside, ref=ref, tol={"pooled": 1e-6, "dx": 1e-6}, every_round=front_is_zero if bwd else None)


for first in (1, 4):
    token_pool_case(False, first)
    token_pool_case(True, first)


def mix_case(which):
    """include/vit_amd_mix.h: the partner of sample b is B - 1 - b; out[b, i] is x[p, i] inside the row's span, x[b, i] where
    u == 0 or p == b (x[p] is not read for it), else mixed.  Rows other than b and p are outside every footprint of out[b]."""
    f32_ = lambda v: float(np.float32(v))
    B, L, Cn = 5, 203, 7
    w = f32_(0.37)
    IDENT = (1.0, 0.0, 0, 0, 1.0, 0.0)
    rows = [IDENT, (w, f32_(1 - 0.37), 0, 0, w, f32_(1 - 0.37)), IDENT, (1.0, 0.0, 3, 10, f32_(0.75), f32_(0.25)),
            (1.0, 0.0, 100, 107, 0.0, 1.0)]

    def make(dev):
        if which == "signal":
            return {"x": randn((B, L), dev, 100)}
        if which == "targets_reg":
            return {"y": rand((B, 3), dev, 23)}
        return {"y": torch.randint(0, Cn, (B,), generator=torch.Generator().manual_seed(37)).to(dev)}

    def run(d):
        import vit_amd.functional as vf
        from test_mix_gpu import device_plan

        t = d["x"] if which == "signal" else d["y"]
        plan = device_plan(t.device, rows)
        if which == "signal":
            return {"out": vf.mix_signal(t, plan, B)}
        if which == "targets_reg":
            return {"out": vf.mix_targets(t, plan, B)}
        return {"out": vf.mix_targets(t, plan, B, Cn, 0.9 + 0.1 / Cn, 0.1 / Cn)}

    def ref(d):
        if which == "signal":
            x = d["x"].double()
            out = torch.empty_like(x)
            for b, (ww, u, lo, hi, _, _) in enumerate(rows):
                out[b] = ww * x[b] + u * x[B - 1 - b] if u else x[b]
                out[b, lo:hi] = x[B - 1 - b, lo:hi]
            return {"out": out}
        y = d["y"]
        if which == "targets_cls":
            on, off = np.float32(0.9 + 0.1 / Cn), np.float32(0.1 / Cn)
            oh = torch.full((B, Cn), float(off), dtype=torch.float64, device=y.device)
            oh[torch.arange(B), y] = float(on)
            y = oh
        y = y.double()
        return {"out": torch.stack([wy * y[b] + uy * y[B - 1 - b] for b, (_, _, _, _, wy, uy) in enumerate(rows)])}

    targets, outside = [], []
    for b, (ww, u, lo, hi, wy, uy) in enumerate(rows):
        p = B - 1 - b
        if which == "signal":
            o = [("x", others(B, [b, p]))]
            if p != b and lo < hi:  # CutMix: the sample's own span and the partner outside the span are not read
                o += [("x", (b, sl(lo, hi))), ("x", (p, others(L, sl(lo, hi))))]
            elif p != b and not u:
                o.append(("x", p))
            targets.append(("out", b))
            outside.append(o)
        elif which == "targets_reg":
            targets.append(("out", b))
            outside.append([("y", others(B, [b] if not uy else [b, p]))])
        else:
            targets.append(("out", b))
            outside.append([IntIn("y", others(B, [b] if not uy else [b, p]), 0, Cn)])
    if which == "signal":  # element ranges of a mixed row: unaligned ends, the row's tail
        for rng in (sl(1, 6), sl(L - 3, L)):
            targets.append(("out", (1, rng)))
            outside.append([("x", others(B, [1, 3])), ("x", (1, others(L, rng))), ("x", (3, others(L, rng)))])
    entry = "vit_mix_signal" if which == "signal" else "vit_mix_targets"
    add(f"{entry} {which} B=5", entry, make, run, targets, outside, ref=ref, tol={"out": 1e-6})


for which in ("signal", "targets_reg", "targets_cls"):
    mix_case(which)


# =================================================================================================== head + loss
HEAD_T, HEAD_D = 6, 192


def head_inputs(kind, B, Cn, dev, T=HEAD_T):
    from vit_amd._cabi import LOSS_BCE, LOSS_CE, LOSS_L1, LOSS_MSE, LOSS_SOFT_CE

    gen = torch.Generator(device="cpu").manual_seed(63)
    if kind == "ce":
        labels = torch.randint(0, Cn, (B,), generator=gen)
    elif kind == "soft_ce":
        labels = torch.rand((B, Cn), generator=gen).softmax(-1)
    else:
        labels = torch.rand((B, Cn) if Cn > 1 or kind == "bce" else (B,), generator=gen)
    return {"last": randn((B * T, HEAD_D), dev, 60), "W": randn((Cn, HEAD_D), dev, 61, 0.1), "b": randn((Cn,), dev, 62, 0.1),
            "labels": labels.to(dev), "code": {"mse": LOSS_MSE, "l1": LOSS_L1, "ce": LOSS_CE, "soft_ce": LOSS_SOFT_CE, "bce": LOSS_BCE}[kind]}


def head_loss_of(kind, lg, labels):
    if kind == "ce":
        return F.cross_entropy(lg, labels)
    if kind == "l1":
        return F.l1_loss(lg.view(-1), labels.double().view(-1))
    if kind == "mse":
        return F.mse_loss(lg.view(-1), labels.double().view(-1))
    if kind == "soft_ce":
        return -(labels.double() * lg.log_softmax(-1)).sum(-1).mean()
    return F.binary_cross_entropy_with_logits(lg, labels.double())


def head_case(kind, B, Cn, bwd, T=HEAD_T):
    """vit_head_loss_fwd: logits of sample b depend on last_hidden[b, 0, :] (the CLS row), W and b: rows t >= 1 are outside every
    footprint.  vit_head_loss_bwd (logits are an input): dlast_hidden rows of sample b depend on logits[b] and labels[b] -- and are
    exactly zero outside the CLS rows in every round; dW's columns S depend on columns S of the CLS rows.
    T = 1 is the pooled form (model.global_pool avg: the engine hands the head a [B, 1, D] tensor of pooled rows): every row is
    then a sample's own, and the rows of the other samples are outside its footprint."""
    D = HEAD_D

    def make(dev):
        d = head_inputs(kind, B, Cn, dev, T)
        if bwd:
            d["logits"] = F.linear(d["last"].view(B, T, D)[:, 0], d["W"], d["b"])
        return d

    def run(d):
        import vit_amd.functional as vf

        last = d["last"].view(B, T, D)
        if not bwd:
            return {"logits": vf.head_loss_fwd(last, d["W"], d["b"], d["labels"], d["code"])[0]}
        dlast, dW, db = vf.head_loss_bwd(last, d["W"], d["logits"], d["labels"], torch.full((1,), 1.7, device=last.device), d["code"])
        return {"dlast": dlast.view(B * T, D), "dW": dW, "db": db}

    def ref(d):
        cls = d["last"].double().view(B, T, D)[:, 0]
        if not bwd:
            return {"logits": F.linear(cls, d["W"].double(), d["b"].double())}
        lg = d["logits"].double().requires_grad_(True)
        (head_loss_of(kind, lg, d["labels"]) * 1.7).backward()
        dlast = torch.zeros(B, T, D, dtype=torch.float64, device=cls.device)
        dlast[:, 0] = lg.grad @ d["W"].double()
        return {"dlast": dlast.view(B * T, D), "dW": lg.grad.t() @ cls, "db": lg.grad.sum(0)}

    def only_cls_rows(out):
        assert bool((out["dlast"].view(B, T, D)[:, 1:] == 0).all()), "dlast_hidden is not exactly zero outside the CLS rows"

    noncls = others(B * T, sl(0, None, T))
    targets, outside = [], []
    for S in row_picks(B, 16):
        rest = others(B, S)
        if not bwd:
            targets.append(("logits", S))
            outside.append([("last", noncls), ("last", rest * T)])
        else:
            lab = [IntIn("labels", rest, 0, Cn)] if kind == "ce" else [("labels", rest)]
            targets.append(("dlast", sl(S.start * T, S.stop * T)))
            outside.append([("last", ALL), ("logits", rest)] + lab)
    if bwd:
        for S in col_picks(D)[:3]:
            targets.append(("dW", (ALL, S)))
            outside.append([("last", noncls), ("last", (ALL, others(D, S)))])
        targets.append(("db", ALL))
        outside.append([("last", ALL)])
    entry = "vit_head_loss_bwd" if bwd else "vit_head_loss_fwd"
    add(f"{entry} {kind} B={B} C={Cn}" + (" pooled rows (T=1)" if T == 1 else ""), entry, make, run, targets, outside, ref=ref,
        tol={"logits": 1e-5, "dlast": 1e-5, "dW": 1e-5, "db": 1e-5}, every_round=only_cls_rows if bwd else None)


for B in (37, 300):
    for kind, Cn in (("mse", 1), ("l1", 3), ("ce", 5), ("soft_ce", 10), ("soft_ce", 130), ("bce", 10), ("bce", 130)):
        if B == 37 or Cn in (5, 130):
            head_case(kind, B, Cn, False)
            head_case(kind, B, Cn, True)
        if B == 37:
            head_case(kind, B, Cn, False, T=1)
            head_case(kind, B, Cn, True, T=1)


# =================================================================================================== optimizers
# include/vit_amd_optim.h: element i of p, m, v and the bf16 shadow depends on element i of the inputs, on the scalars and on
# sqnorm (a device scalar, held fixed); with a group table, on its own group's row and on no other row.  LAMB: on its own
# tensor (segment), through the trust ratio, and on no other tensor.
OPT_N, OPT_CUT = 1003, 500  # n = 4 k + 3: a vector tail; two segments [0, 500) and [500, 1003)
OPT_GROUPS = ((1e-3, 0.01, 0.9), (5e-4, 0.0, 0.5), (7e-4, 0.02, 0.3))  # (lr, weight_decay, momentum); the third owns nothing
OPT_RANGES = (sl(0, 1), sl(333, 350), sl(OPT_CUT - 3, OPT_CUT + 3), sl(OPT_N - 3, OPT_N), sl(OPT_N - 6, OPT_N - 1))
MAX_NORM = 1.0


def opt_case(kind, groups=False, dyn=False):
    lamb = kind == "lamb"
    state = ("p", "g", "m") + (() if kind == "sgd" else ("v",))

    def make(dev):
        d = {"p": randn((OPT_N,), dev, 1), "g": randn((OPT_N,), dev, 2, 0.1), "m": randn((OPT_N,), dev, 3, 0.05)}
        if kind != "sgd":
            d["v"] = randn((OPT_N,), dev, 4, 0.05).abs()
        d["sqnorm"] = (d["g"].double() ** 2).sum().float().reshape(1)
        if groups:
            d["groups"] = torch.tensor([list(r) + [0.0] for r in OPT_GROUPS], dtype=F32).to(dev)
        return d

    def run(d):
        import vit_amd.functional as vf
        from test_poison_gpu import bound_record, nothing

        p, g, m, v = d["p"], d["g"], d["m"], d.get("v")
        dev = p.device
        pb = E(dev, OPT_N, dt=BF16)
        out = {"p": p, "m": m, "p_bf16": pb}
        if v is not None:
            out["v"] = v
        clip = dict(sqnorm=d["sqnorm"], max_norm=MAX_NORM)
        lr, wd, mo = OPT_GROUPS[0]
        with bound_record(dev) if dyn else nothing() as rec:
            if dyn:
                rec.advance()
            if groups:
                triples = [(0, OPT_CUT, 0), (OPT_CUT, OPT_N - OPT_CUT, 1)]
                tables = (vf.optim_param_tables if lamb else vf.optim_group_tables)(triples, len(OPT_GROUPS), dev, total=OPT_N)
                tables.groups = d["groups"]
            if lamb:
                out["trust"] = E(dev, 2 if groups else 1)
                if groups:
                    vf.lamb_step_groups(p, g, m, v, pb, tables, out["trust"], step=1, dyn=dyn, **clip)
                else:
                    vf.lamb_step(p, g, m, v, pb, lr=lr, weight_decay=wd, step=1, trust=out["trust"], **clip)
            elif kind == "sgd" and groups:
                vf.sgd_step_groups(p, g, m, pb, tables, nesterov=True, dyn=dyn, **clip)
            elif kind == "sgd":
                vf.sgd_step(p, g, m, pb, lr=lr, momentum=mo, weight_decay=wd, nesterov=True, **clip)
            elif groups:
                vf.adamw_step_groups(p, g, m, v, pb, tables, step=1, l2=kind == "adam_l2", dyn=dyn, **clip)
            else:
                (vf.adamw_step if kind == "adamw" else vf.adam_l2_step)(p, g, m, v, pb, lr=lr, weight_decay=wd, step=1, **clip)
        return out

    def ref(d):
        """The header's arithmetic in fp64, one step at step = 1 from the given state."""
        p, g, m = d["p"].double(), d["g"].double(), d["m"].double()
        dev = p.device
        clip = min(1.0, MAX_NORM / (math.sqrt(float(d["sqnorm"].double())) + 1e-6))
        rows = torch.tensor(OPT_GROUPS, dtype=torch.float64, device=dev)
        own = (torch.arange(OPT_N, device=dev) >= OPT_CUT).long() if groups else torch.zeros(OPT_N, dtype=torch.long, device=dev)
        lr, wd, mo = (rows[own, i] for i in range(3))
        b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
        if kind == "sgd":
            g2 = g * clip + wd * p
            m2 = mo * m + g2
            return {"p": p - lr * (g2 + mo * m2), "m": m2}
        v = d["v"].double()
        g2 = g * clip + (wd * p if kind == "adam_l2" else 0.0)
        om2 = 1.0 - 0.999 if kind == "adam_l2" else 1.0 - b2  # vit_adam_l2_step reads the betas back as torch's doubles
        om1 = 1.0 - 0.9 if kind == "adam_l2" else 1.0 - b1
        m2, v2 = b1 * m + om1 * g2, b2 * v + om2 * g2 * g2
        eps = 1e-6 if lamb else 1e-8
        u = (m2 / (1 - b1)) / (torch.sqrt(v2) / math.sqrt(1 - b2) + float(np.float32(eps)))
        if lamb:
            u = u + wd * p
            pn = p.clone()
            for seg in ((sl(0, OPT_CUT), sl(OPT_CUT, OPT_N)) if groups else (sl(0, OPT_N),)):
                r = float(p[seg].norm() / u[seg].norm()) if float(wd[seg][0]) != 0 else 1.0
                pn[seg] = p[seg] - lr[seg] * r * u[seg]
            return {"p": pn, "m": m2, "v": v2}
        if kind == "adamw":
            p = p * (1 - lr * wd)
        return {"p": p - lr * u, "m": m2, "v": v2}

    targets, outside = [], []
    if lamb:
        segs = (sl(0, OPT_CUT), sl(OPT_CUT, OPT_N)) if groups else ()
        for i, S in enumerate(segs):  # one tensor's range: the other tensor is outside (the per-tensor trust ratio)
            targets.append([(k, S) for k in ("p", "m", "v", "p_bf16")] + [("trust", i)])
            outside.append([(k, others(OPT_N, S)) for k in state] + [("groups", others(len(OPT_GROUPS), [i]))])
        for S in OPT_RANGES:  # m and v are elementwise in every form
            targets.append([("m", S), ("v", S)])
            outside.append([(k, others(OPT_N, S)) for k in ("g", "m", "v")])
    else:
        for S in OPT_RANGES:
            o = [(k, others(OPT_N, S)) for k in state]
            if groups:
                used = sorted({int(i >= OPT_CUT) for i in range(OPT_N)[S]})
                o.append(("groups", others(len(OPT_GROUPS), used)))
            targets.append([(k, S) for k in state if k != "g"] + [("p_bf16", S)])
            outside.append(o)
    entry = f"vit_{kind}_step" + ("_groups" if groups else "") + ("_dyn" if dyn else "")
    add(f"{entry} n={OPT_N}" + (" bound record at step 1" if dyn else ""), entry, make, run, targets, outside, ref=ref,
        tol={"p": 1e-6, "m": 1e-6, "v": 1e-6})


for kind in ("adamw", "adam_l2", "sgd", "lamb"):
    opt_case(kind)
    opt_case(kind, groups=True)
    opt_case(kind, groups=True, dyn=True)


# =================================================================================================== elementwise
EL_N = 1003
EL_RANGES = (sl(0, 1), sl(333, 350), sl(EL_N - 3, EL_N), sl(EL_N - 6, EL_N - 1))


def elementwise_case(cid, entry, make, run, ins, outs, ref, tol, n=EL_N, ranges=EL_RANGES):
    """Element i of every output depends on element i of every input of `ins` (flat tensors of n elements)."""
    targets = [[(k, S) for k in outs] for S in ranges]
    outside = [[(k, others(n, S)) for k in ins] for S in ranges]
    add(cid, entry, make, run, targets, outside, ref=ref, tol=tol)


def sam_cases():
    rho = 0.05

    def make(dev):
        g = randn((EL_N,), dev, 12, 0.1)
        return {"p": randn((EL_N,), dev, 11), "g": g, "sq": (g.double() ** 2).sum().float().reshape(1)}

    for adaptive in (False, True):
        def run(d, adaptive=adaptive):
            import vit_amd.functional as vf

            dev = d["p"].device
            backup, pb = E(dev, EL_N), E(dev, EL_N, dt=BF16)
            vf.sam_ascend(d["p"], d["g"], backup, pb, rho, d["sq"], adaptive=adaptive)
            return {"p": d["p"], "backup": backup, "p_bf16": pb}

        def ref(d, adaptive=adaptive):
            p, g = d["p"].double(), d["g"].double()
            s = rho / (math.sqrt(float(d["sq"].double())) + 1e-12)
            return {"p": p + (p * p if adaptive else 1.0) * g * s, "backup": p}

        elementwise_case(f"vit_sam_ascend n={EL_N}" + (" adaptive" if adaptive else ""), "vit_sam_ascend", make, run, ("p", "g"),
                         ("p", "backup", "p_bf16"), ref, {"p": 1e-6, "backup": 0})

    def run_d(d):
        import vit_amd.functional as vf

        pb = E(d["p"].device, EL_N, dt=BF16)
        vf.sam_descend(d["p"], d["g"], pb)  # `g` stands for the backup
        return {"p": d["p"], "p_bf16": pb}

    elementwise_case(f"vit_sam_descend n={EL_N}", "vit_sam_descend", make, run_d, ("p", "g"), ("p", "p_bf16"),
                     lambda d: {"p": d["g"].double(), "p_bf16": d["g"].to(BF16).double()}, {"p": 0, "p_bf16": 0})


sam_cases()


def ema_cases():
    def make(dev):
        return {"p": randn((EL_N,), dev, 1), "ema": randn((EL_N,), dev, 2)}

    def run_u(d):
        import vit_amd.functional as vf

        vf.ema_update(d["ema"], d["p"], 0.01)
        return {"ema": d["ema"]}

    def run_s(d):
        import vit_amd.functional as vf

        pb = E(d["p"].device, EL_N, dt=BF16)
        vf.ema_swap(d["p"], d["ema"], pb)
        return {"p": d["p"], "ema": d["ema"], "p_bf16": pb}

    elementwise_case(f"vit_ema_update n={EL_N}", "vit_ema_update", make, run_u, ("p", "ema"), ("ema",),
                     lambda d: {"ema": d["ema"].double() + 0.01 * (d["p"].double() - d["ema"].double())}, {"ema": 1e-6})
    elementwise_case(f"vit_ema_swap n={EL_N}", "vit_ema_swap", make, run_s, ("p", "ema"), ("p", "ema", "p_bf16"),
                     lambda d: {"p": d["ema"].double(), "ema": d["p"].double(), "p_bf16": d["ema"].to(BF16).double()},
                     {"p": 0, "ema": 0, "p_bf16": 0})


ema_cases()


def cast_cases():
    def run_a(d):
        import vit_amd.functional as vf

        return {"out": vf.cast_f32_bf16(d["src"])}

    def run_b(d):
        import vit_amd.functional as vf

        return {"out": vf.cast_bf16_f32(d["src"], E(d["src"].device, EL_N), 0.5)}

    elementwise_case(f"vit_cast_f32_bf16 n={EL_N}", "vit_cast_f32_bf16", lambda dev: {"src": randn((EL_N,), dev, 51)}, run_a, ("src",), ("out",),
                     lambda d: {"out": d["src"].to(BF16).double()}, {"out": 0})
    elementwise_case(f"vit_cast_bf16_f32 n={EL_N} scale=0.5", "vit_cast_bf16_f32", lambda dev: {"src": bf(randn((EL_N,), dev, 51))}, run_b,
                     ("src",), ("out",), lambda d: {"out": d["src"].double() * 0.5}, {"out": 0})


cast_cases()


def add_noise_case():
    """n % 4 == 0 is the entry point's contract; only the distribution of the noise is contractual, so the reference is the
    level-0 identity and the noisy call is judged by the rounds alone (the normal of element i is keyed by (seed, i))."""
    n = 1004
    rng = (sl(0, 1), sl(333, 350), sl(n - 3, n), sl(n - 6, n - 1))

    def make(dev):
        return {"flux": randn((n,), dev, 100), "err": rand((n,), dev, 101) * 0.2 + 0.05}

    for level in (0.0, 0.5):
        def run(d, level=level):
            import vit_amd.functional as vf

            return {"out": vf.add_noise(d["flux"], d["err"], level, seed=1234)}

        elementwise_case(f"vit_add_noise n={n} level={level}", "vit_add_noise", make, run, ("flux", "err"), ("out",),
                         (lambda d: {"out": d["flux"].double()}) if level == 0.0 else None, {"out": 0}, n=n, ranges=rng)


add_noise_case()


def dropout_bwd_cast_case(rows, cols, odt, drop):
    def make(dev):
        return {"dx": randn((rows, cols), dev, 50)}

    def run(d):
        import vit_amd.functional as vf

        return {"out": vf.dropout_bwd_cast(d["dx"], drop, out_dtype=odt)}

    def ref(d):
        return {"out": (d["dx"] * drop_mult(drop, rows, cols, d["dx"].device)).to(odt).double()}

    targets, outside = [], []
    for R in row_picks(rows):
        for Cs in (ALL, sl(cols - 3, cols), sl(1, 6)):
            targets.append(("out", (R, Cs)))
            o = [("dx", others(rows, R))]
            if Cs != ALL:
                o.append(("dx", (R, others(cols, Cs))))
            outside.append(o)
    add(f"vit_dropout_bwd_cast ({rows}, {cols}) {dn(odt)} p={drop[0]}", "vit_dropout_bwd_cast", make, run, targets, outside, ref=ref,
        tol={"out": 0})


for rows, cols in ((37, 36), (77, 1028)):
    for odt in (BF16, F32):
        dropout_bwd_cast_case(rows, cols, odt, (0.1, 7, 2))
dropout_bwd_cast_case(37, 36, BF16, (0.0, 0, 0))


def layer_scale_case(which, odt=F32):
    """One entry of the table per matrix: the outputs of entry e depend on the inputs of entry e (row r of them on row r)."""
    shapes = ((5, 36), (64, 32), (7, 12))
    names = ("W", "b", "lam") if which == "fold" else ("W", "b", "lam", "dW_raw", "db_raw")

    def make(dev):
        g = torch.Generator().manual_seed(11)
        d = {}
        for e, (r, c) in enumerate(shapes):
            d[f"lam{e}"] = torch.exp(torch.empty(r).uniform_(float(np.log(1e-3)), float(np.log(2.0)), generator=g)).to(dev)
            d[f"W{e}"], d[f"b{e}"] = torch.randn(r, c, generator=g).to(dev), torch.randn(r, generator=g).to(dev)
            if which == "grad":
                d[f"dW_raw{e}"], d[f"db_raw{e}"] = torch.randn(r, c, generator=g).to(dev), torch.randn(r, generator=g).to(dev)
        return d

    def run(d):
        import vit_amd.functional as vf

        dev = d["W0"].device
        ents, out = [], {}
        for e, (r, c) in enumerate(shapes):
            ent = {k: d[f"{k}{e}"] for k in names}
            if which == "fold":
                ent.update(Wf=E(dev, r, c, dt=odt), bf=E(dev, r))
                out[f"Wf{e}"], out[f"bf{e}"] = ent["Wf"], ent["bf"]
            else:
                ent.update(dW=E(dev, r, c), db=E(dev, r), dlam=E(dev, r))
                out[f"dW{e}"], out[f"db{e}"], out[f"dlam{e}"] = ent["dW"], ent["db"], ent["dlam"]
            ents.append(ent)
        tab = vf.layer_scale_table(ents, dev)
        if which == "fold":
            vf.layer_scale_fold(tab, odt)
        else:
            vf.layer_scale_grad(tab, False)
        return out

    def ref(d):
        out = {}
        for e in range(len(shapes)):
            lam, W, b = d[f"lam{e}"], d[f"W{e}"], d[f"b{e}"]
            if which == "fold":  # one f32 product each: exact restatements
                out[f"Wf{e}"], out[f"bf{e}"] = (lam[:, None] * W).to(odt).double(), (lam * b).double()
            else:
                out[f"dW{e}"], out[f"db{e}"] = (lam[:, None] * d[f"dW_raw{e}"]).double(), (lam * d[f"db_raw{e}"]).double()
                out[f"dlam{e}"] = (d[f"dW_raw{e}"].double() * W.double()).sum(1) + d[f"db_raw{e}"].double() * b.double()
        return out

    outs = ("Wf", "bf") if which == "fold" else ("dW", "db", "dlam")
    targets, outside = [], []
    for e, (r, c) in enumerate(shapes):
        foreign = [(f"{k}{o}", ALL) for o in range(len(shapes)) if o != e for k in names]
        targets.append([(f"{k}{e}", ALL) for k in outs])
        outside.append(foreign)
        for S in (sl(0, 1), sl(r - 1, r), sl(r // 2, r // 2 + 2)):
            targets.append([(f"{k}{e}", S) for k in outs])
            outside.append(foreign + [(f"{k}{e}", others(r, S)) for k in names])
    tol = {f"{k}{e}": (0 if k != "dlam" else 1e-5) for k in outs for e in range(len(shapes))}
    add(f"vit_layer_scale_{which} 5x36 + 64x32 + 7x12" + (f" {dn(odt)}" if which == "fold" else ""), f"vit_layer_scale_{which}", make, run,
        targets, outside, ref=ref, tol=tol)


layer_scale_case("fold", BF16)
layer_scale_case("fold", F32)
layer_scale_case("grad")


# =================================================================================================== column sums, covariance
def colsum_case(rows, cols, dt, pad):
    def make(dev):
        return {"a": randn((rows, cols + pad), dev, 50).to(dt)}

    def run(d):
        import vit_amd.functional as vf

        return {"out": vf.colsum(d["a"][:, :cols])}

    picks = col_picks(cols)
    add(f"vit_colsum ({rows}, {cols}) {dn(dt)} lda=cols+{pad}", "vit_colsum", make, run, [("out", S) for S in picks],
        [[("a", (ALL, others(cols + pad, S)))] for S in picks], ref=lambda d: {"out": d["a"][:, :cols].double().sum(0)}, tol={"out": 1e-5})


for dt in (F32, BF16):
    colsum_case(1234, 768, dt, 4)
    colsum_case(37, 36, dt, 0)
colsum_case(5000, 64, F32, 8)


def cov_cases():
    """include/vit_amd_cov.h: acc[i, j] (upper 128 x 128 tiles) depends on columns i and j of x and on mean[i], mean[j];
    vit_cov_finish's cov[i, j] on acc[min, max]; vit_cov_mean_finish is elementwise."""
    n, L = 300, 200

    def make(dev):
        x = randn((n, L + 8), dev, 7) + 3.0
        return {"x": x, "mean": x[:, :L].double().mean(0).float(), "acc0": randn((L, L), dev, 8)}

    def run_acc(d):
        import vit_amd.functional as vf

        acc = torch.zeros((L, L), device=d["x"].device)
        vf.cov_accumulate(d["x"], d["mean"], acc, cols=L)
        return {"acc": acc}

    def ref_acc(d):
        c = d["x"][:, :L].double() - d["mean"].double()
        return {"acc": torch.triu(c.t() @ c)}

    blocks = ((sl(0, 2), sl(0, 2)), (sl(5, 8), sl(190, 200)), (sl(126, 130), sl(126, 130)), (sl(100, 103), sl(128, 140)), (sl(198, 200), sl(198, 200)))
    targets, outside = [], []
    for I, J in blocks:  # I <= J: inside the upper triangle, across the 128-column tile boundary
        used = sorted(set(range(L)[I]) | set(range(L)[J]))
        targets.append(("acc", (torch.tensor([i for i in range(L)[I] for j in range(L)[J] if i <= j]),
                                torch.tensor([j for i in range(L)[I] for j in range(L)[J] if i <= j]))))
        outside.append([("x", (ALL, others(L + 8, used))), ("mean", others(L, used))])
    add("vit_cov_accumulate (300, 200) ld=208", "vit_cov_accumulate", make, run_acc, targets, outside, ref=ref_acc, tol={"acc": 1e-5})

    def run_fin(d):
        import vit_amd.functional as vf

        return {"cov": vf.cov_finish(d["acc0"], n)}

    def ref_fin(d):
        u = torch.triu(d["acc0"].double()) / (n - 1)
        return {"cov": u + torch.triu(u, 1).t()}

    targets, outside = [], []
    for I, J in blocks:
        keep = torch.zeros(L, L, dtype=torch.bool)
        keep[I, J] = True
        keep = keep | keep.t()
        targets.append([("cov", (I, J)), ("cov", (J, I))])
        outside.append([("acc0", ~torch.triu(keep))])  # the lower triangle of acc is never read
    add("vit_cov_finish 200 x 200", "vit_cov_finish", make, run_fin, targets, outside, ref=ref_fin, tol={"cov": 1e-6})

    def run_mean(d):
        import vit_amd.functional as vf

        return {"mean": vf.cov_mean_finish(d["mean"], n)}

    picks = (sl(0, 1), sl(99, 103), sl(L - 3, L))
    add("vit_cov_mean_finish 200", "vit_cov_mean_finish", make, run_mean, [("mean", S) for S in picks],
        [[("mean", others(L, S))] for S in picks], ref=lambda d: {"mean": d["mean"].double() / n}, tol={"mean": 1e-6})


cov_cases()


@pytest.mark.gpu
def test_patch_select_is_per_sample(dev):
    """vit_patch_select has no tensor input, so it has no footprint case; what can be pinned is that sample b's idx and slot rows
    do not depend on how many samples follow it: the call with B + 3 samples gives the call with B samples in its first B rows."""
    import vit_amd.functional as vf

    N, K, seed, site = 13, 3, 0x1234567, 49

    def select(B):
        idx, slot = torch.zeros((B, K), dtype=torch.int32, device=dev), torch.zeros((B, N), dtype=torch.int32, device=dev)
        return vf.patch_select(B, N, K, seed, site, idx, slot)

    (i5, s5), (i8, s8) = select(5), select(8)
    assert torch.equal(i8[:5], i5) and torch.equal(s8[:5], s5)
    assert not torch.equal(i8[5:8], i5[:3])  # and the samples do differ


# ===================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_footprint(dev, case):
    footprint(dev, case)
