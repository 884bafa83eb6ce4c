"""Fused Muon on the MI355X, from the kernels of vit_amd/csrc/muon.hip up to the trainer.

The yardsticks (tests/_muon_ref.py):
  * the grouped product alone against an f64 product of the same bf16 operands, per element
        |err| <= 2^-8 |ref| + K 2^-23 (|A| |B|)_ij
    -- one bf16 rounding of the result plus the f32 accumulation; no measured tolerance;
  * the orthogonalisation against the unrounded f64 iteration: rel(O_hip, O_f64) <= 1.5 * e_ref, e_ref being torch.optim.Muon's
    own distance from that iteration on the same input, computed here (the margin: tests/_muon_ref.py);
  * momentum_buffer against torch's within 4 f32 ulps at the buffer's magnitude per step taken (the lerp's three roundings);
  * everything on the AdamW side, the captured step and a resumed run: bit for bit.

POISON_CASES / FOOTPRINT_CASES cover every entry point of include/vit_amd_muon.h (tests/test_muon_cpu.py checks that they do)."""
import functools
import warnings
from collections import namedtuple

import pytest
import torch

import _muon_ref as mr
from _footprint import Case as FCase
from _footprint import footprint
from _poison import poisoned

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PCase = namedtuple("PCase", "id entries fn")
POISON_CASES, FOOTPRINT_CASES = [], []


def padd(cid, entries, fn):
    POISON_CASES.append(PCase(cid, (entries,) if isinstance(entries, str) else tuple(entries), fn))


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ================================================================================================ 1. the grouped product alone
MIXED = [(32, 32, 32), (32, 32, 128), (32, 128, 32), (96, 96, 32), (48, 80, 48), (192, 192, 768)]  # (m, n, K)


def _operands(dev, shapes, b_trans, beta, seed, lead_pad=0):
    """Per problem (A, B, R, C, alpha, beta) on `dev`; `lead_pad`: extra columns in every leading dimension (views of wider
    buffers, so edge tiles sit beside memory that must stay untouched)."""
    out = []
    for i, (m, n, k) in enumerate(shapes):
        def mat(r, c, s):
            full = randn((r, c + lead_pad), seed + 10 * i + s).to(dev).to(BF16)
            return full[:, :c]
        A, B = mat(m, k, 1), mat(n, k, 2) if b_trans else mat(k, n, 2)
        R = mat(m, n, 3) if beta != 0 else None
        C = torch.zeros(m, n + lead_pad, dtype=BF16, device=dev)[:, :n]
        out.append((A, B, R, C, 1.0 if beta != 0 else (1.0, -0.5, 2.0315)[i % 3], beta))
    return out


def _product_ref(prob, b_trans):
    A, B, R, _, alpha, beta = prob
    A, B = A.double().cpu(), B.double().cpu()
    Bm = B.T if b_trans else B
    ref = alpha * (A @ Bm) + (beta * R.double().cpu() if R is not None else 0.0)
    mag = A.abs() @ Bm.abs()
    return ref, mag


def _check_products(probs, b_trans, say):
    worst = 0.0
    for i, p in enumerate(probs):
        ref, mag = _product_ref(p, b_trans)
        K = p[0].shape[1]
        err = (p[3].double().cpu() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
        frac = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, frac)
        say(f"  problem {i} (m, n, K) = {tuple(p[3].shape) + (K,)}: max |err| / bound = {frac:.3f}")
        assert bool((err <= bound).all()), (i, frac)
    return worst


@pytest.mark.parametrize("beta", [0.0, 3.4445], ids=["beta0", "beta"])
@pytest.mark.parametrize("b_trans", [True, False], ids=["ABt", "AB"])
def test_grouped_product_mixed_shapes_within_the_arithmetic_bound(dev, b_trans, beta):
    import vit_amd.functional as vf

    probs = _operands(dev, MIXED, b_trans, beta, seed=100 + 7 * b_trans)
    table = vf.muon_problem_table(probs, b_trans, dev)
    assert table.n_problems == 6 and table.n_tiles == 1 + 1 + 2 + 4 + 2 + 9
    vf.muon_gemm_grouped(table)
    torch.cuda.synchronize()
    print(f"[muon grouped product {'A B^T' if b_trans else 'A B'} beta {beta}]")
    _check_products(probs, b_trans, print)


@pytest.mark.parametrize("b_trans", [True, False], ids=["ABt", "AB"])
def test_grouped_product_one_problem_table_and_padded_leading_dimensions(dev, b_trans):
    import vit_amd.functional as vf

    for shape, pad in (((48, 80, 48), 0), ((48, 80, 48), 24), ((192, 192, 768), 8)):
        probs = _operands(dev, [shape], b_trans, 2.0, seed=300 + pad, lead_pad=pad)
        table = vf.muon_problem_table(probs, b_trans, dev)
        assert table.n_problems == 1
        vf.muon_gemm_grouped(table)
        torch.cuda.synchronize()
        _check_products(probs, b_trans, lambda s: None)
        if pad:
            C = probs[0][3]
            assert not bool(C._base[:, C.shape[1]:].float().abs().sum()) if C._base is not None else True


def test_an_asymmetric_operand_pins_the_output_orientation(dev):
    """A = I with an asymmetric B: a swapped row / column map in the epilogue, or B read transposed, shows as B^T."""
    import vit_amd.functional as vf

    n = 48
    eye = torch.eye(n, dtype=BF16, device=dev)
    B = (torch.arange(n * n, dtype=F32, device=dev).view(n, n) % 17 - 8 + torch.arange(n, device=dev).view(n, 1)).to(BF16)
    for b_trans in (True, False):
        C = torch.zeros(n, n, dtype=BF16, device=dev)
        vf.muon_gemm_grouped(vf.muon_problem_table([(eye, B, None, C, 1.0, 0.0)], b_trans, dev))
        assert torch.equal(C, B.T.contiguous() if b_trans else B) and not torch.equal(B, B.T.contiguous())


def _poison_product(dev, b_trans, beta):
    """Outputs pre-filled: every element of every C_i is written, the columns beside C_i (the leading dimension's pad) are not."""
    import vit_amd.functional as vf

    probs = _operands(dev, MIXED, b_trans, beta, seed=500 + b_trans, lead_pad=16)
    table = vf.muon_problem_table(probs, b_trans, dev)
    outs = [p[3] for p in probs]
    pads = [p[3]._base[:, p[3].shape[1]:] for p in probs]
    poisoned(dev, lambda: vf.muon_gemm_grouped(table), outs, pads)
    _check_products(probs, b_trans, lambda s: None)


for _bt in (True, False):
    for _beta in (0.0, -4.775):
        padd(f"muon_gemm_grouped-{'ABt' if _bt else 'AB'}-beta{_beta:g}", "vit_muon_gemm_grouped",
             functools.partial(_poison_product, b_trans=_bt, beta=_beta))


def _fp_product_case(b_trans):
    import vit_amd.functional as vf

    shapes = [(32, 32, 32), (48, 80, 48), (96, 96, 32)]

    def make(dev):
        d = {}
        for i, (m, n, k) in enumerate(shapes):
            d[f"A{i}"] = randn((m, k), 700 + i).to(dev).to(BF16)
            d[f"B{i}"] = randn((n, k) if b_trans else (k, n), 710 + i).to(dev).to(BF16)
            d[f"R{i}"] = randn((m, n), 720 + i).to(dev).to(BF16)
        return d

    def run(d):
        dev = d["A0"].device
        Cs = [torch.zeros(m, n, dtype=BF16, device=dev) for m, n, _ in shapes]
        vf.muon_gemm_grouped(vf.muon_problem_table([(d[f"A{i}"], d[f"B{i}"], d[f"R{i}"], Cs[i], 1.0, 0.5) for i in range(3)],
                                                   b_trans, dev))
        return {f"C{i}": Cs[i] for i in range(3)}

    def ref(d):
        return {f"C{i}": d[f"A{i}"].double() @ (d[f"B{i}"].double().T if b_trans else d[f"B{i}"].double()) + 0.5 * d[f"R{i}"].double()
                for i in range(3)}

    everything = slice(None)
    outside = [[(f"{x}{j}", everything) for j in range(3) if j != i for x in "ABR"] for i in range(3)]
    # rel over a whole C of one bf16 rounding per element is below 2^-8; the products' own test is the per-element bound above
    return FCase(f"muon_gemm_grouped-{'ABt' if b_trans else 'AB'}", "vit_muon_gemm_grouped", make, run,
                 [(f"C{i}", everything) for i in range(3)], outside, ref=ref, tol={f"C{i}": 2.0 ** -8 for i in range(3)})


FOOTPRINT_CASES += [_fp_product_case(True), _fp_product_case(False)]


# ================================================================================================ 2. the orthogonalisation
ORTHO = [(32, 32), (32, 128), (128, 32), (96, 32), (192, 768)]


def _ortho_entries(shapes, gap=24):
    """(off, xoff, rows, cols, group, ratio) with a gap of `gap` elements behind every matrix in the flat buffer."""
    ents, off, xoff = [], 8, 0
    for i, (r, c) in enumerate(shapes):
        ents.append((off, xoff, r, c, i % 2, 1.0))
        off += r * c + gap
        xoff += r * c
    return ents, off, xoff


class Pipeline:
    """The streaming passes and the plan over one table, on buffers of its own."""

    def __init__(self, dev, shapes, ratios=None):
        import vit_amd.functional as vf

        ents, self.n_flat, self.n_x = _ortho_entries(shapes)
        if ratios is not None:
            ents = [e[:5] + (r,) for e, r in zip(ents, ratios)]
        self.tables = vf.muon_mat_table(ents, dev, total=self.n_flat, compact_total=self.n_x)
        self.buf = torch.zeros(self.n_x, dtype=F32, device=dev)
        self.x = [torch.zeros(self.n_x, dtype=BF16, device=dev) for _ in range(2)]
        self.plan = vf.MuonPlan(self.tables, mr.COEFFS, dev, x=self.x)
        self.part = torch.zeros(self.tables.n_tiles, dtype=F64, device=dev)
        self.inv = torch.zeros(self.tables.n_mats, dtype=F32, device=dev)
        self.norms = torch.zeros(self.tables.n_mats, dtype=F32, device=dev)
        self.dev, self.vf = dev, vf

    def flat(self, mats, fill=0.0):
        g = torch.full((self.n_flat,), fill, dtype=F32, device=self.dev)
        for (off, _, r, c, _, _), m in zip(self.tables.entries, mats):
            g[off:off + r * c] = m.reshape(-1).to(self.dev)
        return g

    def orthogonalise(self, g, momentum=0.0, nesterov=False, ns_steps=5, sqnorm=None, max_norm=0.0):
        vf = self.vf
        vf.muon_momentum(g, self.buf, self.x[1], self.tables, self.part, momentum=momentum, nesterov=nesterov, sqnorm=sqnorm,
                         max_norm=max_norm)
        vf.muon_norms(self.tables, self.part, self.inv, self.norms)
        vf.muon_normalize(self.x[1], self.x[0], self.tables, self.inv)
        return self.plan.iterate(ns_steps)

    def result(self, out):
        """O per matrix, transposed back to [rows, cols], on the host."""
        res = []
        for _, xoff, r, c, _, _ in self.tables.entries:
            X = out[xoff:xoff + r * c].view(min(r, c), max(r, c))
            res.append((X if r <= c else X.T).double().cpu())
        return res


_YARD = {}


def yardstick(key, u):
    """(e_ref, O_f64) of the input `u`, computed once per key."""
    if key not in _YARD:
        _YARD[key] = mr.e_ref(u)
    return _YARD[key]


def test_orthogonalisation_within_the_margin_of_torchs_own_error(dev):
    us = [randn(s, 900 + i) for i, s in enumerate(ORTHO)]
    pipe = Pipeline(dev, ORTHO)
    out = pipe.orthogonalise(pipe.flat(us))  # momentum 0: buf = g, u = buf
    got = pipe.result(out)
    norms = pipe.norms.cpu()
    worst = 0.0
    for i, (u, O) in enumerate(zip(us, got)):
        e, exact = yardstick(("ortho", i), u)
        d = mr.rel(O, exact)
        worst = max(worst, d / e)
        print(f"[muon ortho {ORTHO[i]}] e_ref {e:.3e}, hip {d:.3e}, ratio {d / e:.3f} (allowed {mr.MARGIN})")
        assert d <= mr.MARGIN * e, (ORTHO[i], d, e)
        want = float(u.bfloat16().double().norm())
        assert abs(float(norms[i]) - want) <= 2.0 ** -22 * want
        assert torch.equal(pipe.buf[pipe.tables.entries[i][1]:][:u.numel()].cpu(), u.reshape(-1))  # lerp with weight 1
    print(f"[muon ortho] worst ratio {worst:.3f}")


def test_ill_conditioned_inputs_stay_finite_and_bounded(dev):
    gen = torch.Generator().manual_seed(77)
    us = [mr.low_rank(r, c, 4, 0.05, gen) for r, c in ORTHO]
    pipe = Pipeline(dev, ORTHO)
    for O in pipe.result(pipe.orthogonalise(pipe.flat(us))):
        assert bool(torch.isfinite(O).all())
        sv = torch.linalg.svdvals(O)
        assert 0.0 <= float(sv.min()) and float(sv.max()) <= 1.3, float(sv.max())


def test_an_all_zero_gradient_gives_a_zero_update_and_w_only_decays(dev):
    import vit_amd.functional as vf

    shapes = [(32, 32), (128, 32)]
    pipe = Pipeline(dev, shapes, ratios=[1.0, 2.0])
    g = pipe.flat([torch.zeros(s) for s in shapes])
    out = pipe.orthogonalise(g, momentum=0.95, nesterov=True)
    assert not bool(out.float().abs().sum()) and not bool(pipe.norms.abs().sum()) and bool(torch.isfinite(pipe.inv).all())
    W0 = [randn(s, 40 + i) for i, s in enumerate(shapes)]
    p = pipe.flat(W0, fill=3.0)
    groups = torch.tensor([[1e-2, 0.5, 0, 0], [2e-2, 0.25, 0, 0]], dtype=F32, device=dev)
    shadow = torch.zeros(pipe.n_flat, dtype=BF16, device=dev)
    vf.muon_apply(p, shadow, out, pipe.tables, groups)
    for (off, _, r, c, gi, _), w in zip(pipe.tables.entries, W0):
        decay = torch.tensor(1.0, dtype=F32) - groups[gi, 0].cpu() * groups[gi, 1].cpu()
        want = w.reshape(-1) * decay
        assert torch.equal(p[off:off + r * c].cpu(), want) and torch.equal(shadow[off:off + r * c].cpu(), want.bfloat16())


# ---- poison and footprint of the streaming passes
STREAM_SHAPES = [(32, 32), (128, 32), (96, 48), (32, 160)]  # tall and wide, 16-multiples that are no multiple of the 32-tile
STREAM_TILES = [slice(0, 1), slice(1, 2), slice(2, 4), slice(4, 6)]  # their streaming tiles: one, one full, two (the last short) twice


def _stream_state(dev, seed=60):
    pipe = Pipeline(dev, STREAM_SHAPES, ratios=[1.0, 0.5, 2.0, 1.5])
    g = pipe.flat([randn(s, seed + i) for i, s in enumerate(STREAM_SHAPES)], fill=float("nan"))  # the gaps: never read
    return pipe, g


def _poison_momentum(dev):
    import vit_amd.functional as vf

    pipe, g = _stream_state(dev)
    buf0 = randn((pipe.n_x,), 61, 0.1).to(dev)

    def run():
        pipe.buf.copy_(buf0)
        vf.muon_momentum(g, pipe.buf, pipe.x[1], pipe.tables, pipe.part, momentum=0.95, nesterov=True)

    (u,) = poisoned(dev, run, [pipe.x[1]])
    parts = []
    for fill in (float("nan"), 3.0e38):  # the f64 partials by hand: tests/_poison.py fills 2- and 4-byte elements
        pipe.part.fill_(fill)
        run()
        parts.append(pipe.part.clone())
    part = parts[0]
    assert bool(torch.isfinite(part).all()) and torch.equal(parts[0], parts[1])
    gd, bd = torch.cat([g[o:o + r * c] for o, _, r, c, _, _ in pipe.tables.entries]).double(), buf0.double()
    b1, want = mr.momentum_update(bd, gd)
    assert float((pipe.buf.double() - b1).abs().max()) <= 4 * 2.0 ** -24 * float(b1.abs().max())
    assert float((u.double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    sums = torch.stack([u[x:x + r * c].double().pow(2).sum() for _, x, r, c, _, _ in pipe.tables.entries])
    got = torch.stack([part[t].sum() for t in STREAM_TILES])
    assert part.numel() == 6 and float((got - sums).abs().max()) <= 1e-12 * float(sums.max())


def _poison_norms(dev):
    import vit_amd.functional as vf

    pipe, _ = _stream_state(dev)
    pipe.part.copy_(torch.tensor([4.0, 0.0, 1.25e-20, 1.0e-20, 5.0, 4.0], dtype=F64))
    inv, norms = poisoned(dev, lambda: vf.muon_norms(pipe.tables, pipe.part, pipe.inv, pipe.norms), [pipe.inv, pipe.norms])
    assert norms.tolist() == [2.0, 0.0, float(torch.tensor(1.5e-10, dtype=F32)), 3.0]
    assert inv.tolist() == [0.5, float(torch.tensor(1e7, dtype=F32)), float(torch.tensor(1e7, dtype=F32)),
                            float(torch.tensor(1.0 / 3.0, dtype=F32))]


def _wide(u, entries):
    """The wide image [m, n] of every matrix of a compact [rows, cols] buffer."""
    out = torch.empty_like(u)
    for _, x, r, c, _, _ in entries:
        m = u[x:x + r * c].view(r, c)
        out[x:x + r * c] = (m if r <= c else m.T).reshape(-1)
    return out


def _poison_normalize(dev):
    import vit_amd.functional as vf

    pipe, _ = _stream_state(dev)
    u = randn((pipe.n_x,), 62).to(dev).to(BF16)
    pipe.inv.copy_(torch.tensor([0.5, 0.25, 2.0, 1.0 / 3.0]))
    (x,) = poisoned(dev, lambda: vf.muon_normalize(u, pipe.x[0], pipe.tables, pipe.inv), [pipe.x[0]])
    scale = torch.cat([torch.full((r * c,), float(pipe.inv[i]), device=dev) for i, (_, _, r, c, _, _) in enumerate(pipe.tables.entries)])
    assert torch.equal(x, _wide((u.float() * scale).to(BF16), pipe.tables.entries))


def _poison_apply(dev):
    """In place on p by contract, so p is restored before every run; the shadow is the poisoned output, the gaps of p and of the
    shadow are pads."""
    import vit_amd.functional as vf

    pipe, _ = _stream_state(dev)
    ents = pipe.tables.entries
    p0 = pipe.flat([randn(s, 63 + i) for i, s in enumerate(STREAM_SHAPES)], fill=7.0)
    o = randn((pipe.n_x,), 64).to(dev).to(BF16)
    groups = torch.tensor([[1e-2, 0.5, 0, 0], [2e-2, 0.0, 0, 0]], dtype=F32, device=dev)
    p, shadow = p0.clone(), torch.zeros(pipe.n_flat, dtype=BF16, device=dev)
    inside = torch.zeros(pipe.n_flat, dtype=torch.bool, device=dev)
    for off, _, r, c, _, _ in ents:
        inside[off:off + r * c] = True
    bounds = [0] + [b for off, _, r, c, _, _ in ents for b in (off, off + r * c)] + [pipe.n_flat]
    gaps = [shadow[a:b] for a, b in zip(bounds[::2], bounds[1::2]) if b > a]

    def run():
        p.copy_(p0)
        vf.muon_apply(p, shadow, o, pipe.tables, groups)

    poisoned(dev, run, [shadow[off:off + r * c] for off, _, r, c, _, _ in ents], gaps)
    assert torch.equal(p[~inside], p0[~inside]) and torch.equal(shadow[inside], p[inside].to(BF16))
    for off, x, r, c, gi, ratio in ents:
        lr, wd = float(groups[gi, 0]), float(groups[gi, 1])
        O = o[x:x + r * c].view(min(r, c), max(r, c))
        O = (O if r <= c else O.T).double().reshape(-1)
        want = p0[off:off + r * c].double() * (1 - lr * wd) - lr * ratio * O
        assert float((p[off:off + r * c].double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())


padd("muon_momentum", "vit_muon_momentum", _poison_momentum)
padd("muon_norms", "vit_muon_norms", _poison_norms)
padd("muon_normalize", "vit_muon_normalize", _poison_normalize)
padd("muon_apply", "vit_muon_apply", _poison_apply)


def _fp_stream_cases():
    import vit_amd.functional as vf

    ents, n_flat, n_x = _ortho_entries(STREAM_SHAPES)
    ents = [e[:5] + (r,) for e, r in zip(ents, [1.0, 0.5, 2.0, 1.5])]
    fl = [slice(off, off + r * c) for off, _, r, c, _, _ in ents]
    cp = [slice(x, x + r * c) for _, x, r, c, _, _ in ents]
    one = [slice(i, i + 1) for i in range(4)]
    tab = functools.lru_cache(None)(lambda dev: vf.muon_mat_table(ents, dev, total=n_flat, compact_total=n_x))
    not_i = lambda name, sl, i: [(name, s) for j, s in enumerate(sl) if j != i]

    def flat_of(dev, seed, fill=0.0):
        t = torch.full((n_flat,), fill, dtype=F32, device=dev)
        for s in fl:
            t[s] = randn((s.stop - s.start,), seed + s.start).to(dev)
        return t

    def run_mom(d):
        dev = d["g"].device
        u, part = torch.zeros(n_x, dtype=BF16, device=dev), torch.zeros(6, dtype=F64, device=dev)
        vf.muon_momentum(d["g"], d["buf"], u, tab(dev), part, momentum=0.9, nesterov=True)
        return {"buf": d["buf"], "u": u, "part": part.view(torch.int32)}  # the f64 sums as their bits: compared exactly

    def ref_mom(d):
        g = torch.cat([d["g"][s] for s in fl]).double()
        buf, u = mr.momentum_update(d["buf"].double(), g, 0.9, True)
        return {"buf": buf, "u": u}

    gaps = [("g", slice(0, fl[0].start))] + [("g", slice(a.stop, b.start)) for a, b in zip(fl, fl[1:])]
    yield FCase("muon_momentum", "vit_muon_momentum", lambda dev: {"g": flat_of(dev, 800), "buf": randn((n_x,), 801, 0.1).to(dev)},
                run_mom, [[("buf", cp[i]), ("u", cp[i]), ("part", slice(2 * STREAM_TILES[i].start, 2 * STREAM_TILES[i].stop), False)] for i in range(4)],
                [not_i("g", fl, i) + not_i("buf", cp, i) + gaps for i in range(4)], ref=ref_mom, tol={"buf": 1e-6, "u": 2.0 ** -8})

    def run_norms(d):
        dev = d["part"].device  # f32 here (the helpers perturb 2- and 4-byte elements), widened exactly for the kernel
        inv, norms = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
        vf.muon_norms(tab(dev), d["part"].double(), inv, norms)
        return {"inv": inv, "norms": norms}

    yield FCase("muon_norms", "vit_muon_norms", lambda dev: {"part": randn((6,), 802).abs().to(dev) + 0.5}, run_norms,
                [[("inv", one[i], False), ("norms", one[i], False)] for i in range(4)],
                [not_i("part", STREAM_TILES, i) for i in range(4)])

    def run_nrm(d):
        dev = d["u"].device
        x = torch.zeros(n_x, dtype=BF16, device=dev)
        vf.muon_normalize(d["u"], x, tab(dev), d["inv"])
        return {"x": x}

    def ref_nrm(d):
        scale = torch.cat([d["inv"][i].double().expand(s.stop - s.start) for i, s in enumerate(cp)])
        return {"x": _wide(d["u"].double() * scale, ents)}

    yield FCase("muon_normalize", "vit_muon_normalize",
                lambda dev: {"u": randn((n_x,), 803).to(dev).to(BF16), "inv": (randn((4,), 804).abs() + 0.5).to(dev)}, run_nrm,
                [("x", cp[i]) for i in range(4)], [not_i("u", cp, i) + not_i("inv", one, i) for i in range(4)], ref=ref_nrm,
                tol={"x": 2.0 ** -8})

    def run_apply(d):
        dev = d["p"].device
        shadow = torch.zeros(n_flat, dtype=BF16, device=dev)
        vf.muon_apply(d["p"], shadow, d["o"], tab(dev), d["groups"])
        return {"p": d["p"], "shadow": shadow}

    def ref_apply(d):
        p = d["p"].double().clone()
        for off, x, r, c, gi, ratio in ents:
            lr, wd = float(d["groups"][gi, 0]), float(d["groups"][gi, 1])
            O = d["o"][x:x + r * c].view(min(r, c), max(r, c)).double()
            p[off:off + r * c] = p[off:off + r * c] * (1 - lr * wd) - lr * ratio * (O if r <= c else O.T).reshape(-1)
        return {"p": p, "shadow": p}

    def make_apply(dev):
        return {"p": flat_of(dev, 805, fill=7.0), "o": randn((n_x,), 806).to(dev).to(BF16),
                "groups": torch.tensor([[1e-2, 0.5, 0, 0], [2e-2, 0.1, 0, 0]], dtype=F32, device=dev)}

    # matrix i belongs to group i % 2: the other group's row is outside its footprint too, and so is the row's momentum
    yield FCase("muon_apply", "vit_muon_apply", make_apply, run_apply,
                [[("p", fl[i]), ("shadow", fl[i])] for i in range(4)],
                [not_i("p", fl, i) + not_i("o", cp, i) + [("groups", (slice(1 - i % 2, 2 - i % 2), slice(0, 2))),
                                                          ("groups", (slice(None), slice(2, 4)))] for i in range(4)],
                ref=ref_apply, tol={"p": 1e-6, "shadow": 2.0 ** -8})


FOOTPRINT_CASES += list(_fp_stream_cases())


@pytest.mark.parametrize("case", POISON_CASES, ids=[c.id for c in POISON_CASES])
def test_poison(dev, case):
    case.fn(dev)


@pytest.mark.parametrize("case", FOOTPRINT_CASES, ids=[c.id for c in FOOTPRINT_CASES])
def test_footprint(dev, case):
    footprint(dev, case)


# ================================================================================================ 3. the optimizer on the l3 layout
LR, WD, CLIP = 2e-3, 0.05, 0.5


def _l3(dev, precision="32"):
    from test_cls_tail_gpu import build, case

    rc, sd, flux, labels, _, _ = case("l3")
    return build(rc, sd, dev, precision).eval(), flux.to(dev), labels.to(dev)  # eval: no dropout, so a resumed run sees the same g


def _fused(model, cls=None, nesterov=True, **kw):
    from vit_amd.optimizer import FusedAdamW, FusedMuon, build_param_groups

    groups = build_param_groups(model, LR, WD, no_decay=True, layer_decay=0.75)
    if cls is FusedAdamW:
        return FusedAdamW(model, lr=LR, weight_decay=WD, param_groups=groups)
    return FusedMuon(model, lr=LR, weight_decay=WD, nesterov=nesterov, param_groups=groups, **kw)


_SYN = {}


def _synthetic_grads(n_total, steps=3):
    if "g" not in _SYN:
        _SYN["g"] = [randn((n_total,), 2000 + s, 1e-2) for s in range(steps)]
    return _SYN["g"]


def _feed(model, g):
    """The flat gradient buffer <- g; every trainable parameter's .grad is its view, as after a backward."""
    eng = model.engine
    eng._ensure_device_state()
    eng.grads.copy_(g.to(eng.grads.device))
    lay = eng.layout
    for name, p in zip(model._param_names, model._param_list):
        p.grad = eng.g(name) if (lay.entries[name][0] < lay.n_trainable and p.requires_grad) else None


@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "plain"])
def test_optimizer_steps_on_synthetic_gradients(dev, nesterov):
    from vit_amd.optimizer import FusedAdamW

    model, _, _ = _l3(dev)
    twin, _, _ = _l3(dev)
    # one matrix alone, and a layer's query AND key together: the reference's qk-freeze, which in this model is exactly that --
    # requires_grad off on the two projections, so their .grad stays None and no run of the step covers them
    frozen = ["vit.encoder.layer.1.attention.attention.key.weight", "vit.encoder.layer.2.attention.attention.query.weight",
              "vit.encoder.layer.2.attention.attention.key.weight"]
    for m in (model, twin):
        for n in frozen:
            dict(m.named_parameters())[n].requires_grad_(False)
    opt, ada = _fused(model, nesterov=nesterov), _fused(twin, FusedAdamW)
    opt.set_grad_clip(CLIP)
    ada.set_grad_clip(CLIP)
    lay = model.engine.layout
    gs = _synthetic_grads(lay.n_total)
    mats, rest = opt.muon_split()
    assert len(mats) == 18 and all(n in mats for n in frozen)
    SENTINEL = 123.5  # in the frozen matrices' slices of the momentum buffer: "never written" is not "written with zeros"
    opt._ensure_state()
    for name, _, _, xoff, rows, cols in opt._matrices():
        if name in frozen:
            opt._buf[xoff:xoff + rows * cols] = SENTINEL
    by_name = dict(model.named_parameters())
    W0 = {n: by_name[n].detach().cpu().clone() for n in mats}
    tbuf = {n: torch.zeros_like(W0[n]) for n in mats}
    tparam = {n: torch.nn.Parameter(W0[n].clone()) for n in mats}
    lr_of = {n: opt._group_for(by_name[n])["lr"] for n in mats}
    wd_of = {n: opt._group_for(by_name[n])["weight_decay"] for n in mats}
    topt = {n: torch.optim.Muon([tparam[n]], lr=lr_of[n], weight_decay=wd_of[n], momentum=0.95, nesterov=nesterov,
                                adjust_lr_fn="match_rms_adamw") for n in mats if n not in frozen}
    assert len(set(lr_of.values())) == 3 and set(wd_of.values()) == {WD}
    worst = 0.0
    for s in range(3):
        _feed(model, gs[s])
        _feed(twin, gs[s])
        opt.step()
        ada.step()
        sq = opt.last_grad_norm.cpu()  # the f32 squared norm the kernels read; the coefficient in their f32 arithmetic
        clip = torch.minimum(torch.tensor(1.0), torch.tensor(CLIP, dtype=F32) / (sq.sqrt() + torch.tensor(1e-6, dtype=F32)))[0]
        assert float(clip) < 1.0 and float(opt.last_grad_norm) == float(ada.last_grad_norm)
        for n in rest:  # the AdamW side: FusedAdamW's bits, parameter and both moments
            off, k = lay.entries[n][0], lay.numel(n)
            for a, b in ((model.engine.flat, twin.engine.flat), (opt._m, ada._m), (opt._v, ada._v)):
                assert torch.equal(a[off:off + k], b[off:off + k]), (s, n)
        names, norms = opt.last_ns_norms
        assert names == [n for n in mats if n not in frozen] and bool((norms > 0).all())
        assert len(opt._active_ranges()) == 3  # the frozen matrices split the buffer: key | query + key (neighbours) between runs
        for n in mats:
            _, _, off, xoff, rows, cols = next(m for m in opt._matrices() if m[0] == n)
            buf = opt._buf[xoff:xoff + rows * cols].view(rows, cols).cpu()
            if n in frozen:
                assert torch.equal(by_name[n].detach().cpu(), W0[n]) and bool((buf == SENTINEL).all()), (s, n)
                continue
            g = lay.view(gs[s], n).float() * clip
            tparam[n].grad = g.clone()
            topt[n].step()
            want = topt[n].state[tparam[n]]["momentum_buffer"]
            ulp = 2.0 ** -23 * float(want.abs().max())
            assert float((buf - want).abs().max()) <= 4 * (s + 1) * ulp, (s, n)
            if s == 0:  # the first step's update against the f64 iteration, torch fed the same g
                u = mr.momentum_update(torch.zeros_like(g).double(), g.double(), 0.95, nesterov)[1].float()
                e, exact = mr.e_ref(u)
                scale = lr_of[n] * mr.ratio("match_rms_adamw", rows, cols)
                dW = (by_name[n].detach().cpu().double() - W0[n].double() * (1 - lr_of[n] * wd_of[n])) / -scale
                d = mr.rel(dW, exact)
                worst = max(worst, d / e)
                assert d <= mr.MARGIN * e, (n, d, e)
    print(f"[muon optimizer nesterov={nesterov}] worst first-step ratio to e_ref {worst:.3f} (allowed {mr.MARGIN})")


# ================================================================================================ 4. the model
@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_model_step_against_the_references(dev, precision):
    """g from the engine's flat gradient buffer after one backward; the GPU step beside _muon_ref and torch.optim.Muon +
    torch.optim.AdamW fed those same g."""
    model, x, labels = _l3(dev, precision)
    opt = _fused(model)
    lay, eng = model.engine.layout, model.engine
    opt.zero_grad()
    model(x, labels=labels).loss.backward()
    g = eng.grads.detach().cpu().clone()
    by_name = dict(model.named_parameters())
    before = {n: p.detach().cpu().clone() for n, p in by_name.items()}
    opt.step()
    mats, rest = opt.muon_split()
    worst = 0.0
    for n in mats:
        rows, cols = lay.entries[n][1]
        grp = opt._group_for(by_name[n])
        gn = lay.view(g, n)
        u = mr.momentum_update(torch.zeros_like(gn).double(), gn.double(), 0.95, True)[1].float()
        e, exact = mr.e_ref(u)
        W64 = mr.muon_step(before[n], gn, torch.zeros_like(gn), lr=grp["lr"], weight_decay=grp["weight_decay"])[0]
        tp = torch.nn.Parameter(before[n].clone())
        tp.grad = gn.clone()
        torch.optim.Muon([tp], lr=grp["lr"], weight_decay=grp["weight_decay"], adjust_lr_fn="match_rms_adamw").step()
        scale = grp["lr"] * mr.ratio("match_rms_adamw", rows, cols)
        decayed = before[n].double() * (1 - grp["lr"] * grp["weight_decay"])
        d_hip = mr.rel((by_name[n].detach().cpu().double() - decayed) / -scale, exact)
        d_torch = mr.rel((tp.detach().double() - decayed) / -scale, exact)
        worst = max(worst, d_hip / e)
        assert d_hip <= mr.MARGIN * e, (n, d_hip, e, d_torch)
        assert mr.rel(by_name[n].detach().cpu(), W64) <= mr.MARGIN * e * scale * float(exact.norm()) / float(W64.norm()) + 1e-6
    print(f"[muon model {precision}] worst ratio to e_ref {worst:.3f} (allowed {mr.MARGIN})")
    for n in rest:  # torch.optim.AdamW on the same g: one f32 step apart at most a few ulps
        grp = opt._group_for(by_name[n])
        tp = torch.nn.Parameter(before[n].clone())
        tp.grad = lay.view(g, n).clone()
        torch.optim.AdamW([tp], lr=grp["lr"], weight_decay=grp["weight_decay"]).step()
        assert float((by_name[n].detach().cpu() - tp.detach()).abs().max()) <= 1e-6 * max(1.0, float(tp.detach().abs().max())), n
    if eng.precision == "bf16":
        k = lay.n_trainable
        assert torch.equal(eng.shadow[:k], eng.flat[:k].bfloat16())


def test_state_dict_round_trip_is_bit_identical(dev):
    def one_step(model, x, labels, opt):
        opt.zero_grad()
        model(x, labels=labels).loss.backward()
        opt.step()

    model, x, labels = _l3(dev, "bf16-mixed")
    opt = _fused(model)
    opt.set_grad_clip(CLIP)
    for _ in range(2):
        one_step(model, x, labels, opt)
    sd, weights = opt.state_dict(), {k: v.detach().clone() for k, v in model.state_dict().items()}
    index = {id(p): i for i, p in enumerate(opt._all_params())}
    mats, rest = opt.muon_split()
    by_name = dict(model.named_parameters())
    for n in mats:
        assert set(sd["state"][index[id(by_name[n])]]) == {"momentum_buffer"}
    for n in rest:
        assert set(sd["state"][index[id(by_name[n])]]) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["param_groups"][0]["ns_steps"] == 5 and sd["param_groups"][0]["adjust_lr"] == "match_rms_adamw"
    one_step(model, x, labels, opt)
    model2, _, _ = _l3(dev, "bf16-mixed")
    opt2 = _fused(model2)
    opt2.set_grad_clip(CLIP)
    model2.load_state_dict(weights)
    opt2.load_state_dict(sd)
    assert opt2._step == 2
    one_step(model2, x, labels, opt2)
    n = model.engine.layout.n_trainable
    assert torch.equal(model.engine.flat[:n], model2.engine.flat[:n]) and torch.equal(opt._buf, opt2._buf)
    assert torch.equal(opt._m[:n], opt2._m[:n]) and torch.equal(opt._v[:n], opt2._v[:n])
    assert torch.equal(opt.last_ns_norms[1], opt2.last_ns_norms[1])


MUON_CFG = {"type": "muon", "lr": 2e-3, "weight_decay": 0.05, "no_decay": True, "layer_decay": 0.75}


@pytest.mark.parametrize("precision", ["32", "bf16-mixed"])
def test_hip_graph_step_equals_eager(dev, precision):
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.graph import GraphedTrainStep
    from vit_amd.optimizer import FusedMuon

    batches = list(Batches(64, 5))
    finals = {}
    for mode in ("eager", "graph"):
        cfg = c1_config(precision=precision, hip_graph=(mode == "graph"))
        cfg["opt"] = dict(MUON_CFG)
        cfg["data"]["num_samples"] = 64
        module, trainer = make(cfg)
        module.model.config.hidden_dropout_prob = 0.0
        module.model.config.attention_probs_dropout_prob = 0.0
        trainer._setup(module)
        module.train()
        opt = trainer.optimizer
        assert type(opt) is FusedMuon and len(opt.param_groups) == 10
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
        names, norms = opt.last_ns_norms
        finals[mode] = (losses, {k: v.detach().cpu().clone() for k, v in module.model.state_dict().items()},
                        [getattr(opt, name).detach().cpu().clone() for name in opt._STATE], float(opt.last_grad_norm), opt._step,
                        names, norms.cpu().clone())
        if mode == "graph":
            assert trainer.use_graph
            assert len(trainer._graphed) == 1 and all(isinstance(g, GraphedTrainStep) for g in trainer._graphed.values())
    e, g = finals["eager"], finals["graph"]
    assert e[0] == g[0], (e[0], g[0])
    for k in e[1]:
        assert torch.equal(e[1][k], g[1][k]), k
    assert len(e[2]) == 3 and all(torch.equal(a, b) for a, b in zip(e[2], g[2]))
    assert e[3] == g[3] and e[4] == g[4] == 4
    assert e[5] == g[5] and len(e[5]) == 18 and torch.equal(e[6], g[6])
    assert e[0][0] != e[0][2]  # the parameters moved


def test_two_steps_with_weight_averaging_attached(dev):
    from test_trainer_gpu import Batches, c1_config, make
    from vit_amd.optimizer import FusedMuon

    cfg = c1_config(precision="bf16-mixed", hip_graph=False)
    cfg["opt"] = dict(MUON_CFG)
    cfg["train"]["ema_decay"] = 0.9
    cfg["data"]["num_samples"] = 64
    module, trainer = make(cfg)
    trainer._setup(module)
    module.train()
    assert type(trainer.optimizer) is FusedMuon and trainer.averager is not None
    start = module.model.engine.flat.detach().clone()
    batches = list(Batches(64, 5))
    for i in range(2):
        loss = trainer.training_step(module, tuple(t.cuda() for t in batches[i % 2]), i)
        assert bool(torch.isfinite(loss))
    n = module.model.engine.layout.n_trainable
    assert trainer.optimizer._step == 2 and bool(torch.isfinite(module.model.engine.flat[:n]).all())
    assert not torch.equal(start[:n], module.model.engine.flat[:n]) and trainer.averager.n_averaged >= 1
