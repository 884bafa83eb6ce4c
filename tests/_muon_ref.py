"""The Muon contract of include/vit_amd_muon.h restated in float64 on CPU tensors, with (`rounded=True`) and without the bf16
rounding points, beside torch.optim.Muon itself.

The yardstick the GPU tests use: for one input matrix u, e_ref = rel(torch.optim.Muon's orthogonalisation, the unrounded f64
iteration) -- the distance a correct bf16 implementation sits from exact arithmetic on that very input.  A kernel result O must
satisfy rel(O, f64) <= 1.5 * e_ref; two independent correct bf16 implementations (torch's, and `newton_schulz(rounded=True)`)
sit at 0.88 .. 1.07 of each other's distance, a missing rounding point or a wrong coefficient moves the result by O(1)."""
import math

import torch

COEFFS = (3.4445, -4.775, 2.0315)
MARGIN = 1.5


def bf(x):
    """One bf16 rounding of an f64 tensor, back in f64 (through f32, as the kernels hold their values before they round)."""
    return x.to(torch.float32).bfloat16().double()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def ratio(mode, rows, cols):
    if mode == "original":
        return math.sqrt(max(1, rows / cols))
    if mode == "match_rms_adamw":
        return 0.2 * math.sqrt(max(rows, cols))
    return 1.0


def momentum_update(buf, g, momentum=0.95, nesterov=True):
    """(buf', u) in the dtype of the inputs (f64 for the reference)."""
    buf = buf + (1 - momentum) * (g - buf)
    return buf, (g + momentum * (buf - g)) if nesterov else buf


def newton_schulz(u, coefficients=COEFFS, ns_steps=5, eps=1e-7, rounded=False, with_norm=False):
    """O [rows, cols] (f64) from u [rows, cols]; `rounded`: bf16 at the contract's rounding points."""
    r = bf if rounded else (lambda t: t)
    a, b, c = coefficients
    X = r(u.double())
    wide = X.shape[0] <= X.shape[1]
    if not wide:
        X = X.T
    nrm = float(X.pow(2).sum().sqrt())
    inv = float(torch.tensor(1.0 / max(nrm, eps), dtype=torch.float32)) if rounded else 1.0 / max(nrm, eps)
    X = r(X * inv)
    for _ in range(ns_steps):
        A = r(X @ X.T)
        B = r(b * A + c * (A @ A))
        X = r(a * X + B @ X)
    O = X if wide else X.T
    return (O, nrm) if with_norm else O


def torch_newton_schulz(u, coefficients=COEFFS, ns_steps=5, eps=1e-7):
    """torch.optim.Muon's own orthogonalisation of u (f32), read off one step on W = 0 with lr 1, no decay, no momentum."""
    W = torch.nn.Parameter(torch.zeros_like(u, dtype=torch.float32))
    opt = torch.optim.Muon([W], lr=1.0, weight_decay=0.0, momentum=0.0, nesterov=False, ns_coefficients=tuple(coefficients),
                           eps=eps, ns_steps=ns_steps, adjust_lr_fn="original" if u.shape[0] <= u.shape[1] else None)
    W.grad = u.detach().float().clone()
    opt.step()
    scale = ratio("original", *u.shape)  # W = -ratio * O
    return (-W.detach().double()) / scale


def e_ref(u, **kw):
    """(e_ref, O_f64): torch's distance from the unrounded f64 iteration on u, and that iteration's result."""
    exact = newton_schulz(u, rounded=False, **kw)
    return rel(torch_newton_schulz(u, **kw), exact), exact


def muon_step(W, g, buf, *, lr, weight_decay, momentum=0.95, nesterov=True, coefficients=COEFFS, ns_steps=5, eps=1e-7,
              adjust="match_rms_adamw", clip=1.0, rounded=False):
    """One step of the contract in f64: (W', buf', O, ||X0||)."""
    W, g, buf = W.double(), g.double() * clip, buf.double()
    buf, u = momentum_update(buf, g, momentum, nesterov)
    O, nrm = newton_schulz(u, coefficients, ns_steps, eps, rounded, with_norm=True)
    W = W * (1 - lr * weight_decay) - lr * ratio(adjust, *W.shape) * O
    return W, buf, O, nrm


def low_rank(rows, cols, rank, noise, gen):
    """An ill-conditioned input: rank `rank` plus `noise` (relative) of N(0, 1)."""
    core = torch.randn(rows, rank, generator=gen) @ torch.randn(rank, cols, generator=gen) / math.sqrt(rank)
    return core + noise * torch.randn(rows, cols, generator=gen)
