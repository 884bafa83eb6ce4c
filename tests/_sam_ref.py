"""Host restatements of sharpness-aware minimisation (include/vit_amd_sam.h, vit_amd/sam.py): the two perturbation formulas in
numpy f32 with the norm summed in float64, and `oracle_sam` -- the CPU oracle (oracle/refvit.py, not edited) run twice on one
batch with the same masks, at w and at w + eps, gradients by autograd.
"""
import numpy as np
import torch

EPS = 1e-12  # davda54/sam: scale = rho / (grad_norm + 1e-12)


def sqnorm(p: np.ndarray, g: np.ndarray, adaptive: bool) -> float:
    """sum (a_i g_i)^2 in float64, a_i = |p_i| if adaptive else 1 -- of the f32 products the kernel squares."""
    g = np.asarray(g, dtype=np.float32)
    t = (np.abs(np.asarray(p, dtype=np.float32)) * g).astype(np.float32) if adaptive else g
    return float(np.sum(t.astype(np.float64) ** 2))


def scale(sq: float, rho: float) -> np.float32:
    """s = rho / (sqrt(sq) + 1e-12) as the kernel forms it from the f32 cell: every operation an f32 one."""
    return np.float32(np.float32(rho) / (np.sqrt(np.float32(sq)) + np.float32(EPS)))


def epsilon(p: np.ndarray, g: np.ndarray, rho: float, adaptive: bool, sq: float = None) -> np.ndarray:
    """e = c * g * s elementwise in f32, c = p^2 if adaptive else 1; `sq`: the squared norm over EVERY perturbed element when p, g
    are one run of several (default: of these)."""
    p, g = np.asarray(p, dtype=np.float32), np.asarray(g, dtype=np.float32)
    s = scale(sqnorm(p, g, adaptive) if sq is None else sq, rho)
    u = ((p * p).astype(np.float32) * g).astype(np.float32) if adaptive else g
    return (u * s).astype(np.float32)


def ascend(p: np.ndarray, g: np.ndarray, rho: float, adaptive: bool, sq: float = None) -> np.ndarray:
    """w' = w + e in f32 (the kernel fuses the last multiply and the add: at most one rounding of w' apart)."""
    return (np.asarray(p, dtype=np.float32) + epsilon(p, g, rho, adaptive, sq)).astype(np.float32)


def named_epsilon(sd, grads, rho: float, adaptive: bool):
    """{name: e} over the tensors of `grads` (every perturbed tensor), one norm over all of them."""
    names = sorted(grads)
    sq = sum(sqnorm(sd[k].detach().numpy(), grads[k].detach().numpy(), adaptive) for k in names)
    return {k: torch.from_numpy(epsilon(sd[k].detach().numpy(), grads[k].detach().numpy(), rho, adaptive, sq)).view(sd[k].shape)
            for k in names}


def _default_step(rc, params, flux, labels, masks):
    from oracle import refvit

    out = refvit.forward(rc, params, flux, labels, training=masks is not None, masks=masks)
    return out.loss, out.logits


def _grad_pass(rc, sd, flux, labels, masks, step):
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    loss, logits = step(rc, params, flux, labels, masks)
    loss.backward()
    return float(loss.detach()), logits.detach(), {k: p.grad for k, p in params.items() if p.grad is not None}


def oracle_sam(rc, sd, flux, labels, masks, rho, adaptive, eps=None, step=None):
    """The oracle's two passes with the same `masks` (None: evaluation mode, no dropout).  Returns a dict: `loss`, `logits`, `g`
    of the first pass, `eps` = {name: e} from g, and `loss_sam`, `g_sam` at w + eps.  With `eps` given the first pass is skipped
    (`loss`, `logits`, `g` are None) and the second runs at w + eps.  `step(rc, params, flux, labels, masks) -> (loss, logits)`
    replaces the plain refvit.forward (a moved head, folded scales, a masked reconstruction)."""
    step = _default_step if step is None else step
    loss = logits = g = None
    if eps is None:
        loss, logits, g = _grad_pass(rc, sd, flux, labels, masks, step)
        eps = named_epsilon(sd, g, rho, adaptive)
    moved = {k: (v.detach() + eps[k]).float() if k in eps else v.detach() for k, v in sd.items()}
    loss_sam, _, g_sam = _grad_pass(rc, moved, flux, labels, masks, step)
    return dict(loss=loss, logits=logits, g=g, eps=eps, loss_sam=loss_sam, g_sam=g_sam)


def davda_first_step(params, grads, rho: float, adaptive: bool):
    """The first step of davda54/sam's SAM.first_step, directly in torch: e_w = (p^2 if adaptive else 1) * g * rho / (norm + 1e-12),
    norm = || stack(|| (|p| if adaptive else 1) * g ||_2 over the tensors) ||_2.  Returns [p + e_w]."""
    norm = torch.norm(torch.stack([((p.abs() if adaptive else 1.0) * g).norm(p=2) for p, g in zip(params, grads)]), p=2)
    s = rho / (norm + EPS)
    return [p + (p.pow(2) if adaptive else 1.0) * g * s for p, g in zip(params, grads)]
