"""The yardstick of tests/test_lamb_gpu.py (NOT a test module): LAMB as include/vit_amd_optim.h states it, restated in plain torch
ops as a torch.optim.Optimizer on CPU tensors.

    g' = g * clip,  clip = min(1, max_norm / (sqrt(sqnorm) + 1e-6))      (no clip: 1)
    m  = beta1 * m + (1 - beta1) * g'          v = beta2 * v + (1 - beta2) * g'^2
    u  = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)   [+ weight_decay * p   if weight_decay != 0]
    r  = (weight_decay != 0 or always_adapt) and ||p|| > 0 and ||u|| > 0 ? ||p|| / ||u|| : 1;  trust_clip: r = min(r, 1)
    p -= lr * r * u

It runs in the dtype of the parameters it is given: float64 is the reference, float32 the yardstick -- the f32 run's distance
from the f64 run, per tensor in max-norm, is `d32`, and the kernels must lie within 4 * d32 + 1 ulp of the f64 run (`bound`; the
ulp is f32's at the tensor's largest reference magnitude).  The factor 4 covers fma and summation orders other than torch's; it
is a margin over the restatement's own error, not a tuned constant.

Every number that crosses the C ABI as an f32 (lr, betas, eps, weight_decay, max_norm, the squared gradient norm) enters both
runs as that f32's value; 1 - beta is 1.f - beta, the bias corrections are formed in double from the f32 betas: all as in
the library."""
import math

import numpy as np
import torch


def f32(x) -> float:
    return float(np.float32(x))


class RefLamb(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, always_adapt=False, trust_clip=False,
                 max_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, always_adapt=always_adapt,
                                      trust_clip=trust_clip))
        self.max_norm = max_norm
        self.steps = 0
        self.trust = {}  # id(p) -> the last step's ratio, a 0-dim tensor of the run's dtype

    @torch.no_grad()
    def step(self, sqnorm=None):
        """`sqnorm`: the squared global gradient norm as the f32 the kernels read; None: formed here from the gradients."""
        self.steps += 1
        clip = 1.0
        if self.max_norm is not None:
            if sqnorm is None:
                sqnorm = f32(sum(float(p.grad.double().pow(2).sum()) for grp in self.param_groups for p in grp["params"]
                                 if p.grad is not None))
        for grp in self.param_groups:
            b1, b2 = f32(grp["betas"][0]), f32(grp["betas"][1])
            omb1, omb2 = float(np.float32(1) - np.float32(b1)), float(np.float32(1) - np.float32(b2))
            lr, wd, eps = f32(grp["lr"]), f32(grp["weight_decay"]), f32(grp["eps"])
            bc1, bc2 = 1.0 - b1 ** self.steps, 1.0 - b2 ** self.steps
            for p in grp["params"]:
                if p.grad is None:
                    continue
                dt = p.dtype
                if self.max_norm is not None:  # in the run's dtype, from the f32 inputs
                    one, mx, sq = torch.ones((), dtype=dt), torch.tensor(f32(self.max_norm), dtype=dt), torch.tensor(sqnorm, dtype=dt)
                    clip = torch.minimum(one, mx / (sq.sqrt() + torch.tensor(1e-6, dtype=torch.float32).to(dt)))
                st = self.state[p]
                if not st:
                    st["m"], st["v"] = torch.zeros_like(p), torch.zeros_like(p)
                g = p.grad.to(dt) * clip
                st["m"].mul_(b1).add_(g * omb1)
                st["v"].mul_(b2).add_(g * g * omb2)
                u = (st["m"] / bc1) / (st["v"].sqrt() / math.sqrt(bc2) + eps)
                if wd != 0:
                    u = u + wd * p
                r = torch.ones((), dtype=dt)
                pn, un = p.norm(), u.norm()
                if (wd != 0 or grp["always_adapt"]) and pn > 0 and un > 0:
                    r = pn / un
                if grp["trust_clip"]:
                    r = torch.minimum(r, torch.ones((), dtype=dt))
                self.trust[id(p)] = r.clone()
                p.sub_(lr * r * u)


def ulp32(x: float) -> float:
    """f32's spacing at |x| (its smallest normal's for 0)."""
    return float(np.spacing(np.float32(max(abs(float(x)), float(np.finfo(np.float32).tiny)))))


def bound(ref64: torch.Tensor, run32: torch.Tensor):
    """(d32, allowed): the f32 restatement's max-norm distance from the f64 one, and 4 * d32 + 1 ulp."""
    ref64 = ref64.double().reshape(-1)
    d32 = float((run32.double().reshape(-1) - ref64).abs().max())
    return d32, 4.0 * d32 + ulp32(float(ref64.abs().max()))
