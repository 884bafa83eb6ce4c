"""ORACLE (test infrastructure, NOT product code): host restatement of the dropout masks the HIP kernels draw.

The masks are counter-based and stateless (vit_amd/csrc/common.h:56-112), so every one of them can be rebuilt here, for any
shape, from integers alone:
  * make_drop: thr = (unsigned)(p * 65536.0f + 0.5f) clamped to 65535 (0 = off), scale = 65536.0f / (65536 - thr), both in
    float32; the two 32-bit keys (k0, k1) are the halves of splitmix64(seed + phi * (site + 1));
  * drop_hash (row key): a 32-bit hash of (k0, k1, 64-bit row index);
  * drop_bits: one 32-bit word per PAIR of columns, word = drop_bits(rowkey, col / 2); column `col` draws the low (even col)
    or the high (odd col) 16 bits; keep <=> r16 >= thr, kept values are multiplied by `scale` (which is NOT 1 / (1 - p));
  * resolve_drop: a bound per-step record (vit_step_state_bind) XORs its (key0, key1) into (k0, k1) when thr != 0;
    step_advance_kernel (elementwise.hip:755) derives those keys from splitmix64(base_seed + phi * step).

Layouts of the engine's sites (vit_amd/engine.py:364-395):
  * the step seed is base_seed + 0x9E3779B97F4A7C15 * step_counter (mod 2^64); a training forward increments step_counter
    before it draws;
  * site 0 = embedding dropout, site 1 + 4 * layer + {0: attention probabilities, 1: attention-output projection, 2: FC2};
  * hidden / embedding sites are [B*T, D] with row b*T + t (the CLS row included, t = 0);
  * attention is [B*H*T, T] with row (b*H + h)*T + q and column = key (attn_fwd_kernel, attn_bwd_dq_kernel,
    attn_bwd_dkv_kernel, attn32_row_kernel and the other forms in vit_amd/csrc/attention_*.hip).
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np

PHI = 0x9E3779B97F4A7C15
M64 = 0xFFFFFFFFFFFFFFFF
M32 = 0xFFFFFFFF

DropCfg = Tuple[int, float, int, int]  # (thr, scale, k0, k1)


def splitmix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def thr_scale(p: float) -> Tuple[int, float]:
    """make_drop's threshold and kept-value scale, in float32 as the C++ computes them."""
    if p <= 0.0:
        return 0, 1.0
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))  # float -> unsigned truncates
    thr = min(thr, 65535)
    scale = float(np.float32(65536.0) / np.float32(65536 - thr))
    return thr, scale


def drop_cfg(p: float, seed: int, site: int) -> DropCfg:
    """make_drop(p, seed, site) (common.h:90-104): (thr, scale, k0, k1)."""
    thr, scale = thr_scale(p)
    z = splitmix64((seed + PHI * (site + 1)) & M64)
    return thr, scale, z & M32, z >> 32


def step_seed(base_seed: int, step_counter: int) -> int:
    """The eager forward's seed (engine.py:393-395): base_seed + phi * step_counter, mod 2^64."""
    return (base_seed + PHI * step_counter) & M64


def step_keys(base_seed: int, step: int) -> Tuple[int, int]:
    """(key0, key1) that step_advance_kernel writes for the record's new step count `step`."""
    z = splitmix64((base_seed + PHI * step) & M64)
    return z & M32, z >> 32


def step_record(base_seed: int, step: int, beta1: float = 0.9, beta2: float = 0.999):
    """The whole record after step_advance_kernel has moved it to `step`: (key0, key1, bc1, rsqrt_bc2, step).  The betas
    travel to the kernel as float32 and are widened to double there; the corrections are computed in double and rounded
    to float32."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    k0, k1 = step_keys(base_seed, step)
    bc1 = np.float32(1.0 - b1 ** step)
    rbc2 = np.float32(1.0 / (1.0 - b2 ** step) ** 0.5)
    return k0, k1, bc1, rbc2, step


def _u64(x) -> np.ndarray:
    return np.asarray(x, dtype=np.uint64)


_C = {name: np.uint64(v) for name, v in dict(
    m32=M32, g=0x9E3779B9, h1=0x7FEB352D, h2=0x846CA68B, b1=0x2C1B3C6D, b2=0x297A2D39).items()}
_S = {n: np.uint64(n) for n in (15, 16, 32)}


def drop_hash(k0: int, k1: int, idx) -> np.ndarray:
    """Row key (common.h:66-70), vectorised over uint64 row indices."""
    idx = _u64(idx)
    m = _C["m32"]
    x = (idx & m) ^ np.uint64(k0) ^ (((idx >> _S[32]) * _C["g"]) & m)
    x ^= x >> _S[16]
    x = (x * _C["h1"]) & m
    x = (x + np.uint64(k1)) & m
    x ^= x >> _S[15]
    x = (x * _C["h2"]) & m
    x ^= x >> _S[16]
    return x


def drop_bits(rowkey, colpair) -> np.ndarray:
    """The word of one column pair (common.h:71-75); broadcasts rowkey against colpair."""
    m = _C["m32"]
    x = ((_u64(colpair) ^ _u64(rowkey)) * _C["b1"]) & m
    x ^= x >> _S[15]
    x = (x * _C["b2"]) & m
    x ^= x >> _S[16]
    return x


def _resolved(cfg: DropCfg, keys_xor: Optional[Tuple[int, int]]) -> DropCfg:
    thr, scale, k0, k1 = cfg
    if thr and keys_xor is not None:  # resolve_drop: the record is only consulted when dropout is on
        k0, k1 = k0 ^ (keys_xor[0] & M32), k1 ^ (keys_xor[1] & M32)
    return thr, scale, k0, k1


def draws(cfg: DropCfg, rows: int, cols: int, row0: int = 0, keys_xor: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The 16-bit draw r16 of every element of rows [row0, row0 + rows) x cols [0, cols), uint32 [rows, cols]."""
    _, _, k0, k1 = _resolved(cfg, keys_xor)
    rk = drop_hash(k0, k1, np.arange(row0, row0 + rows, dtype=np.uint64))[:, None]
    col = np.arange(cols, dtype=np.uint64)[None, :]
    w = drop_bits(rk, col >> np.uint64(1))
    r16 = np.where((col & np.uint64(1)) == 1, w >> _S[16], w & np.uint64(0xFFFF))
    return r16.astype(np.uint32)


def keep_mask(cfg: DropCfg, rows: int, cols: int, row0: int = 0, keys_xor: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """bool [rows, cols]: True where the element is kept.  thr == 0 (dropout off) keeps everything."""
    if cfg[0] == 0:
        return np.ones((rows, cols), dtype=bool)
    return draws(cfg, rows, cols, row0, keys_xor) >= cfg[0]


def multiplier(cfg: DropCfg, rows: int, cols: int, row0: int = 0, keys_xor: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """float32 [rows, cols]: 0 or scale (1 everywhere when dropout is off)."""
    if cfg[0] == 0:
        return np.ones((rows, cols), dtype=np.float32)
    return np.where(keep_mask(cfg, rows, cols, row0, keys_xor), np.float32(cfg[1]), np.float32(0.0)).astype(np.float32)


# --------------------------------------------------------------------------- the engine's sites
def site_of(layer: int, which: int) -> int:
    """engine.py:364-365: 1 + 4 * layer + {0: attention, 1: attention-output projection, 2: FC2}; 0 is the embedding."""
    return 1 + 4 * layer + which


def hidden_multiplier(cfg: DropCfg, B: int, T: int, D: int, keys_xor=None) -> np.ndarray:
    """[B, T, D] multiplier of a hidden / embedding site (row b*T + t)."""
    return multiplier(cfg, B * T, D, keys_xor=keys_xor).reshape(B, T, D)


def attn_multiplier(cfg: DropCfg, B: int, H: int, T: int, keys_xor=None) -> np.ndarray:
    """[B, H, T(query), T(key)] multiplier of an attention site (row (b*H + h)*T + q, column = key)."""
    return multiplier(cfg, B * H * T, T, keys_xor=keys_xor).reshape(B, H, T, T)


def engine_masks(p_hidden: float, p_attn: float, seed: int, keys_xor=None) -> Callable:
    """`masks` callable for oracle.refvit.forward: (site, shape) -> float32 torch multiplier, the masks the engine's kernels
    draw at step seed `seed` (step_seed(base_seed, step_counter)); `keys_xor`: the bound record's keys (graph replays).
    The oracle names its attention site by the engine's site number and passes a 4-D [B, H, T, T] shape; hidden sites
    get a 3-D [B, T, D] shape."""
    import torch

    def masks(site: int, shape) -> "torch.Tensor":
        attn = len(shape) == 4
        cfg = drop_cfg(p_attn if attn else p_hidden, seed, site)
        if attn:
            B, H, T, _ = shape
            m = attn_multiplier(cfg, B, H, T, keys_xor)
        else:
            B, T, D = shape
            m = hidden_multiplier(cfg, B, T, D, keys_xor)
        return torch.from_numpy(m)

    return masks
