"""The semantics of include/vit_amd_mix.h in numpy float64: the yardstick of tests/test_mix_cpu.py and tests/test_mix_gpu.py (not
a test module).  Every number that crosses the C ABI as an f32 -- the plan's weights, `on` / `off`, the signal, regression labels
-- enters here as that f32, widened exactly; nothing else is rounded.

A plan row is (w, u, lo, hi, wy, uy); the partner of sample b in a batch of B is p = B - 1 - b.

    out[b, i] = x[p, i]                       if lo <= i < hi
              = x[b, i]                       else if u == 0 or p == b
              = w * x[b, i] + u * x[p, i]     otherwise
    reg:  yout[b, :] = wy * y[b, :] + uy * y[p, :]                     (uy == 0: y[b, :])
    cls:  tout[b, c] = wy * oh(y[b])[c] + uy * oh(y[p])[c]             (uy == 0: oh(y[b])[c])
          oh(k)[c] = on if c == k else off;  off = s / C, on = 1 - s + off
"""
import numpy as np

IDENTITY = (1.0, 0.0, 0, 0, 1.0, 0.0)


def f32(v):
    return float(np.float32(v))


def row_of(rows, b):
    return rows[b] if len(rows) > 1 else rows[0]


def clamp_span(lo, hi, L):
    return min(max(int(lo), 0), L), min(max(int(hi), 0), L)


def mix_signal(x, rows):
    """x: [B, L] (f32 values) -> (out float64 [B, L], kind int8 [B, L], bound float64 [B, L]).
    kind: 0 = the sample's own element (bit copy), 1 = the partner's (bit copy), 2 = mixed; bound = |w x_b| + |u x_p| where
    mixed (the magnitudes the f32 roundings are relative to), 0 elsewhere."""
    x = np.asarray(x, dtype=np.float64)
    B, L = x.shape
    out, kind, bound = x.copy(), np.zeros((B, L), np.int8), np.zeros((B, L))
    idx = np.arange(L)
    for b in range(B):
        p = B - 1 - b
        w, u, lo, hi, _, _ = row_of(rows, b)
        w, u = float(np.float32(w)), float(np.float32(u))
        lo, hi = clamp_span(lo, hi, L)
        span = (idx >= lo) & (idx < hi)
        if u != 0.0 and p != b:
            out[b] = w * x[b] + u * x[p]
            kind[b] = 2
            bound[b] = np.abs(w * x[b]) + np.abs(u * x[p])
        out[b, span] = x[p, span]
        kind[b, span] = 1 if p != b else 0
        bound[b, span] = 0.0
    return out, kind, bound


def on_off(smoothing, C):
    """(on, off) in double, as the caller forms them; they cross the ABI as f32(on), f32(off)."""
    off = smoothing / C
    return 1.0 - smoothing + off, off


def one_hot(y, C, on, off):
    """Smoothed one-hot rows [B, C] in float64 from the f32 values of on / off; a label outside [0, C) selects no `on`."""
    y = np.asarray(y).astype(np.int64)
    t = np.full((y.shape[0], C), float(np.float32(off)))
    for b, k in enumerate(y):
        if 0 <= k < C:
            t[b, k] = float(np.float32(on))
    return t


def mix_rows(t, rows):
    """t: [B, C] float64 (regression labels or one-hot rows) -> (mixed [B, C], bound [B, C], copied bool [B])."""
    t = np.asarray(t, dtype=np.float64)
    B = t.shape[0]
    out, bound, copied = t.copy(), np.zeros_like(t), np.ones(B, bool)
    for b in range(B):
        p = B - 1 - b
        wy, uy = (float(np.float32(v)) for v in row_of(rows, b)[4:6])
        if uy != 0.0:
            out[b] = wy * t[b] + uy * t[p]
            bound[b] = np.abs(wy * t[b]) + np.abs(uy * t[p])
            copied[b] = False
    return out, bound, copied


def mix_targets_reg(y, rows):
    y = np.asarray(y, dtype=np.float64)
    return mix_rows(y.reshape(y.shape[0], -1), rows)


def mix_targets_cls(y, rows, C, smoothing=0.0):
    on, off = on_off(smoothing, C)
    return mix_rows(one_hot(y, C, on, off), rows)


# ---- the soft losses, as torch states them (used where a test wants them in float64 without torch)
def soft_ce(z, t):
    z, t = np.asarray(z, np.float64), np.asarray(t, np.float64)
    m = z.max(axis=1, keepdims=True)
    logp = z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    return float(-(t * logp).sum(axis=1).mean())


def bce(z, t):
    z, t = np.asarray(z, np.float64), np.asarray(t, np.float64)
    return float((np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))).mean())
