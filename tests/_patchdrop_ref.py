"""Host restatements of patch dropout (include/vit_amd_patchdrop.h), built on oracle/dropmask.py: what the select kernel draws
and the pieces the model tests assemble an oracle run from.

The site: a step's (seed, site) slots are 0 for the embedding dropout and 1 + 4 i + {0, 1, 2, 3} for layer i (attention
probabilities, attention-output projection, FC2, the stochastic-depth gates: oracle.dropmask.site_of, ViTEngine._site).  The
selection draws from `select_site(L)` = site_of(L, 0) = 1 + 4 L, the first slot behind the last layer's: no dropout mask and
no path gate of an L-layer model uses it.
"""
import numpy as np

from oracle import dropmask as dm


def select_site(num_layers: int) -> int:
    return dm.site_of(num_layers, 0)


def kept(N: int, rate: float) -> int:
    """timm's PatchDropout: max(1, int(N * (1 - rate))) in Python doubles."""
    return max(1, int(N * (1.0 - rate)))


def select(B: int, N: int, K: int, seed: int, site: int, keys_xor=None):
    """(idx int32 [B, K], slot int32 [B, N]) of vit_patch_select: key(b, n) = drop_hash(k0, k1, b * N + n) with make_drop's keys
    of (seed, site) -- XORed with a bound record's keys ALWAYS (the selection has no threshold whose zero means "off") -- and
    sample b keeps the K patches smallest under (key, n), listed in ascending n; slot is the inverse map, -1 for a dropped patch."""
    _, _, k0, k1 = dm.drop_cfg(0.0, seed, site)
    if keys_xor is not None:
        k0, k1 = k0 ^ (keys_xor[0] & dm.M32), k1 ^ (keys_xor[1] & dm.M32)
    keys = dm.drop_hash(k0, k1, np.arange(B * N, dtype=np.uint64)).reshape(B, N)
    order = np.argsort(keys, axis=1, kind="stable")  # stable: equal keys stay in ascending n
    idx = np.sort(order[:, :K], axis=1).astype(np.int32)
    return idx, slot_of(idx, N)


def slot_of(idx: np.ndarray, N: int) -> np.ndarray:
    B, K = idx.shape
    slot = np.full((B, N), -1, dtype=np.int32)
    slot[np.arange(B)[:, None], idx] = np.arange(K, dtype=np.int32)[None, :]
    return slot


def positions(idx: np.ndarray) -> np.ndarray:
    """int64 [B, 1 + K]: the original position of every compact token (0 = CLS, 1 + n for patch n)."""
    B = idx.shape[0]
    return np.concatenate([np.zeros((B, 1), dtype=np.int64), 1 + idx.astype(np.int64)], axis=1)


def worst_sigma(idx: np.ndarray, N: int) -> float:
    """The largest deviation of a patch's keep frequency over the batch from K / N, in units of sigma = sqrt(p (1 - p) / B)."""
    B, K = idx.shape
    p = K / N
    freq = np.bincount(idx.reshape(-1), minlength=N) / B
    return float(np.abs(freq - p).max() / np.sqrt(p * (1 - p) / B))


def shortened_signal(flux, idx: np.ndarray, P: int):
    """x'[b] = the kept patches of sample b side by side (stride == patch size): the signal of a model with image_size K * P
    whose tokens are exactly the kept tokens.  flux: torch [B, L]."""
    import torch

    B, K = idx.shape
    cols = (torch.from_numpy(idx.astype(np.int64))[:, :, None] * P + torch.arange(P)[None, None, :]).reshape(B, K * P)
    return torch.gather(flux, 1, cols)
