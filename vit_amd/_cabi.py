"""ctypes binding of libvit_amd.so (include/vit_amd.h).  Fails loudly when the library is missing or a call errors:
there is no CPU / eager fallback anywhere in vit_amd."""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# VIT_AMD_LIB: another build of the same library, e.g. of another commit for an A/B run of bench.py
LIB_PATH = os.environ.get("VIT_AMD_LIB") or os.path.join(_HERE, "lib", "libvit_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vit_amd.h")

VIT_OK, VIT_ERR_WORKSPACE = 0, -4
VIT_F32, VIT_BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_DGELU, ACT_GELU_GRAD, ACT_MUL_AUX = 0, 1, 2, 3, 4
LOSS_MSE, LOSS_L1, LOSS_CE = 0, 1, 2
LOSS_SOFT_CE, LOSS_BCE = 3, 4  # the soft-target kinds: labels are f32 [B, C] targets
MIX_LABELS_F32, MIX_LABELS_I64 = 0, 1


class VitError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("a_trans", C.c_int), ("b_trans", C.c_int),
        ("ab_dtype", C.c_int),
        ("A", C.c_void_p), ("lda", C.c_int64),
        ("B", C.c_void_p), ("ldb", C.c_int64),
        ("C", C.c_void_p), ("ldc", C.c_int64), ("c_dtype", C.c_int),
        ("alpha", C.c_float),
        ("bias", C.c_void_p),
        ("act", C.c_int),
        ("aux_out", C.c_void_p),
        ("aux_in", C.c_void_p),
        ("ldaux", C.c_int64),
        ("dropout_p", C.c_float), ("seed", C.c_uint64), ("site", C.c_uint64),
        ("residual", C.c_void_p), ("ldres", C.c_int64),
        ("rows_per_batch", C.c_int), ("out_batch_rows", C.c_int), ("out_row_offset", C.c_int),
        ("split_k", C.c_int),
        ("accumulate", C.c_int),
        ("colsum_out", C.c_void_p),
        ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p),
        ("rope_T", C.c_int), ("rope_dh", C.c_int), ("rope_cols", C.c_int),
        ("drop_row_stride", C.c_int),
    ]


class LayerScaleEntry(C.Structure):
    """vit_layer_scale_entry (include/vit_amd_layerscale.h): one matrix of a fold / gradient table, 96 bytes."""
    _fields_ = [
        ("W", C.c_void_p), ("b", C.c_void_p), ("lam", C.c_void_p),
        ("Wf", C.c_void_p), ("bf", C.c_void_p),
        ("dW_raw", C.c_void_p), ("db_raw", C.c_void_p), ("dW", C.c_void_p), ("db", C.c_void_p), ("dlam", C.c_void_p),
        ("rows", C.c_int32), ("cols", C.c_int32),
        ("reserved", C.c_int64),
    ]


class MixRow(C.Structure):
    """vit_mix_row (include/vit_amd_mix.h): one row of a Mixup / CutMix plan, 32 bytes."""
    _fields_ = [("w", C.c_float), ("u", C.c_float), ("lo", C.c_int32), ("hi", C.c_int32), ("wy", C.c_float), ("uy", C.c_float),
                ("reserved", C.c_int32 * 2)]


class MuonMat(C.Structure):
    """vit_muon_mat (include/vit_amd_muon.h): one matrix of a Muon table, 48 bytes."""
    _fields_ = [("off", C.c_int64), ("xoff", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("group", C.c_int32),
                ("ratio", C.c_float), ("tile0", C.c_int32), ("ttile0", C.c_int32), ("reserved", C.c_int64)]


class MuonProblem(C.Structure):
    """vit_muon_problem (include/vit_amd_muon.h): one product of a grouped launch, 72 bytes."""
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("R", C.c_void_p), ("C", C.c_void_p),
                ("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("ldr", C.c_int32), ("ldc", C.c_int32),
                ("alpha", C.c_float), ("beta", C.c_float), ("reserved", C.c_int32)]


_P, _I, _F, _U64, _I64, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_int64, C.c_size_t

# name -> argtypes (restype is int unless listed in _RESTYPES)
_PROTOS = {
    "vit_version": [],
    "vit_last_error": [],
    "vit_create": [C.POINTER(_P), _I],
    "vit_destroy": [_P],
    "vit_set_workspace": [_P, _P, _SZ],
    "vit_workspace_needed": [],
    "vit_set_option": [C.c_char_p, _I],
    "vit_handle_set_option": [_P, C.c_char_p, _I],
    "vit_step_state_bind": [_P, _P],
    "vit_step_advance": [_P, _U64, _F, _F, _P],
    "vit_gemm": [_P, C.POINTER(GemmDesc), _P],
    "vit_last_gemm_kernel": [],
    "vit_linear_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _F, _U64, _U64, _P, _P],
    "vit_linear_bwd_dx": [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P],
    "vit_linear_bwd_dw": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vit_layernorm_fwd": [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _P],
    "vit_layernorm_fwd_residual": [_P, _P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _P],
    "vit_linear_bwd_dw_rows": [_P, _P, _I64, _P, _I64, _I, _P, _I, _I, _I, _I64, _I64, _P],
    "vit_colsum_rows": [_P, _P, _I, _I64, _P, _I, _I, _I64, _I64, _P],
    "vit_layernorm_fwd_residual_rows": [_P, _P, _I64, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _P],
    "vit_layernorm_bwd_rows": [_P, _P, _I, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _I, _I, _P, _I, _P, _F, _U64, _U64, _I64, _P],
    "vit_layernorm_bwd": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "vit_layernorm_bwd_fused": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _I, _P, _F, _U64, _U64, _P],
    "vit_attention_fwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _U64, _U64, _P],
    "vit_attention_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _U64, _U64, _P, _P],
    "vit_attention_probs": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _P],
    "vit_unfold_cast": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "vit_fold_add": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vit_add_noise": [_P, _P, _P, _P, C.c_long, _F, _U64, _P],
    "vit_rope_qk": [_P, _P, _I, _P, _P, C.c_long, _I, _I, _I, C.c_long, _I, _P],
    "vit_embed_finish": [_P, _P, _P, _P, _I, _I, _I, _F, _U64, _U64, _P],
    "vit_embed_finish_bwd": [_P, _P, _P, _I, _P, _P, _I, _I, _I, _F, _U64, _U64, _I, _P],
    "vit_dropout_bwd_cast": [_P, _P, _P, _I, _I, _I, _F, _U64, _U64, _P],
    "vit_colsum": [_P, _P, _I, _I64, _P, _I, _I, _I, _P],
    "vit_cov_accumulate": [_P, _P, _I64, _P, _P, _I, _I, _P],
    "vit_cov_finish": [_P, _P, _P, _I, _I64, _P],
    "vit_cov_mean_finish": [_P, _P, _I, _I64, _P],
    "vit_cast_f32_bf16": [_P, _P, _P, _I64, _P],
    "vit_cast_bf16_f32": [_P, _P, _P, _I64, _F, _P],
    "vit_head_loss_fwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vit_head_loss_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "vit_grad_sqnorm": [_P, _P, _I64, _P, _P],
    "vit_grad_sqnorm_acc": [_P, _P, _I64, _P, _P],
    "vit_adamw_step": [_P, _P, _P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _I, _P, _F, _P],
    "vit_sgd_step": [_P, _P, _P, _P, _P, _I64, _F, _F, _F, _I, _P, _F, _P],
    "vit_adam_l2_step": [_P, _P, _P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _I, _P, _F, _P],
    # (h, p, g, m, v, p_bf16, n, base, seg_end, seg_group, n_segments, groups, n_groups, beta1, beta2, eps, [step,] sqnorm, ...)
    "vit_adamw_step_groups": [_P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _F, _F, _F, _I, _P, _F, _P],
    "vit_adamw_step_groups_dyn": [_P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _F, _F, _F, _P, _F, _P],
    "vit_adam_l2_step_groups": [_P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _F, _F, _F, _I, _P, _F, _P],
    "vit_adam_l2_step_groups_dyn": [_P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _F, _F, _F, _P, _F, _P],
    "vit_sgd_step_groups": [_P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _I, _P, _F, _P],
    "vit_sgd_step_groups_dyn": [_P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _I, _P, _F, _P],
    "vit_optim_groups_write": [_P, _P, _I, C.POINTER(C.c_float), _P],
    # (h, p, g, m, v, p_bf16, n, lr, beta1, beta2, eps, weight_decay, always_adapt, trust_clip, step, sqnorm, max_norm, trust, stream)
    "vit_lamb_step": [_P, _P, _P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _I, _I, _I, _P, _F, _P, _P],
    # (h, p, g, m, v, p_bf16, n, base, seg_end, seg_group, n_segments, groups, n_groups, beta1, beta2, eps, always_adapt,
    #  trust_clip, [step,] sqnorm, max_norm, trust, stream)
    "vit_lamb_step_groups": [_P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _F, _F, _F, _I, _I, _I, _P, _F, _P, _P],
    "vit_lamb_step_groups_dyn": [_P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _I, _P, _I, _F, _F, _F, _I, _I, _P, _F, _P, _P],
    # (h, ema, p, n, weight, weight_dev, stream) / (h, p, ema, p_bf16, n, stream)
    "vit_ema_update": [_P, _P, _P, _I64, _F, _P, _P],
    "vit_ema_swap": [_P, _P, _P, _P, _I64, _P],
    # the _rows forms' arguments + (path_p, seed, path_site, rows_per_sample, branch) / (path_p, path_site, rows_per_sample, branch)
    "vit_layernorm_fwd_residual_path": [_P, _P, _I64, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _F, _F, _U64, _U64, _I, _I, _P],
    "vit_layernorm_bwd_path": [_P, _P, _I, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _I, _I, _P, _I, _P, _F, _U64, _U64, _I64, _F,
                               _U64, _I, _I, _P],
    # (h, table, entries, count, stream) / (h, table, n_entries, max_rows, out_dtype | accumulate, stream)
    "vit_layer_scale_table_write": [_P, _P, C.POINTER(LayerScaleEntry), _I, _P],
    "vit_layer_scale_fold": [_P, _P, _I, _I, _I, _P],
    "vit_layer_scale_grad": [_P, _P, _I, _I, _I, _P],
    # (h, plan_dev, n_rows, host_rows, stream) / (h, x, out, plan_dev, n_rows, B, L, stream) /
    # (h, labels, label_kind, out, plan_dev, n_rows, B, C, on, off, stream)
    "vit_mix_plan_write": [_P, _P, _I, C.POINTER(MixRow), _P],
    "vit_mix_signal": [_P, _P, _P, _P, _I, _I, _I, _P],
    "vit_mix_targets": [_P, _P, _I, _P, _P, _I, _I, _I, _F, _F, _P],
    # patch dropout (include/vit_amd_patchdrop.h): (h, idx, slot, B, N, K, seed, site, stream) /
    # (h, x, idx, patches, out_dtype, B, L, P, S, N, K, stream) / (h, tokens, cls, pos, idx, B, Tc, T_full, D, p, seed, site, stream) /
    # (h, dtokens, slot, dpatch, dpatch_dtype, dcls, dpos, B, Tc, T_full, D, p, seed, site, accumulate, stream) /
    # (h, table, idx, out, B, Tc, T_full, W, stream) / (h, dpatches, slot, dx, B, L, P, S, N, K, stream)
    "vit_patch_select": [_P, _P, _P, _I, _I, _I, _U64, _U64, _P],
    "vit_patch_slot": [_P, _P, _P, _I, _I, _I, _P],
    "vit_unfold_gather_cast": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "vit_embed_finish_gather": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _U64, _U64, _P],
    "vit_embed_finish_gather_bwd": [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _F, _U64, _U64, _I, _P],
    "vit_rows_gather": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vit_fold_add_gather": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    # masked spectrum modelling (include/vit_amd_mim.h): (h, slot_blocks, mask, B, N, Nb, span, stream) /
    # (h, tokens, cls, pos, mask, mask_token, B, T, D, p, seed, site, stream) /
    # (h, dtokens, mask, dpatch, dpatch_dtype, dcls, dpos, dmask_token, B, T, D, p, seed, site, accumulate, stream) /
    # (h, x, pred, pred_dtype, mask, loss, count, B, L, P, S, N, T, kind, norm_target, stream) /
    # (h, x, pred, pred_dtype, mask, count, dloss, dpred, dpred_dtype, B, L, P, S, N, T, kind, norm_target, stream)
    "vit_mim_mask": [_P, _P, _P, _I, _I, _I, _I, _P],
    "vit_embed_finish_masked": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _U64, _U64, _P],
    "vit_embed_finish_masked_bwd": [_P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _F, _U64, _U64, _I, _P],
    "vit_mim_loss_fwd": [_P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vit_mim_loss_bwd": [_P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    # global average pooling (include/vit_amd_pool.h): (h, x, pooled, B, T, D, first, stream) / (h, dpooled, dx, B, T, D, first, stream)
    "vit_token_pool_fwd": [_P, _P, _P, _I, _I, _I, _I, _P],
    "vit_token_pool_bwd": [_P, _P, _P, _I, _I, _I, _I, _P],
    # sharpness-aware minimisation (include/vit_amd_sam.h): (h, p, g, n, adaptive, accumulate, out, stream) /
    # (h, p, g, backup, p_bf16, n, rho, adaptive, sqnorm_dev, stream) / (h, p, backup, p_bf16, n, stream)
    "vit_sam_sqnorm": [_P, _P, _P, _I64, _I, _I, _P, _P],
    "vit_sam_ascend": [_P, _P, _P, _P, _P, _I64, _F, _I, _P, _P],
    "vit_sam_descend": [_P, _P, _P, _P, _I64, _P],
    # register tokens (include/vit_amd_registers.h): (h, tokens, cls, reg, pos, mask, mask_token, B, R, N, D, p, seed, site, stream) /
    # (h, dtokens, mask, dpatch, dpatch_dtype, dcls, dreg, dpos, dmask_token, B, R, N, D, p, seed, site, accumulate, stream)
    "vit_embed_finish_reg": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _U64, _U64, _P],
    "vit_embed_finish_reg_bwd": [_P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _F, _U64, _U64, _I, _P],
}
# Muon (include/vit_amd_muon.h, which includes vit_amd.h and is not included by it): a table of its own, bound beside _PROTOS
# (h, g, buf, u, mats, n_mats, n_tiles, momentum, nesterov, sqnorm, max_norm, part, stream) /
# (h, mats, n_mats, part, eps, inv_norm, norms, stream) / (h, u, x, mats, n_mats, n_ttiles, inv_norm, stream) /
# (h, problems, n_problems, tiles, n_tiles, b_trans, stream) / (h, p, p_bf16, o, mats, n_mats, n_ttiles, groups, n_groups, stream)
_PROTOS_MUON = {
    "vit_muon_momentum": [_P, _P, _P, _P, _P, _I, _I, C.c_double, _I, _P, _F, _P, _P],
    "vit_muon_norms": [_P, _P, _I, _P, _F, _P, _P, _P],
    "vit_muon_normalize": [_P, _P, _P, _P, _I, _I, _P, _P],
    "vit_muon_gemm_grouped": [_P, _P, _I, _P, _I, _I, _P],
    "vit_muon_apply": [_P, _P, _P, _P, _P, _I, _I, _P, _I, _P],
}
MUON_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vit_amd_muon.h")
_RESTYPES = {"vit_last_error": C.c_char_p, "vit_last_gemm_kernel": C.c_char_p, "vit_workspace_needed": C.c_size_t}

_lib = None
_lock = threading.Lock()


def declared_symbols(header_path: str = HEADER_PATH):
    """Every function the C header declares, the headers it includes from its own directory (vit_amd_cov.h, vit_amd_optim.h, vit_amd_ema.h, vit_amd_droppath.h, vit_amd_layerscale.h, vit_amd_mix.h, vit_amd_patchdrop.h, vit_amd_mim.h, vit_amd_pool.h, vit_amd_sam.h, vit_amd_registers.h) included (used by
    the CPU test that checks the library exports them all)."""
    seen, names, todo = set(), set(), [os.path.abspath(header_path)]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        names.update(re.findall(r"\b(vit_[a-z0-9_]+)\s*\(", text))
        for inc in re.findall(r'#include\s+"([^"]+)"', text):
            sub = os.path.join(os.path.dirname(path), inc)
            if os.path.exists(sub):
                todo.append(sub)
    return sorted(names)


def declared_muon_symbols():
    """The functions vit_amd_muon.h itself declares (what vit_amd.h's closure declares is `declared_symbols()`'s)."""
    return sorted(set(declared_symbols(MUON_HEADER_PATH)) - set(declared_symbols()))


def load():
    """dlopen the library (after torch, so both share torch's HIP runtime) and set prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (must be first: see vit_amd/build.py)

        if not os.path.exists(LIB_PATH):
            raise VitError(
                f"{LIB_PATH} is missing: run `python -m vit_amd.build` (or __graft_entry__.build()). "
                "vit_amd has no fallback path; the HIP library is required.")
        lib = C.CDLL(LIB_PATH)
        for name, argtypes in {**_PROTOS, **_PROTOS_MUON}.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int)
        _lib = lib
        # VIT_OPTIONS="name=value,name=value": kernel-selection knobs of vit_set_option for A/B runs of unmodified scripts
        for item in filter(None, os.environ.get("VIT_OPTIONS", "").split(",")):
            name, _, value = item.partition("=")
            rc = lib.vit_set_option(name.strip().encode(), int(value))
            if rc != VIT_OK:
                raise VitError(f"VIT_OPTIONS: vit_set_option({name!r}, {value}) failed: {lib.vit_last_error().decode()}")
        return lib


def set_option(name: str, value: int):
    check(load().vit_set_option(name.encode(), int(value)), f"vit_set_option({name})")


def check(rc: int, what: str = ""):
    if rc != VIT_OK:
        msg = load().vit_last_error()
        raise VitError(f"{what or 'vit call'} failed (status {rc}): {msg.decode() if msg else ''}")


class Handle:
    """vit_handle + a torch-owned workspace on one device."""

    def __init__(self, device_index: int, workspace_bytes: int = 256 << 20):
        import torch

        self.lib = load()
        self.device_index = device_index
        h = C.c_void_p()
        check(self.lib.vit_create(C.byref(h), device_index), "vit_create")
        self.h = h
        self._ws = None
        self.set_workspace(workspace_bytes)

    def set_workspace(self, nbytes: int):
        import torch

        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=f"cuda:{self.device_index}")
        check(self.lib.vit_set_workspace(self.h, self._ws.data_ptr(), nbytes), "vit_set_workspace")
        self.workspace_bytes = nbytes

    def set_option(self, name: str, value: int):
        """Per-handle options (vit_handle_set_option): 'reserve_cus' (launch geometry of the calls made through THIS handle),
        'grad_accumulate' (parameter-gradient outputs store old + new), 'lamb_passes' (measurement only: which of LAMB's
        three launches a call makes)."""
        check(self.lib.vit_handle_set_option(self.h, name.encode(), int(value)), f"vit_handle_set_option({name})")

    def fill_workspace(self, byte: int):
        """Every byte of the workspace <- `byte`, on the current stream (tests: a call's result must not depend on what the
        workspace held before it)."""
        self._ws.fill_(int(byte) & 0xFF)

    def ensure_workspace(self, nbytes: int):
        if nbytes > self.workspace_bytes:
            self.set_workspace(int(nbytes * 1.25))

    def call(self, name: str, *args):
        """lib.<name>(handle, *args).  The library states what a call needs of the workspace: one that needs more has launched
        nothing (VIT_ERR_WORKSPACE), so the workspace grows to vit_workspace_needed() and the call is made once more."""
        fn = getattr(self.lib, name)
        rc = fn(self.h, *args)
        if rc == VIT_ERR_WORKSPACE:
            self.ensure_workspace(self.lib.vit_workspace_needed())
            rc = fn(self.h, *args)
        check(rc, name)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.vit_destroy(self.h)
                self.h = None
        except Exception:
            pass


_handles = {}


def handle_for(device) -> Handle:
    import torch

    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _handles:
        _handles[idx] = Handle(idx)
    return _handles[idx]
