"""ctypes binding of libvitlora_hip.so (C ABI: include/vitlora.h).

The library is the product path.  There is no CPU fallback: if the shared object is
missing or does not export every symbol of the header, importing callers fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VITLORA_LIB: another build of the same library (kernel A/B runs on one GPU box); never a fallback
LIB_PATH = os.environ.get("VITLORA_LIB") or os.path.join(_HERE, "libvitlora_hip.so")

VL_T = {"q": 1, "k": 2, "v": 4, "o": 8, "fc1": 16, "fc2": 32}
VL_PREC = {"f16": 0, "fp16": 0, "f32": 1, "fp32": 1, "bf16": 2}


class VLConfig(C.Structure):
    _fields_ = [
        ("image_size", C.c_int32), ("patch_size", C.c_int32), ("hidden", C.c_int32),
        ("layers", C.c_int32), ("heads", C.c_int32), ("mlp", C.c_int32),
        ("num_labels", C.c_int32), ("ln_eps", C.c_float),
        ("lora_r", C.c_int32), ("lora_alpha", C.c_float), ("lora_dropout", C.c_float),
        ("lora_targets", C.c_uint32), ("lora_merged", C.c_int32),
        ("precision", C.c_int32),          # VL_PREC_F16 = 0 (fp16 operands, fp32 accumulate), VL_PREC_F32 = 1 (parity mode), VL_PREC_BF16 = 2 (bf16 operands)
        ("reserved", C.c_int32 * 3),
    ]


# name -> (restype, argtypes); mirrors include/vitlora.h one to one
SIGNATURES = {
    "vl_version": (C.c_char_p, []),
    "vl_last_error": (C.c_char_p, []),
    "vl_create": (C.c_int, [C.POINTER(VLConfig), C.POINTER(C.c_void_p)]),
    "vl_destroy": (C.c_int, [C.c_void_p]),
    "vl_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "vl_param_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "vl_param_flat": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "vl_lora_commit": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vl_params_changed": (C.c_int, [C.c_void_p]),
    "vl_debug_counter": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "vl_merge_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "vl_set_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "vl_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vl_loss_ce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_set_dlogits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_set_normalization": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vl_channel_affine": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int64, C.c_void_p]),
    "vl_backward_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_backward_lora": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_pgd_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64, C.c_void_p]),
    "vl_pgd_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_int64, C.c_void_p]),
    "vl_pgd_attack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]),
    "vl_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int64, C.c_void_p]),
    "vl_quantize_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "vl_patch_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vl_patch_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vl_patch_apply_persp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vl_patch_grad_persp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vl_clamp": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int64, C.c_void_p]),
    "vl_set_dropout_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "vl_dropout_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vl_bench_gemm": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_float)]),
    "vl_check_gemm": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_float)]),
    "vl_debug_set_gemm_pp": (C.c_int, [C.c_int]),
    "vl_debug_set_gemm_stream": (C.c_int, [C.c_int]),
    "vl_debug_set_cus": (C.c_int, [C.c_void_p, C.c_int]),
    "vl_check_errors": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vl_swin_check_errors": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vl_debug_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "vl_profile_begin": (C.c_int, []),
    "vl_profile_report": (C.c_int, [C.c_char_p, C.c_size_t]),
    "vl_debug_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
}

class VLGemmCase(C.Structure):
    """vl_gemm_case of include/vitlora.h (field for field)."""
    _fields_ = [
        ("M", C.c_int32), ("N", C.c_int32), ("K1", C.c_int32), ("K2", C.c_int32),
        ("epi", C.c_int32), ("bn", C.c_int32), ("Mvalid", C.c_int32), ("n_store", C.c_int32), ("k2_used", C.c_int32),
        ("route", C.c_int32),
        ("A1", C.c_void_p), ("W1", C.c_void_p), ("A2", C.c_void_p), ("W2", C.c_void_p),
        ("lda1", C.c_int32), ("ldw1", C.c_int32), ("lda2", C.c_int32), ("ldw2", C.c_int32),
        ("bias", C.c_void_p), ("C", C.c_void_p), ("C2", C.c_void_p), ("R", C.c_void_p), ("G", C.c_void_p),
        ("ldc", C.c_int32), ("ldc2", C.c_int32), ("ldr", C.c_int32), ("ldg", C.c_int32),
        ("pos", C.c_void_p), ("row_scale", C.c_void_p),
        ("tokens", C.c_int32), ("patches", C.c_int32), ("grid", C.c_int32), ("psize", C.c_int32), ("img", C.c_int32),
        ("a_gather", C.c_int32), ("inv_std", C.c_float * 3),
        ("pgd_eps", C.c_float), ("pgd_alpha", C.c_float), ("pgd_lo", C.c_float), ("pgd_hi", C.c_float),
        ("drop_p", C.c_float), ("drop_stream", C.c_uint32), ("drop_seed", C.c_uint64),
        ("down_W", C.c_void_p), ("down_out", C.c_void_p),
        ("down_ldw", C.c_int32), ("down_ld", C.c_int32), ("down_groups", C.c_int32), ("ones_col", C.c_int32),
        ("f32_big", C.c_int32), ("transA", C.c_int32), ("transW", C.c_int32), ("Mstore", C.c_int32),
        ("alpha", C.c_float), ("reserved", C.c_int32 * 3),
    ]


SIGNATURES["vl_debug_gemm"] = (C.c_int, [C.c_void_p, C.POINTER(VLGemmCase), C.c_void_p])


class VLAttnCase(C.Structure):
    """vl_attn_case of include/vitlora.h (field for field)."""
    _fields_ = [
        ("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("kernel", C.c_int32),
        ("qkv", C.c_void_p), ("ctx", C.c_void_p), ("lse", C.c_void_p), ("dctx", C.c_void_p), ("dqkv", C.c_void_p),
        ("down_W", C.c_void_p), ("down_out", C.c_void_p),
        ("r", C.c_int32), ("mods", C.c_uint32), ("reserved", C.c_int32 * 4),
    ]


# vl_attn_case.kernel (the VL_ATTN_* values of include/vitlora.h)
ATTN_KERNELS = {"fwd": 0, "bwd": 1, "img_fwd": 2, "img_bwd": 3, "ring_bwd": 4, "cls_fwd": 5, "cls_bwd": 6,
                "f32_mfma_fwd": 7, "f32_mfma_bwd": 8, "f32_scalar_fwd": 9, "f32_scalar_bwd": 10}

SIGNATURES["vl_debug_attention"] = (C.c_int, [C.c_void_p, C.POINTER(VLAttnCase), C.c_void_p])


class VLApgdArgs(C.Structure):
    """vl_apgd_args of include/vitlora.h (field for field)."""
    _fields_ = [
        ("x0", C.c_void_p), ("labels", C.c_void_p), ("batch", C.c_int32), ("steps", C.c_int32),
        ("eps", C.c_float), ("rho", C.c_float), ("x_init", C.c_void_p),
        ("random_start", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64),
        ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
        ("x_best", C.c_void_p), ("x_best_adv", C.c_void_p), ("loss_best", C.c_void_p), ("robust", C.c_void_p),
        ("trace_loss", C.c_void_p), ("trace_step", C.c_void_p), ("trace_pred", C.c_void_p),
        ("stream", C.c_void_p), ("reserved", C.c_int32 * 4),
    ]


class VLApgdTrackCase(C.Structure):
    """vl_apgd_track_case of include/vitlora.h (field for field)."""
    _fields_ = [
        ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
        ("batch", C.c_int32), ("steps", C.c_int32), ("reset", C.c_int32), ("reserved0", C.c_int32),
        ("eps", C.c_float), ("rho", C.c_float),
        ("loss_img", C.c_void_p), ("logits", C.c_void_p), ("labels", C.c_void_p),
        ("step_out", C.c_void_p), ("flags_out", C.c_void_p), ("loss_best_out", C.c_void_p), ("robust_out", C.c_void_p),
    ]


SIGNATURES.update({
    "vl_apgd_scratch_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "vl_apgd_attack": (C.c_int, [C.c_void_p, C.POINTER(VLApgdArgs)]),
    "vl_apgd_step": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_void_p]),
    "vl_debug_apgd_track": (C.c_int, [C.c_void_p, C.POINTER(VLApgdTrackCase), C.c_void_p]),
})


class VLApgdtArgs(C.Structure):
    """vl_apgdt_args of include/vitlora.h (field for field)."""
    _fields_ = [
        ("x0", C.c_void_p), ("labels", C.c_void_p), ("batch", C.c_int32), ("steps", C.c_int32),
        ("eps", C.c_float), ("rho", C.c_float), ("n_target_classes", C.c_int32), ("n_restarts", C.c_int32),
        ("seed", C.c_uint64), ("targets_in", C.c_void_p),
        ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
        ("x_adv", C.c_void_p), ("robust", C.c_void_p), ("clean_correct", C.c_void_p), ("targets", C.c_void_p),
        ("fooled_by", C.c_void_p), ("loss_best", C.c_void_p), ("robust_run", C.c_void_p),
        ("trace_loss", C.c_void_p), ("trace_step", C.c_void_p), ("trace_pred", C.c_void_p),
        ("stream", C.c_void_p), ("reserved", C.c_int32 * 4),
    ]


SIGNATURES.update({
    "vl_apgdt_scratch_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "vl_apgdt_attack": (C.c_int, [C.c_void_p, C.POINTER(VLApgdtArgs)]),
    "vl_dlr_targeted_loss": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 4),
    "vl_apgd_targets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
})


class VLSquareArgs(C.Structure):
    """vl_square_args of include/vitlora.h (field for field)."""
    _fields_ = [
        ("x0", C.c_void_p), ("labels", C.c_void_p), ("batch", C.c_int32), ("n_queries", C.c_int32),
        ("first", C.c_int32), ("count", C.c_int32), ("eps", C.c_float), ("p_init", C.c_float),
        ("seed", C.c_uint64), ("image_offset", C.c_uint64),
        ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
        ("x_best", C.c_void_p), ("margin_min", C.c_void_p), ("queries", C.c_void_p), ("robust", C.c_void_p),
        ("trace_margin", C.c_void_p), ("trace_win", C.c_void_p),
        ("stream", C.c_void_p), ("reserved", C.c_int32 * 4),
    ]


class VLSquareTrackCase(C.Structure):
    """vl_square_track_case of include/vitlora.h (field for field)."""
    _fields_ = [
        ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
        ("batch", C.c_int32), ("n_queries", C.c_int32), ("reset", C.c_int32), ("reserved0", C.c_int32),
        ("p_init", C.c_float), ("reserved1", C.c_float), ("seed", C.c_uint64), ("image_offset", C.c_uint64),
        ("logits", C.c_void_p), ("labels", C.c_void_p),
        ("flags_out", C.c_void_p), ("win_prev_out", C.c_void_p), ("win_next_out", C.c_void_p),
        ("margin_min_out", C.c_void_p), ("queries_out", C.c_void_p),
    ]


SIGNATURES.update({
    "vl_square_scratch_bytes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "vl_square_attack": (C.c_int, [C.c_void_p, C.POINTER(VLSquareArgs)]),
    "vl_square_step": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "vl_debug_square_track": (C.c_int, [C.c_void_p, C.POINTER(VLSquareTrackCase), C.c_void_p]),
})


class VLSwinConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("patch_size", C.c_int32), ("embed_dim", C.c_int32), ("depths", C.c_int32 * 4),
                ("heads", C.c_int32 * 4), ("window", C.c_int32), ("num_labels", C.c_int32), ("ln_eps", C.c_float),
                ("lora_r", C.c_int32), ("lora_alpha", C.c_float), ("lora_targets", C.c_uint32), ("reserved", C.c_int32 * 4)]


SIGNATURES.update({
    "vl_swin_create": (C.c_int, [C.POINTER(VLSwinConfig), C.POINTER(C.c_void_p)]),
    "vl_swin_destroy": (C.c_int, [C.c_void_p]),
    "vl_swin_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "vl_swin_param_flat": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "vl_swin_param_tensor": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "vl_swin_set_normalization": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vl_swin_plan": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "vl_swin_set_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "vl_swin_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vl_swin_loss_ce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_swin_backward_input": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vl_swin_pgd_attack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_uint64,
                                     C.c_void_p, C.c_void_p]),
})

_lib = None


class VitLoraError(RuntimeError):
    code = 0


class NonFiniteGradient(VitLoraError):
    """VL_ERR_NONFINITE: the fp16 backward left its range (or produced NaN) in an earlier call."""
    code = -5


def load():
    """Load the shared library (once).  Raises if it is not built: `python __graft_entry__.py`
    or `<package>/csrc/build.sh` builds it with hipcc for gfx950."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VitLoraError(
            f"{LIB_PATH} is missing: the HIP extension is not built. There is no CPU fallback; "
            "run `python -c 'import __graft_entry__ as g; g.build()'` at the repo root.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().vl_last_error().decode("utf-8", "replace")
        exc = NonFiniteGradient if rc == -5 else VitLoraError
        e = exc(f"{what or 'vitlora call'} failed ({rc}): {msg}")
        e.code = rc
        raise e
