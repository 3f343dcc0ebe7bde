"""ctypes binding of the C ABI in include/sdmatte.h (libsdmatte_hip.so, hipcc/gfx950).

This is the only bridge between the Python host code (node, model-load API) and the hand-written HIP
kernels.  There is NO fallback: if the shared library is missing or no MI355X-class GPU is visible,
`load_library()` / `Engine()` raise.  PyTorch tensors are used only as device/host memory holders at the
node boundary (`tensor.data_ptr()`).
"""
import ctypes as C
import os

import numpy as np
import torch

from .config import SDMatteConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsdmatte_hip.so")

SDM_PTR_HOST, SDM_PTR_DEVICE = 0, 1
SDM_F32, SDM_F16, SDM_BF16 = 0, 1, 2
_DT = {torch.float32: SDM_F32, torch.float16: SDM_F16, torch.bfloat16: SDM_BF16}


class SdmConfig(C.Structure):
    _fields_ = [
        ("vae_channels", C.c_int32 * 4), ("vae_layers_per_block", C.c_int32),
        ("unet_channels", C.c_int32 * 4), ("unet_heads", C.c_int32 * 4), ("unet_layers_per_block", C.c_int32),
        ("cross_attention_dim", C.c_int32), ("unet_in_channels", C.c_int32), ("unet_out_channels", C.c_int32),
        ("bbox_embeddings_input_dim", C.c_int32), ("groups", C.c_int32),
        ("vae_eps", C.c_float), ("unet_res_eps", C.c_float), ("unet_tf_gn_eps", C.c_float), ("unet_ln_eps", C.c_float),
        ("vae_scaling_factor", C.c_float), ("attn_mask_value", C.c_float),
        ("stream_f32", C.c_int32), ("point_embeddings_input_dim", C.c_int32), ("precise_mask", C.c_int32), ("reserved", C.c_int32 * 5),
    ]


# sdm_precise_stage bits (include/sdmatte.h)
PRECISE_VAE_ENC, PRECISE_VAE_DEC, PRECISE_VAE_ATTN_LIN, PRECISE_UNET_RES, PRECISE_UNET_TF, PRECISE_UNET_ATTN = 1, 2, 4, 8, 16, 32
PRECISE_ALL = 63
PRECISIONS = {
    # fp16 MFMA operands everywhere: fastest; alpha within ~4e-3 of the reference's fp32 CPU path (the rounding floor of any
    # fp16-operand evaluation of this graph, the reference's own CUDA autocast path included)
    "fp16": 0,
    # split-fp16 operands (hi + lo, 3 MFMAs per product) and fp32 activations in every stage: alpha within 1e-3 (measured ~1e-4)
    "fp16x3": PRECISE_ALL,
}
DEFAULT_PRECISION = os.environ.get("SDMATTE_PRECISION", "fp16x3")


def precise_mask_of(precision) -> int:
    if precision is None:
        precision = DEFAULT_PRECISION
    if isinstance(precision, int):
        return precision & PRECISE_ALL
    if precision not in PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}; expected one of {sorted(PRECISIONS)} or a stage bit mask")
    return PRECISIONS[precision]


def to_c_config(cfg: SDMatteConfig, stream_f32: bool = True, precision=None) -> SdmConfig:
    c = SdmConfig()
    for i in range(4):
        c.vae_channels[i] = cfg.vae_channels[i]
        c.unet_channels[i] = cfg.unet_channels[i]
        c.unet_heads[i] = cfg.unet_heads[i]
    c.vae_layers_per_block = cfg.vae_layers_per_block
    c.unet_layers_per_block = cfg.unet_layers_per_block
    c.cross_attention_dim = cfg.cross_attention_dim
    c.unet_in_channels = cfg.unet_in_channels
    c.unet_out_channels = cfg.unet_out_channels
    c.bbox_embeddings_input_dim = cfg.bbox_embeddings_input_dim
    c.groups = cfg.unet_groups
    c.vae_eps, c.unet_res_eps = cfg.vae_eps, cfg.unet_res_eps
    c.unet_tf_gn_eps, c.unet_ln_eps = cfg.unet_tf_gn_eps, cfg.unet_ln_eps
    c.vae_scaling_factor, c.attn_mask_value = cfg.vae_scaling_factor, cfg.attn_mask_value
    c.stream_f32 = 1 if stream_f32 else 0
    c.point_embeddings_input_dim = cfg.point_embeddings_input_dim
    c.precise_mask = precise_mask_of(precision)
    return c


EXPORTS = [
    "sdm_default_config", "sdm_create", "sdm_destroy", "sdm_last_error", "sdm_load_tensor", "sdm_finalize_weights",
    "sdm_weight_stats", "sdm_missing_key", "sdm_weight_blob_bytes", "sdm_export_weight_blob", "sdm_import_weight_blob",
    "sdm_host_blob_bytes", "sdm_export_host_blob", "sdm_import_host_blob", "sdm_forward", "sdm_forward_ex", "sdm_forward_rect", "sdm_apply_matte", "sdm_apply_matte_node",
    "sdm_make_trimap", "sdm_clean_mask", "sdm_apply_matte_mask", "sdm_subject_roi", "sdm_apply_matte_roi", "sdm_subject_boxes", "sdm_apply_matte_boxes", "sdm_band_tiles", "sdm_apply_matte_tiles", "sdm_estimate_foreground", "sdm_refine_alpha_guided", "sdm_compose_canvas",
    "sdm_distance_field", "sdm_offset_mask", "sdm_outline", "sdm_smooth_alpha_temporal", "sdm_smooth_alpha_motion", "sdm_defocus_background", "sdm_fill_background", "sdm_harmonize", "sdm_screen_colour", "sdm_chroma_key", "sdm_matte_metrics",
    "sdm_synchronize", "sdm_release_memory", "sdm_resident_bytes", "sdm_weight_bytes", "sdm_last_forward_ms", "sdm_profile_enable", "sdm_profile_count", "sdm_profile_get", "sdm_profile_dump",
    "sdm_op_conv", "sdm_op_conv_ex", "sdm_op_conv_stats", "sdm_op_gn_partials", "sdm_op_gn_tables", "sdm_op_conv_up_stats", "sdm_op_gemm_p3", "sdm_debug_run_layer", "sdm_debug_set_input_cmask", "sdm_debug_temb_row", "sdm_conv_num_cfgs", "sdm_bench_conv", "sdm_bench_attn", "sdm_bench_gemm_p3", "sdm_op_groupnorm", "sdm_op_layernorm", "sdm_op_attention", "sdm_op_attention_ex", "sdm_op_attention_split", "sdm_op_attention_split_ex", "sdm_debug_attn_plan", "sdm_op_resize_aa",
    "sdm_op_mask_bias", "sdm_debug_patch_token_map", "sdm_op_groupnorm_p3", "sdm_op_gemm_p3_tokens", "sdm_op_mask_bias_tokens", "sdm_op_active_tiles",
    "sdm_op_cross_patch_planes", "sdm_op_cross_patch_planes_ex", "sdm_op_attention_shared", "sdm_debug_cross_attention", "sdm_op_cross_core",
    "sdm_set_option", "sdm_get_option", "sdm_reset_options", "sdm_option_name", "sdm_option_help", "sdm_kernel_counts", "sdm_kernel_counts_reset",
]


class Bindings:
    """Typed view of an already dlopen()ed engine library."""

    def __init__(self, cdll):
        self.dll = cdll
        vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
        sig = {
            "sdm_default_config": (None, [C.POINTER(SdmConfig)]),
            "sdm_create": (i32, [C.POINTER(vp), i32, C.POINTER(SdmConfig)]),
            "sdm_destroy": (None, [vp]),
            "sdm_last_error": (C.c_char_p, [vp]),
            "sdm_load_tensor": (i32, [vp, C.c_char_p, i32, i32, C.POINTER(i64), vp]),
            "sdm_finalize_weights": (i32, [vp]),
            "sdm_weight_stats": (i32, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
            "sdm_missing_key": (C.c_char_p, [vp, i64]),
            "sdm_weight_blob_bytes": (i64, [vp]),
            "sdm_export_weight_blob": (i32, [vp, vp]),
            "sdm_import_weight_blob": (i32, [vp, vp]),
            "sdm_host_blob_bytes": (i64, [vp]),
            "sdm_export_host_blob": (i32, [vp, vp]),
            "sdm_import_host_blob": (i32, [vp, vp]),
            "sdm_forward": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp]),
            "sdm_forward_ex": (i32, [vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, i32, vp]),
            "sdm_forward_rect": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, i32, vp]),
            "sdm_apply_matte": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp]),
            "sdm_apply_matte_node": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.c_double, vp, vp, i32, vp]),
            "sdm_make_trimap": (i32, [vp, vp, i32, i32, i32, f32, i32, i32, vp, i32, vp]),
            "sdm_clean_mask": (i32, [vp, vp, i32, i32, i32, f32, i32, i32, i32, i32, vp, vp, i32, vp]),
            "sdm_apply_matte_mask": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, i32, i32, i32, i32, C.c_double, vp, vp, vp, i32, vp]),
            "sdm_subject_roi": (i32, [vp, vp, i32, i32, i32, f32, i32, i32, i32, vp, i32, vp]),
            "sdm_apply_matte_roi": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, i32, i32, f32, i32, i32, i32, i32, i32, C.c_double, vp, vp, vp, vp, i32, vp]),
            "sdm_subject_boxes": (i32, [vp, vp, i32, i32, i32, f32, i32, i32, i32, i32, i32, vp, vp, i32, vp]),
            "sdm_apply_matte_boxes": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, i32, C.c_double, vp, vp, i32, vp]),
            "sdm_band_tiles": (i32, [vp, vp, i32, i32, i32, f32, f32, i32, i32, i32, vp, vp, i32, vp]),
            "sdm_apply_matte_tiles": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, i32, i32, C.c_double, vp, vp, i32, vp]),
            "sdm_estimate_foreground": (i32, [vp, vp, vp, i32, i32, i32, f32, f32, i32, i32, vp, i32, vp, i32, vp]),
            "sdm_refine_alpha_guided": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, i32, vp]),
            "sdm_compose_canvas": (i32, [vp, vp, vp, i32, i32, i32, f32, i32, i32, i32, i32, i32, vp, vp, i32, f32, f32, i32, i32, vp, i32, vp, i32, vp]),
            "sdm_distance_field": (i32, [vp, vp, i32, i32, i32, f32, vp, i32, vp]),
            "sdm_offset_mask": (i32, [vp, vp, i32, i32, i32, f32, f32, f32, vp, i32, vp]),
            "sdm_outline": (i32, [vp, vp, vp, i32, i32, i32, f32, i32, f32, f32, vp, f32, vp, vp, i32, vp]),
            "sdm_smooth_alpha_temporal": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, f32, vp, i32, vp]),
            "sdm_smooth_alpha_motion": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, f32, f32, vp, i32, vp]),
            "sdm_defocus_background": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, vp, i32, vp]),
            "sdm_fill_background": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, vp, i32, vp]),
            "sdm_harmonize": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp, i32, vp]),
            "sdm_screen_colour": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp]),
            "sdm_chroma_key": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, i32, i32, f32, vp, vp, vp, i32, vp]),
            "sdm_matte_metrics": (i32, [vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, vp, i32, vp]),
            "sdm_synchronize": (i32, [vp]),
            "sdm_release_memory": (i32, [vp]),
            "sdm_resident_bytes": (i64, [vp]),
            "sdm_weight_bytes": (i64, [vp]),
            "sdm_last_forward_ms": (f32, [vp]),
            "sdm_profile_enable": (i32, [vp, i32]),
            "sdm_profile_count": (i32, [vp]),
            "sdm_profile_dump": (C.c_char_p, [vp]),
            "sdm_profile_get": (i32, [vp, i32, C.POINTER(C.c_char_p), C.POINTER(f32), C.POINTER(i64), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double)]),
            "sdm_op_conv": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp, i32, i32,
                                  f32, i32]),
            "sdm_op_conv_ex": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp, i32, i32,
                                     f32, i32, i32, vp, vp, f32, i32, i32]),
            "sdm_op_conv_stats": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp, i32, i32,
                                        f32, i32, i32, vp, vp, f32, i32, i32, vp, i32, vp, i32, vp, i32, C.POINTER(i32)]),
            "sdm_op_gn_partials": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, f32, vp, vp]),
            "sdm_op_gn_tables": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, f32, vp, vp]),
            "sdm_op_gemm_p3": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, f32, i32, vp, vp, C.POINTER(i32)]),
            "sdm_op_conv_up_stats": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, C.POINTER(i32)]),
            "sdm_debug_run_layer": (i32, [vp, C.c_char_p, vp, i32, i32, i32, vp, i32]),
            "sdm_debug_set_input_cmask": (i32, [vp, vp]),
            "sdm_debug_temb_row": (i32, [vp, i32, i32, vp, vp, i32]),
            "sdm_conv_num_cfgs": (i32, [i32, i32]),
            "sdm_bench_conv": (f32, [vp] + [i32] * 11),
            "sdm_bench_attn": (f32, [vp] + [i32] * 7),
            "sdm_bench_gemm_p3": (f32, [vp, C.c_long, i32, i32, i32, i32]),
            "sdm_op_groupnorm": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, f32, i32, vp]),
            "sdm_op_layernorm": (i32, [vp, vp, i32, C.c_long, i32, vp, vp, f32, vp]),
            "sdm_op_attention": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp, i32]),
            "sdm_op_attention_ex": (i32, [vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32]),
            "sdm_op_attention_split": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
            "sdm_op_attention_split_ex": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
            "sdm_debug_attn_plan": (i32, [i32] * 10 + [C.c_char_p, i32, C.POINTER(i32)]),
            "sdm_op_resize_aa": (i32, [vp, vp, i32, i32, i32, vp, i32, i32]),
            "sdm_op_mask_bias": (i32, [vp, vp, i32, i32, i32, vp]),
            "sdm_debug_patch_token_map": (i32, [i32, i32, vp, vp]),
            "sdm_op_groupnorm_p3": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp]),
            "sdm_op_gemm_p3_tokens": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, C.POINTER(i32)]),
            "sdm_op_mask_bias_tokens": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
            "sdm_op_active_tiles": (i32, [vp, vp, i32, i32, vp]),
            "sdm_op_cross_patch_planes": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
            "sdm_op_cross_patch_planes_ex": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, i32]),
            "sdm_op_cross_core": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
            "sdm_op_attention_shared": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
            "sdm_debug_cross_attention": (i32, [vp, C.c_char_p, vp, i32, i32, i32, vp, i32, i32, vp]),
            "sdm_set_option": (i32, [C.c_char_p, i32]),
            "sdm_get_option": (i32, [C.c_char_p, C.POINTER(i32)]),
            "sdm_reset_options": (None, []),
            "sdm_option_name": (C.c_char_p, [i32]),
            "sdm_option_help": (C.c_char_p, [i32]),
            "sdm_kernel_counts": (i32, [C.c_char_p, i32]),
            "sdm_kernel_counts_reset": (None, []),
        }
        for name in EXPORTS:
            fn = getattr(cdll, name)          # AttributeError = missing export: fail loudly
            fn.restype, fn.argtypes = sig[name]
            setattr(self, name, fn)

    # ---- kernel-selection options (process-wide; tests and tools/ only - the library reads no environment variable) ----
    def set_option(self, name, value):
        if self.sdm_set_option(name.encode(), int(value)) != 0:
            raise KeyError(f"unknown engine option {name!r}; known: {', '.join(self.options())}")

    def get_option(self, name):
        v = C.c_int(0)
        if self.sdm_get_option(name.encode(), C.byref(v)) != 0:
            raise KeyError(name)
        return v.value

    def options(self):
        out, i = {}, 0
        while True:
            n = self.sdm_option_name(i)
            if n is None:
                return out
            out[n.decode()] = self.sdm_option_help(i).decode()
            i += 1

    def reset_options(self):
        self.sdm_reset_options()

    def attn_plan(self, B, heads, Lq, Lk, cus, D=64, prec=2, out_f32=True, has_bias=False, has_tiles=False):
        """(launch-counter name of the kernel, key split) the attention operator would take under the current options (sdm_debug_attn_plan)."""
        buf, ns = C.create_string_buffer(64), C.c_int(0)
        if self.sdm_debug_attn_plan(B, heads, Lq, Lk, D, prec, int(out_f32), int(has_bias), int(has_tiles), cus, buf, 64, C.byref(ns)) != 0:
            raise ValueError(f"sdm_debug_attn_plan: unsupported attention B={B} heads={heads} Lq={Lq} Lk={Lk} D={D} prec={prec}")
        return buf.value.decode(), ns.value

    def kernel_counts(self, reset=False):
        """{kernel variant: launches since the last reset}"""
        n = self.sdm_kernel_counts(None, 0)
        buf = C.create_string_buffer(n + 1)
        self.sdm_kernel_counts(buf, n + 1)
        out = {}
        for item in buf.value.decode().split(";"):
            if item:
                k, v = item.rsplit("=", 1)
                out[k] = int(v)
        if reset:
            self.sdm_kernel_counts_reset()
        return out


_PRODUCT = None


def load_library() -> Bindings:
    """dlopen the gfx950 engine.  Raises if it has not been built (`python -m ... build` / __graft_entry__.build())."""
    global _PRODUCT
    if _PRODUCT is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"SDMatte HIP engine not built: {LIB_PATH} is missing (run __graft_entry__.build()); "
                               "there is no CPU fallback")
        _PRODUCT = Bindings(C.CDLL(LIB_PATH))
    return _PRODUCT


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Engine:
    """One engine per GPU (one process per GPU under torch.distributed, or one per device inside ComfyUI)."""

    def __init__(self, cfg: SDMatteConfig = None, device: int = 0, stream_f32: bool = True, _lib: Bindings = None, precision=None):
        self.lib = _lib or load_library()
        self.cfg = cfg or SDMatteConfig.full()
        self.device = device
        self.precise_mask = precise_mask_of(precision)
        self._ccfg = to_c_config(self.cfg, stream_f32, self.precise_mask)
        h = C.c_void_p()
        rc = self.lib.sdm_create(C.byref(h), device, C.byref(self._ccfg))
        if rc != 0:
            raise RuntimeError(f"sdm_create failed ({rc}): {self.lib.sdm_last_error(None).decode()}")
        self.h = h
        self._on_device = _lib is None       # emulator builds (tests) address host memory

    def close(self):
        if getattr(self, "h", None):
            self.lib.sdm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.sdm_last_error(self.h).decode()}")
        return rc

    # ---- weights -------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = False):
        """Mirror of `load_state_dict(sd, strict=False)` (sdmatte_nodes.py:321): unknown keys are ignored,
        shape mismatches raise.  Returns (missing_keys, n_ignored)."""
        for k, t in state_dict.items():
            if not torch.is_tensor(t):
                continue
            t = t.detach()
            if t.device.type != "cpu":
                t = t.cpu()
            if t.dtype not in _DT:
                t = t.float()
            t = t.contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            self._check(self.lib.sdm_load_tensor(self.h, k.encode(), _DT[t.dtype], t.dim(), shape, _ptr(t)), f"load {k}")
        self._check(self.lib.sdm_finalize_weights(self.h), "finalize")
        nl, nm, ni = C.c_int64(), C.c_int64(), C.c_int64()
        self.lib.sdm_weight_stats(self.h, C.byref(nl), C.byref(nm), C.byref(ni))
        missing = [self.lib.sdm_missing_key(self.h, i).decode() for i in range(nm.value)]
        if strict and missing:
            raise RuntimeError(f"missing keys: {missing[:8]}...")
        return missing, ni.value

    def weight_blob_bytes(self):
        return int(self.lib.sdm_weight_blob_bytes(self.h))

    def export_weights(self, device_u8: torch.Tensor, host_u8: torch.Tensor):
        self._check(self.lib.sdm_export_weight_blob(self.h, _ptr(device_u8)), "export blob")
        self._check(self.lib.sdm_export_host_blob(self.h, _ptr(host_u8)), "export host blob")

    def import_weights(self, device_u8: torch.Tensor, host_u8: torch.Tensor):
        self._check(self.lib.sdm_import_weight_blob(self.h, _ptr(device_u8)), "import blob")
        self._check(self.lib.sdm_import_host_blob(self.h, _ptr(host_u8)), "import host blob")
        self._check(self.lib.sdm_finalize_weights(self.h), "finalize")

    def host_blob_bytes(self):
        return int(self.lib.sdm_host_blob_bytes(self.h))

    # ---- forward -------------------------------------------------------------------------------
    def _kind(self, t):
        return SDM_PTR_DEVICE if (t.device.type == "cuda") else (SDM_PTR_DEVICE if not self._on_device else SDM_PTR_HOST)

    def _check_io(self, what, *tensors):
        """All tensors of one call live in one place: host memory, or THIS engine's GPU (raw pointers cross the C ABI, so a
        tensor on another device would be read as garbage or fault).  Returns the hipStream_t the caller's work is queued on
        (torch's current stream of that device; the engine orders itself after it and makes it wait for the outputs)."""
        devs = {(t.device.type, t.device.index) for t in tensors if t is not None}
        if len(devs) != 1:
            raise ValueError(f"{what}: image, trimap and out must share one device, got {sorted(devs)}")
        (kind, idx), = devs
        if kind == "cuda":
            if not self._on_device or idx != self.device:
                raise ValueError(f"{what}: tensors live on cuda:{idx}, this engine drives cuda:{self.device}")
            return C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)
        if kind != "cpu":
            raise ValueError(f"{what}: unsupported device {kind}")
        return None

    def forward(self, image_b3ss: torch.Tensor, trimap_b1ss: torch.Tensor, is_trans=None, coords=None, out=None, sync=True,
                point_coords=None, use_attention_mask=True):
        """SDMatte.forward(data): image [B,3,S,S] in [-1,1], aux prompt image (trimap / bbox_mask / mask / point_mask) [B,1,S,S]
        in [-1,1] -> alpha [B,1,S,S].  `coords` [B,4] feed bbox_embedding (None -> [0,0,1,1]); `point_coords` [B,N] select the
        point prompt (point_embedding) instead; use_attention_mask=False drops the aux key mask of the self-attention."""
        B, _, SH, SW = image_b3ss.shape                    # square in the reference; rectangles are an extension (sdm_forward_rect)
        image_b3ss = image_b3ss.float().contiguous()
        trimap_b1ss = trimap_b1ss.float().contiguous()
        if out is None:
            out = torch.empty(B, 1, SH, SW, dtype=torch.float32, device=image_b3ss.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * SH * SW:
            raise ValueError("forward: out must be a contiguous fp32 tensor of B*SH*SW elements")
        stream = self._check_io("forward", image_b3ss, trimap_b1ss, out)
        it = np.ascontiguousarray(np.zeros(B, np.int32) if is_trans is None else np.asarray(is_trans, np.int32).reshape(B))
        if point_coords is not None:
            co = np.ascontiguousarray(np.asarray(point_coords, np.float32).reshape(B, -1))
            kind, dim = 1, co.shape[1]
        else:
            co = None if coords is None else np.ascontiguousarray(np.asarray(coords, np.float32).reshape(B, 4))
            kind, dim = 0, 4
        self._check(self.lib.sdm_forward_rect(self.h, _ptr(image_b3ss), _ptr(trimap_b1ss), B, SH, SW, it.ctypes.data_as(C.c_void_p),
                                              co.ctypes.data_as(C.c_void_p) if co is not None else None, dim, kind,
                                              1 if use_attention_mask else 0, _ptr(out), self._kind(image_b3ss), stream), "sdm_forward_rect")
        if sync:
            self.synchronize()
        return out

    def apply_matte(self, image_bhwc: torch.Tensor, trimap_bhw: torch.Tensor, S: int, is_transparent=False, out=None, sync=True):
        """Device part of SDMatteApply.apply_matte: raw image [B,H,W,3] + trimap [B,H,W] in [0,1] -> alpha [B,H,W]."""
        B, H, W, Cc = image_bhwc.shape
        if Cc != 3:
            raise ValueError(f"apply_matte: image must be [B,H,W,3], got {tuple(image_bhwc.shape)}")
        image_bhwc = image_bhwc.float().contiguous()
        trimap_bhw = trimap_bhw.float().contiguous()
        if tuple(trimap_bhw.shape) != (B, H, W):
            raise ValueError(f"apply_matte: trimap must be [B,H,W] = {(B, H, W)}, got {tuple(trimap_bhw.shape)}")
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.float32, device=image_bhwc.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * H * W:
            raise ValueError("apply_matte: out must be a contiguous fp32 tensor of B*H*W elements")
        stream = self._check_io("apply_matte", image_bhwc, trimap_bhw, out)
        self._check(self.lib.sdm_apply_matte(self.h, _ptr(image_bhwc), _ptr(trimap_bhw), B, H, W, int(S), 1 if is_transparent else 0,
                                             _ptr(out), self._kind(image_bhwc), stream), "sdm_apply_matte")
        if sync:
            self.synchronize()
        return out

    OUTPUT_MODES = {"alpha_only": 0, "matted_rgba": 1, "matted_rgb": 2}

    def apply_matte_node(self, image_bhwc, trimap_bhw, S, is_transparent, output_mode, mask_refine, trimap_constraint, sync=True):
        """The whole node body in one C-ABI call: preprocess, model, resize back, mask_refine and output composition, all on
        the GPU.  Returns (alpha [B,H,W], matted [B,H,W,3|4]) on the inputs' device."""
        if output_mode not in self.OUTPUT_MODES:
            raise ValueError(f"unknown output_mode {output_mode!r}")
        B, H, W, Cc = image_bhwc.shape
        if Cc != 3:
            raise ValueError(f"apply_matte_node: image must be [B,H,W,3], got {tuple(image_bhwc.shape)}")
        image_bhwc = image_bhwc.float().contiguous()
        trimap_bhw = trimap_bhw.float().contiguous()
        if trimap_bhw.dim() != 3 or trimap_bhw.shape[0] != B:
            raise ValueError(f"apply_matte_node: trimap must be [B,h,w] with B = {B}, got {tuple(trimap_bhw.shape)}")
        TH, TW = int(trimap_bhw.shape[1]), int(trimap_bhw.shape[2])
        mode = self.OUTPUT_MODES[output_mode]
        if (TH, TW) != (H, W) and (mask_refine or mode == 2):
            # where the reference fails too: it indexes the (H, W) alpha with the trimap (sdmatte_nodes.py:365-380,390-394)
            raise IndexError(f"apply_matte_node: the trimap {(TH, TW)} must match the image {(H, W)} for mask_refine / matted_rgb")
        alpha = torch.empty(B, H, W, dtype=torch.float32, device=image_bhwc.device)
        matted = torch.empty(B, H, W, 4 if mode == 1 else 3, dtype=torch.float32, device=image_bhwc.device)
        stream = self._check_io("apply_matte_node", image_bhwc, trimap_bhw, alpha, matted)
        self._check(self.lib.sdm_apply_matte_node(self.h, _ptr(image_bhwc), _ptr(trimap_bhw), B, H, W, TH, TW, int(S), 1 if is_transparent else 0, mode,
                                                  1 if mask_refine else 0, float(trimap_constraint), _ptr(alpha), _ptr(matted),
                                                  self._kind(image_bhwc), stream), "sdm_apply_matte_node")
        if sync:
            self.synchronize()
        return alpha, matted

    TRIMAP_MAX_RADIUS = 255      # SDM_TRIMAP_MAX_RADIUS (include/sdmatte.h)

    @classmethod
    def _check_radii(cls, what, erode_px, dilate_px):
        for name, r in (("erode_px", erode_px), ("dilate_px", dilate_px)):
            if int(r) != r or not 0 <= int(r) <= cls.TRIMAP_MAX_RADIUS:
                raise ValueError(f"{what}: {name} must be an integer in 0 .. {cls.TRIMAP_MAX_RADIUS}, got {r!r}")
        return int(erode_px), int(dilate_px)

    def make_trimap(self, mask, threshold=0.5, erode_px=10, dilate_px=10, out=None, sync=True):
        """Trimap from a mask on the GPU (sdm_make_trimap): mask [B,H,W] -> fp32 [B,H,W] of exactly 1.0 (mask > threshold, farther than
        erode_px from everything else), 0.0 (not, farther than dilate_px from the foreground) and 0.5.  Needs no loaded weights.
        `sdmatte_nodes.trimap_from_mask` is the same function on CPU tensors, bit for bit."""
        if mask.dim() != 3 or mask.numel() == 0:
            raise ValueError(f"make_trimap: mask must be a non-empty [B,H,W], got {tuple(mask.shape)}")
        erode_px, dilate_px = self._check_radii("make_trimap", erode_px, dilate_px)
        B, H, W = (int(v) for v in mask.shape)
        mask = mask.float().contiguous()
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.float32, device=mask.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * H * W:
            raise ValueError("make_trimap: out must be a contiguous fp32 tensor of B*H*W elements")
        stream = self._check_io("make_trimap", mask, out)
        self._check(self.lib.sdm_make_trimap(self.h, _ptr(mask), B, H, W, float(threshold), erode_px, dilate_px, _ptr(out), self._kind(mask), stream),
                    "sdm_make_trimap")
        if sync:
            self.synchronize()
        return out

    CLEAN_MAX_AREA = 1 << 28     # SDM_FG_MAX_PIXELS (include/sdmatte.h)

    def clean_mask(self, mask, threshold=0.5, min_area=64, keep_largest=False, max_hole_area=64, binarize=False, out=None, sync=True,
                   return_stats=False):
        """Mask clean-up on the GPU (sdm_clean_mask): mask [B,H,W] -> fp32 [B,H,W] without the 8-connected components of `mask > threshold` smaller than
        min_area (with keep_largest: without all but the largest one) and with the holes of at most max_hole_area pixels filled; removed pixels are 0.0,
        filled ones 1.0, every other pixel keeps its value (or becomes 1.0 / 0.0 with binarize).  return_stats: also int32 [B,4] = per image {components,
        components removed, holes filled, pixels changed}.  Needs no loaded weights.  `sdmatte_nodes.clean_mask` is the same function on CPU tensors,
        bit for bit."""
        if mask.dim() != 3 or mask.numel() == 0:
            raise ValueError(f"clean_mask: mask must be a non-empty [B,H,W], got {tuple(mask.shape)}")
        threshold = float(threshold)
        if not (0.0 <= threshold < 1.0) or float(np.float32(threshold)) >= 1.0:
            raise ValueError(f"clean_mask: threshold must be in [0, 1), got {threshold!r}")
        for name, v in (("min_area", min_area), ("max_hole_area", max_hole_area)):
            if int(v) != v or not 0 <= int(v) <= self.CLEAN_MAX_AREA:
                raise ValueError(f"clean_mask: {name} must be an integer in 0 .. {self.CLEAN_MAX_AREA}, got {v!r}")
        B, H, W = (int(v) for v in mask.shape)
        mask = mask.float().contiguous()
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.float32, device=mask.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * H * W:
            raise ValueError("clean_mask: out must be a contiguous fp32 tensor of B*H*W elements")
        stats = torch.empty(B, 4, dtype=torch.int32, device=mask.device) if return_stats else None
        stream = self._check_io("clean_mask", mask, out)
        self._check(self.lib.sdm_clean_mask(self.h, _ptr(mask), B, H, W, threshold, int(min_area), 1 if keep_largest else 0, int(max_hole_area),
                                            1 if binarize else 0, _ptr(out), _ptr(stats), self._kind(mask), stream), "sdm_clean_mask")
        if sync:
            self.synchronize()
        return (out, stats) if return_stats else out

    def apply_matte_mask(self, image_bhwc, mask_bhw, S, is_transparent, output_mode, mask_refine, trimap_constraint, threshold=0.5, erode_px=10,
                         dilate_px=10, sync=True):
        """`apply_matte_node` with the trimap made from `mask_bhw` on the GPU in the same C-ABI call (sdm_apply_matte_mask).  Returns
        (alpha [B,H,W], matted [B,H,W,3|4], trimap [B,h,w]); bit-identical to make_trimap followed by apply_matte_node."""
        if output_mode not in self.OUTPUT_MODES:
            raise ValueError(f"unknown output_mode {output_mode!r}")
        B, H, W, Cc = image_bhwc.shape
        if Cc != 3:
            raise ValueError(f"apply_matte_mask: image must be [B,H,W,3], got {tuple(image_bhwc.shape)}")
        erode_px, dilate_px = self._check_radii("apply_matte_mask", erode_px, dilate_px)
        image_bhwc = image_bhwc.float().contiguous()
        mask_bhw = mask_bhw.float().contiguous()
        if mask_bhw.dim() != 3 or mask_bhw.shape[0] != B:
            raise ValueError(f"apply_matte_mask: mask must be [B,h,w] with B = {B}, got {tuple(mask_bhw.shape)}")
        TH, TW = int(mask_bhw.shape[1]), int(mask_bhw.shape[2])
        mode = self.OUTPUT_MODES[output_mode]
        if (TH, TW) != (H, W) and (mask_refine or mode == 2):
            # the trimap has the mask's size, and apply_matte_node's rule holds for it
            raise IndexError(f"apply_matte_mask: the mask {(TH, TW)} must match the image {(H, W)} for mask_refine / matted_rgb")
        alpha = torch.empty(B, H, W, dtype=torch.float32, device=image_bhwc.device)
        matted = torch.empty(B, H, W, 4 if mode == 1 else 3, dtype=torch.float32, device=image_bhwc.device)
        trimap = torch.empty(B, TH, TW, dtype=torch.float32, device=image_bhwc.device)
        stream = self._check_io("apply_matte_mask", image_bhwc, mask_bhw, alpha, matted, trimap)
        self._check(self.lib.sdm_apply_matte_mask(self.h, _ptr(image_bhwc), _ptr(mask_bhw), B, H, W, TH, TW, int(S), 1 if is_transparent else 0,
                                                  float(threshold), erode_px, dilate_px, mode, 1 if mask_refine else 0, float(trimap_constraint),
                                                  _ptr(alpha), _ptr(matted), _ptr(trimap), self._kind(image_bhwc), stream), "sdm_apply_matte_mask")
        if sync:
            self.synchronize()
        return alpha, matted, trimap

    ROI_MAX_MARGIN_PX = 4096     # SDM_ROI_MAX_MARGIN_PX (include/sdmatte.h)

    @classmethod
    def _check_roi_params(cls, what, roi_threshold, margin_px, margin_pct):
        roi_threshold = float(roi_threshold)
        if not (0.0 <= roi_threshold < 1.0) or float(np.float32(roi_threshold)) >= 1.0:
            raise ValueError(f"{what}: roi_threshold must be in [0, 1), got {roi_threshold!r}")
        for name, v, hi in (("margin_px", margin_px, cls.ROI_MAX_MARGIN_PX), ("margin_pct", margin_pct, 100)):
            if int(v) != v or not 0 <= int(v) <= hi:
                raise ValueError(f"{what}: {name} must be an integer in 0 .. {hi}, got {v!r}")
        return roi_threshold, int(margin_px), int(margin_pct)

    def subject_roi(self, plane, roi_threshold=0.0, margin_px=16, margin_pct=10, square=True, out=None, sync=True):
        """The subject's box on the GPU (sdm_subject_roi): plane [B,H,W] (a trimap, a mask, an alpha) -> int32 [B,4] = per image {y0, x0, h, w}, the
        bounding box of `plane > roi_threshold` with a margin of margin_px + margin_pct % of its extent per side, clipped to the frame and, with `square`,
        grown to a square where the frame allows; the whole frame for an image without such a pixel.  Needs no loaded weights.
        `sdmatte_nodes.subject_roi` is the same function on CPU tensors, exactly."""
        if plane.dim() != 3 or plane.numel() == 0:
            raise ValueError(f"subject_roi: plane must be a non-empty [B,H,W], got {tuple(plane.shape)}")
        roi_threshold, margin_px, margin_pct = self._check_roi_params("subject_roi", roi_threshold, margin_px, margin_pct)
        B, H, W = (int(v) for v in plane.shape)
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"subject_roi: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        plane = plane.float().contiguous()
        if out is None:
            out = torch.empty(B, 4, dtype=torch.int32, device=plane.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (B, 4):
            raise ValueError("subject_roi: out must be a contiguous int32 tensor [B,4]")
        stream = self._check_io("subject_roi", plane, out)
        self._check(self.lib.sdm_subject_roi(self.h, _ptr(plane), B, H, W, roi_threshold, margin_px, margin_pct, 1 if square else 0, _ptr(out),
                                             self._kind(plane), stream), "sdm_subject_roi")
        if sync:
            self.synchronize()
        return out

    def apply_matte_roi(self, image_bhwc, aux_bhw, S, is_transparent, output_mode, mask_refine, trimap_constraint, aux_is_mask=False, threshold=0.5,
                        erode_px=10, dilate_px=10, roi_threshold=0.0, margin_px=16, margin_pct=10, square=True, sync=True):
        """`apply_matte_node` (or, with aux_is_mask, `apply_matte_mask`) on the subject instead of the frame, in one C-ABI call (sdm_apply_matte_roi): the
        model sees the box of the trimap (`subject_roi` with the four box arguments) at S x S, its alpha goes back into the box and is 0 outside,
        mask_refine and the composition run on the whole frame.  `aux_bhw` has the image's size.  Returns (alpha [B,H,W], matted [B,H,W,3|4],
        trimap [B,H,W] with aux_is_mask or None, roi int32 [B,4] = {y0, x0, h, w}); the box is never read by the host on the way."""
        if output_mode not in self.OUTPUT_MODES:
            raise ValueError(f"unknown output_mode {output_mode!r}")
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"apply_matte_roi: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        roi_threshold, margin_px, margin_pct = self._check_roi_params("apply_matte_roi", roi_threshold, margin_px, margin_pct)
        if aux_is_mask:
            erode_px, dilate_px = self._check_radii("apply_matte_roi", erode_px, dilate_px)
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"apply_matte_roi: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        if aux_bhw.dim() != 3 or aux_bhw.shape[0] != B:
            raise ValueError(f"apply_matte_roi: aux must be [B,H,W] with B = {B}, got {tuple(aux_bhw.shape)}")
        if tuple(aux_bhw.shape) != (B, H, W):
            # the box is a box of the image: there is no trimap of another size here
            raise IndexError(f"apply_matte_roi: aux {tuple(aux_bhw.shape[1:])} must match the image {(H, W)}")
        image_bhwc = image_bhwc.float().contiguous()
        aux_bhw = aux_bhw.float().contiguous()
        mode = self.OUTPUT_MODES[output_mode]
        dev = image_bhwc.device
        alpha = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        matted = torch.empty(B, H, W, 4 if mode == 1 else 3, dtype=torch.float32, device=dev)
        trimap = torch.empty(B, H, W, dtype=torch.float32, device=dev) if aux_is_mask else None
        roi = torch.empty(B, 4, dtype=torch.int32, device=dev)
        stream = self._check_io("apply_matte_roi", image_bhwc, aux_bhw, alpha, matted, trimap, roi)
        self._check(self.lib.sdm_apply_matte_roi(self.h, _ptr(image_bhwc), _ptr(aux_bhw), B, H, W, int(S), 1 if is_transparent else 0, 1 if aux_is_mask else 0,
                                                 float(threshold), int(erode_px), int(dilate_px), roi_threshold, margin_px, margin_pct, 1 if square else 0,
                                                 mode, 1 if mask_refine else 0, float(trimap_constraint), _ptr(alpha), _ptr(matted), _ptr(trimap), _ptr(roi),
                                                 self._kind(image_bhwc), stream), "sdm_apply_matte_roi")
        if sync:
            self.synchronize()
        return alpha, matted, trimap, roi

    BOXES_MAX = 8                # SDM_BOXES_MAX (include/sdmatte.h)
    BOXES_MAX_TOTAL = 16         # SDM_BOXES_MAX_TOTAL

    @classmethod
    def _check_boxes_params(cls, what, min_area, max_boxes):
        if int(min_area) != min_area or not 0 <= int(min_area) <= cls.CLEAN_MAX_AREA:
            raise ValueError(f"{what}: min_area must be an integer in 0 .. {cls.CLEAN_MAX_AREA}, got {min_area!r}")
        if int(max_boxes) != max_boxes or not 1 <= int(max_boxes) <= cls.BOXES_MAX:
            raise ValueError(f"{what}: max_boxes must be an integer in 1 .. {cls.BOXES_MAX}, got {max_boxes!r}")
        return int(min_area), int(max_boxes)

    def subject_boxes(self, plane, roi_threshold=0.0, min_area=64, max_boxes=4, margin_px=16, margin_pct=10, square=True, out=None, sync=True,
                      return_count=False):
        """A box per subject on the GPU (sdm_subject_boxes, defined in include/sdmatte.h): plane [B,H,W] -> int32 [B,max_boxes,5] = per image the entries
        {b, y0, x0, h, w}: the `subject_roi` boxes of the up to max_boxes - 1 largest 8-connected components of `plane > roi_threshold` with at least
        min_area pixels (one that lies inside an earlier box gets none), then the box of whatever these leave uncovered; the whole frame for an image
        without such a pixel; {-1, 0, 0, 0, 0} in every further entry.  return_count: also int32 [B], the entries per image.  Needs no loaded weights.
        `sdmatte_nodes.subject_boxes` is the same function on CPU tensors, exactly."""
        if plane.dim() != 3 or plane.numel() == 0:
            raise ValueError(f"subject_boxes: plane must be a non-empty [B,H,W], got {tuple(plane.shape)}")
        roi_threshold, margin_px, margin_pct = self._check_roi_params("subject_boxes", roi_threshold, margin_px, margin_pct)
        min_area, max_boxes = self._check_boxes_params("subject_boxes", min_area, max_boxes)
        B, H, W = (int(v) for v in plane.shape)
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"subject_boxes: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        plane = plane.float().contiguous()
        if out is None:
            out = torch.empty(B, max_boxes, 5, dtype=torch.int32, device=plane.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (B, max_boxes, 5):
            raise ValueError("subject_boxes: out must be a contiguous int32 tensor [B,max_boxes,5]")
        count = torch.empty(B, dtype=torch.int32, device=plane.device) if return_count else None
        stream = self._check_io("subject_boxes", plane, out, count)
        self._check(self.lib.sdm_subject_boxes(self.h, _ptr(plane), B, H, W, roi_threshold, min_area, max_boxes, margin_px, margin_pct, 1 if square else 0,
                                               _ptr(out), _ptr(count), self._kind(plane), stream), "sdm_subject_boxes")
        if sync:
            self.synchronize()
        return (out, count) if return_count else out

    def apply_matte_boxes(self, image_bhwc, trimap_bhw, boxes, S, is_transparent, output_mode, mask_refine, trimap_constraint, sync=True):
        """`apply_matte_node` over a list of boxes in one C-ABI call (sdm_apply_matte_boxes): boxes int32 [N,5] = {b, y0, x0, h, w}, N in 1 .. 16, on the
        device of the planes; the model runs with batch N, one box per slot at S x S, and each frame pixel gets the maximum of the boxes that contain it,
        0 outside all of them; mask_refine and the composition run on the whole frame.  An entry that does not lie inside its image is void (the void
        entries of `subject_boxes` are): it is skipped, but still costs a model pass - `sdmatte_nodes.compact_boxes` drops them on the host.  Returns
        (alpha [B,H,W], matted [B,H,W,3|4])."""
        if output_mode not in self.OUTPUT_MODES:
            raise ValueError(f"unknown output_mode {output_mode!r}")
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"apply_matte_boxes: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"apply_matte_boxes: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        if trimap_bhw.dim() != 3 or trimap_bhw.shape[0] != B:
            raise ValueError(f"apply_matte_boxes: trimap must be [B,H,W] with B = {B}, got {tuple(trimap_bhw.shape)}")
        if tuple(trimap_bhw.shape) != (B, H, W):
            # the boxes are boxes of the image: there is no trimap of another size here
            raise IndexError(f"apply_matte_boxes: trimap {tuple(trimap_bhw.shape[1:])} must match the image {(H, W)}")
        if boxes.dim() != 2 or boxes.shape[1] != 5 or boxes.dtype != torch.int32 or not 1 <= boxes.shape[0] <= self.BOXES_MAX_TOTAL:
            raise ValueError(f"apply_matte_boxes: boxes must be int32 [N,5] with N in 1 .. {self.BOXES_MAX_TOTAL}, got {boxes.dtype} {tuple(boxes.shape)}")
        image_bhwc = image_bhwc.float().contiguous()
        trimap_bhw = trimap_bhw.float().contiguous()
        boxes = boxes.contiguous()
        mode = self.OUTPUT_MODES[output_mode]
        dev = image_bhwc.device
        alpha = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        matted = torch.empty(B, H, W, 4 if mode == 1 else 3, dtype=torch.float32, device=dev)
        stream = self._check_io("apply_matte_boxes", image_bhwc, trimap_bhw, boxes, alpha, matted)
        self._check(self.lib.sdm_apply_matte_boxes(self.h, _ptr(image_bhwc), _ptr(trimap_bhw), B, H, W, int(S), 1 if is_transparent else 0, _ptr(boxes),
                                                   int(boxes.shape[0]), mode, 1 if mask_refine else 0, float(trimap_constraint), _ptr(alpha), _ptr(matted),
                                                   self._kind(image_bhwc), stream), "sdm_apply_matte_boxes")
        if sync:
            self.synchronize()
        return alpha, matted

    TILES_MAX = 16               # SDM_TILES_MAX (include/sdmatte.h)
    TILES_MAX_GRID = 256         # SDM_TILES_MAX_GRID
    TILES_MAX_FEATHER = 1024     # SDM_TILES_MAX_FEATHER

    @classmethod
    def _check_tiles_params(cls, what, band_lo, band_hi, tile, overlap, max_tiles):
        band_lo, band_hi = float(band_lo), float(band_hi)
        lo32, hi32 = float(np.float32(band_lo)), float(np.float32(band_hi))      # what the C ABI's floats will hold
        if not (0.0 <= band_lo < band_hi <= 1.0) or not (0.0 <= lo32 < hi32 <= 1.0):
            raise ValueError(f"{what}: band_lo and band_hi must satisfy 0 <= band_lo < band_hi <= 1, got {band_lo!r}, {band_hi!r}")
        if int(tile) != tile or not 16 <= int(tile) <= cls.FG_MAX_SIDE:
            raise ValueError(f"{what}: tile must be an integer in 16 .. {cls.FG_MAX_SIDE}, got {tile!r}")
        if int(overlap) != overlap or not 0 <= int(overlap) <= int(tile) // 2:
            raise ValueError(f"{what}: overlap must be an integer in 0 .. tile / 2 = {int(tile) // 2}, got {overlap!r}")
        if int(max_tiles) != max_tiles or not 1 <= int(max_tiles) <= cls.TILES_MAX:
            raise ValueError(f"{what}: max_tiles must be an integer in 1 .. {cls.TILES_MAX}, got {max_tiles!r}")
        return band_lo, band_hi, int(tile), int(overlap), int(max_tiles)

    @classmethod
    def _check_tiles_grid(cls, what, H, W, tile, overlap):
        ny, nx = (1 if L <= tile else -(-(L - overlap) // (tile - overlap)) for L in (H, W))
        if ny * nx > cls.TILES_MAX_GRID:
            raise ValueError(f"{what}: a grid of {ny} x {nx} cells is more than {cls.TILES_MAX_GRID} (tile = {tile} is too small for {(H, W)})")

    def band_tiles(self, trimap, band_lo=0.25, band_hi=0.75, tile=1024, overlap=128, max_tiles=16, out=None, sync=True, return_count=False):
        """The tiles of a frame that need the model, on the GPU (sdm_band_tiles, defined in include/sdmatte.h): trimap [B,H,W] -> int32 [B,max_tiles,5] =
        per image the entries {b, y0, x0, h, w} of the grid tiles (`tile` pixels a side, neighbours overlapping by at least `overlap`) that hold a pixel
        with band_lo < trimap < band_hi, in row-major grid order; {-1, 0, 0, 0, 0} in every further entry.  return_count: also int32 [B], the number of
        such tiles per image, also where it exceeds max_tiles.  Needs no loaded weights.  `sdmatte_nodes.band_tiles` is the same function on CPU
        tensors, exactly."""
        if trimap.dim() != 3 or trimap.numel() == 0:
            raise ValueError(f"band_tiles: trimap must be a non-empty [B,H,W], got {tuple(trimap.shape)}")
        band_lo, band_hi, tile, overlap, max_tiles = self._check_tiles_params("band_tiles", band_lo, band_hi, tile, overlap, max_tiles)
        B, H, W = (int(v) for v in trimap.shape)
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"band_tiles: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        self._check_tiles_grid("band_tiles", H, W, tile, overlap)
        trimap = trimap.float().contiguous()
        if out is None:
            out = torch.empty(B, max_tiles, 5, dtype=torch.int32, device=trimap.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (B, max_tiles, 5):
            raise ValueError("band_tiles: out must be a contiguous int32 tensor [B,max_tiles,5]")
        count = torch.empty(B, dtype=torch.int32, device=trimap.device) if return_count else None
        stream = self._check_io("band_tiles", trimap, out, count)
        self._check(self.lib.sdm_band_tiles(self.h, _ptr(trimap), B, H, W, band_lo, band_hi, tile, overlap, max_tiles, _ptr(out), _ptr(count),
                                            self._kind(trimap), stream), "sdm_band_tiles")
        if sync:
            self.synchronize()
        return (out, count) if return_count else out

    def apply_matte_tiles(self, image_bhwc, trimap_bhw, tiles, S, is_transparent, output_mode, mask_refine, trimap_constraint, feather_px=None, base=None,
                          sync=True):
        """`apply_matte_node` over a list of tiles in one C-ABI call (sdm_apply_matte_tiles): tiles int32 [N,5] = {b, y0, x0, h, w}, N in 0 .. 16, on the
        device of the planes; the model runs with batch N, one tile per slot at S x S, and each frame pixel gets the weighted mean of the tiles that contain
        it - weights that ramp over feather_px pixels (None = 0) towards a tile's edges inside the frame - or, outside all of them, `base` [B,H,W] (None:
        1 where trimap > 0.5, else 0); mask_refine and the composition run on the whole frame.  A void entry is skipped but costs a model pass
        (`sdmatte_nodes.compact_boxes` drops them on the host); N = 0 runs no model pass.  Returns (alpha [B,H,W], matted [B,H,W,3|4])."""
        if output_mode not in self.OUTPUT_MODES:
            raise ValueError(f"unknown output_mode {output_mode!r}")
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"apply_matte_tiles: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"apply_matte_tiles: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        if trimap_bhw.dim() != 3 or trimap_bhw.shape[0] != B:
            raise ValueError(f"apply_matte_tiles: trimap must be [B,H,W] with B = {B}, got {tuple(trimap_bhw.shape)}")
        if tuple(trimap_bhw.shape) != (B, H, W):
            # the tiles are tiles of the image: there is no trimap of another size here
            raise IndexError(f"apply_matte_tiles: trimap {tuple(trimap_bhw.shape[1:])} must match the image {(H, W)}")
        if tiles.dim() != 2 or tiles.shape[1] != 5 or tiles.dtype != torch.int32 or not 0 <= tiles.shape[0] <= self.TILES_MAX:
            raise ValueError(f"apply_matte_tiles: tiles must be int32 [N,5] with N in 0 .. {self.TILES_MAX}, got {tiles.dtype} {tuple(tiles.shape)}")
        feather_px = 0 if feather_px is None else feather_px
        if int(feather_px) != feather_px or not 0 <= int(feather_px) <= self.TILES_MAX_FEATHER:
            raise ValueError(f"apply_matte_tiles: feather_px must be an integer in 0 .. {self.TILES_MAX_FEATHER}, got {feather_px!r}")
        if base is not None and tuple(base.shape) != (B, H, W):
            raise ValueError(f"apply_matte_tiles: base must be [B,H,W] = {(B, H, W)}, got {tuple(base.shape)}")
        image_bhwc = image_bhwc.float().contiguous()
        trimap_bhw = trimap_bhw.float().contiguous()
        tiles = tiles.contiguous()
        base = base.float().contiguous() if base is not None else None
        mode = self.OUTPUT_MODES[output_mode]
        dev = image_bhwc.device
        alpha = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        matted = torch.empty(B, H, W, 4 if mode == 1 else 3, dtype=torch.float32, device=dev)
        N = int(tiles.shape[0])
        stream = self._check_io("apply_matte_tiles", image_bhwc, trimap_bhw, tiles, base, alpha, matted)
        self._check(self.lib.sdm_apply_matte_tiles(self.h, _ptr(image_bhwc), _ptr(trimap_bhw), B, H, W, int(S), 1 if is_transparent else 0,
                                                   _ptr(tiles) if N else None, N, int(feather_px), _ptr(base), mode, 1 if mask_refine else 0,
                                                   float(trimap_constraint), _ptr(alpha), _ptr(matted), self._kind(image_bhwc), stream),
                    "sdm_apply_matte_tiles")
        if sync:
            self.synchronize()
        return alpha, matted

    # SDM_FG_* (include/sdmatte.h)
    FG_DEFAULTS = {"regularization": 1e-5, "gradient_weight": 1.0, "n_small_iters": 10, "n_big_iters": 2}
    FG_MAX_SMALL_ITERS = 64
    FG_MAX_BIG_ITERS = 4
    FG_MAX_SIDE = 32768
    FG_MAX_PIXELS = 1 << 28

    @classmethod
    def _check_fg_params(cls, what, regularization, gradient_weight, n_small_iters, n_big_iters):
        import math
        regularization, gradient_weight = float(regularization), float(gradient_weight)
        if not (math.isfinite(regularization) and regularization > 0.0):
            raise ValueError(f"{what}: regularization must be a finite number above 0, got {regularization!r}")
        if not (math.isfinite(gradient_weight) and gradient_weight >= 0.0):
            raise ValueError(f"{what}: gradient_weight must be a finite number, 0 or above, got {gradient_weight!r}")
        for name, v, hi in (("n_small_iters", n_small_iters, cls.FG_MAX_SMALL_ITERS), ("n_big_iters", n_big_iters, cls.FG_MAX_BIG_ITERS)):
            if int(v) != v or not 1 <= int(v) <= hi:
                raise ValueError(f"{what}: {name} must be an integer in 1 .. {hi}, got {v!r}")
        return regularization, gradient_weight, int(n_small_iters), int(n_big_iters)

    def estimate_foreground(self, image_bhwc, alpha_bhw, regularization=1e-5, gradient_weight=1.0, n_small_iters=10, n_big_iters=2, rgba=False,
                            want_background=True, sync=True):
        """Foreground / background colours of every pixel from the image [B,H,W,3] and its alpha [B,H,W] on the GPU (sdm_estimate_foreground, the
        multi-level estimator defined in include/sdmatte.h).  Returns (fg [B,H,W,3], or [B,H,W,4] with the sanitised alpha as channel 3 when `rgba`;
        bg [B,H,W,3], or None without `want_background`).  Needs no loaded weights.  `sdmatte_nodes.estimate_foreground` is the same function on CPU
        tensors, equal to fp32 rounding."""
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"estimate_foreground: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if tuple(alpha_bhw.shape) != (B, H, W):
            raise ValueError(f"estimate_foreground: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha_bhw.shape)}")
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"estimate_foreground: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        regularization, gradient_weight, n_small_iters, n_big_iters = self._check_fg_params("estimate_foreground", regularization, gradient_weight,
                                                                                            n_small_iters, n_big_iters)
        image_bhwc = image_bhwc.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        ch = 4 if rgba else 3
        fg = torch.empty(B, H, W, ch, dtype=torch.float32, device=image_bhwc.device)
        bg = torch.empty(B, H, W, 3, dtype=torch.float32, device=image_bhwc.device) if want_background else None
        stream = self._check_io("estimate_foreground", image_bhwc, alpha_bhw, fg, bg)
        self._check(self.lib.sdm_estimate_foreground(self.h, _ptr(image_bhwc), _ptr(alpha_bhw), B, H, W, regularization, gradient_weight, n_small_iters,
                                                     n_big_iters, _ptr(fg), ch, _ptr(bg), self._kind(image_bhwc), stream),
                    "sdm_estimate_foreground")
        if sync:
            self.synchronize()
        return fg, bg

    # SDM_GF_* (include/sdmatte.h)
    GF_DEFAULTS = {"radius": 2, "eps": 1e-4}
    GF_MAX_SUBSAMPLE = 16
    GF_MAX_RADIUS = 32

    @classmethod
    def _check_gf_params(cls, what, subsample, radius, eps):
        import math
        for name, v, hi in (("subsample", subsample, cls.GF_MAX_SUBSAMPLE), ("radius", radius, cls.GF_MAX_RADIUS)):
            if int(v) != v or not 1 <= int(v) <= hi:
                raise ValueError(f"{what}: {name} must be an integer in 1 .. {hi}, got {v!r}")
        eps = C.c_float(float(eps)).value                                # the value that crosses the C ABI
        if not (math.isfinite(eps) and C.c_float(1e-6).value <= eps <= 1.0):
            raise ValueError(f"{what}: eps must be a finite number in [1e-6, 1], got {eps!r}")
        return int(subsample), int(radius), eps

    def refine_alpha_guided(self, image_bhwc, alpha_bhw, subsample, radius=2, eps=1e-4, sync=True):
        """The alpha [B,H,W] refined at the resolution of the image [B,H,W,3] on the GPU (sdm_refine_alpha_guided, the subsampled colour guided filter
        defined in include/sdmatte.h): `subsample` is the factor between the image and the resolution the alpha was made at
        (`sdmatte_nodes.auto_subsample`).  Returns fp32 [B,H,W] in [0,1] on the inputs' device.  Needs no loaded weights.
        `sdmatte_nodes.guided_refine_alpha` is the same function in torch, equal to fp32 rounding."""
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"refine_alpha_guided: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if tuple(alpha_bhw.shape) != (B, H, W):
            raise ValueError(f"refine_alpha_guided: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha_bhw.shape)}")
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"refine_alpha_guided: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        subsample, radius, eps = self._check_gf_params("refine_alpha_guided", subsample, radius, eps)
        image_bhwc = image_bhwc.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        out = torch.empty(B, H, W, dtype=torch.float32, device=image_bhwc.device)
        stream = self._check_io("refine_alpha_guided", image_bhwc, alpha_bhw, out)
        self._check(self.lib.sdm_refine_alpha_guided(self.h, _ptr(image_bhwc), _ptr(alpha_bhw), B, H, W, subsample, radius, eps, _ptr(out),
                                                     self._kind(image_bhwc), stream), "sdm_refine_alpha_guided")
        if sync:
            self.synchronize()
        return out

    # SDM_CANVAS_* (include/sdmatte.h)
    CANVAS_MAX_SHADOW_SIGMA = 32
    CANVAS_MAX_SHADOW_RADIUS = 96
    CANVAS_MAX_SHADOW_OFFSET = 4096
    CANVAS_VALIGN = {"top": 0, "center": 1, "bottom": 2}

    @classmethod
    def _check_canvas_params(cls, what, B, canvas_h, canvas_w, fill_pct, valign, shadow_opacity, shadow_sigma, shadow_dy, shadow_dx):
        """The argument limits of sdm_compose_canvas; returns the values that cross the C ABI (valign as 0 .. 2, the floats rounded to fp32)."""
        import math
        valign = cls.CANVAS_VALIGN.get(valign, valign)
        for name, v, lo, hi in (("canvas_h", canvas_h, 1, cls.FG_MAX_SIDE), ("canvas_w", canvas_w, 1, cls.FG_MAX_SIDE), ("fill_pct", fill_pct, 1, 100),
                                ("valign", valign, 0, 2), ("shadow_dy", shadow_dy, -cls.CANVAS_MAX_SHADOW_OFFSET, cls.CANVAS_MAX_SHADOW_OFFSET),
                                ("shadow_dx", shadow_dx, -cls.CANVAS_MAX_SHADOW_OFFSET, cls.CANVAS_MAX_SHADOW_OFFSET)):
            if isinstance(v, str) or int(v) != v or not lo <= int(v) <= hi:
                raise ValueError(f"{what}: {name} must be an integer in {lo} .. {hi}, got {v!r}")
        if B * int(canvas_h) * int(canvas_w) > cls.FG_MAX_PIXELS:
            raise ValueError(f"{what}: a canvas of {(B, int(canvas_h), int(canvas_w))} is too large ({cls.FG_MAX_PIXELS} pixels in all)")
        shadow_opacity, shadow_sigma = C.c_float(float(shadow_opacity)).value, C.c_float(float(shadow_sigma)).value
        if not (math.isfinite(shadow_opacity) and 0.0 <= shadow_opacity <= 1.0):
            raise ValueError(f"{what}: shadow_opacity must be a finite number in [0, 1], got {shadow_opacity!r}")
        if shadow_opacity > 0.0 and not (math.isfinite(shadow_sigma) and 0.0 < shadow_sigma <= cls.CANVAS_MAX_SHADOW_SIGMA):
            raise ValueError(f"{what}: shadow_sigma must be a finite number in (0, {cls.CANVAS_MAX_SHADOW_SIGMA}], got {shadow_sigma!r}")
        return int(canvas_h), int(canvas_w), int(fill_pct), int(valign), shadow_opacity, shadow_sigma, int(shadow_dy), int(shadow_dx)

    def compose_canvas(self, fg_bhw3, alpha_bhw, canvas_h, canvas_w, fill_pct=80, valign="center", bg_color=None, bg_image=None, shadow_opacity=0.0,
                       shadow_sigma=8.0, shadow_dy=0, shadow_dx=0, roi_threshold=0.0, out_channels=None, out=None, sync=True, return_placement=False):
        """The cut-out on a canvas on the GPU (sdm_compose_canvas, defined in include/sdmatte.h): the box of `alpha_bhw > roi_threshold` of the straight-alpha
        cut-out (fg [B,H,W,3], alpha [B,H,W]) is resampled premultiplied to fill `fill_pct` % of a canvas_h x canvas_w canvas (valign "top", "center",
        "bottom" or 0 .. 2), over `bg_image` ([1 or B,canvas_h,canvas_w,3]), else the colour `bg_color` (3 floats), else transparency, with a black shadow
        (opacity, Gaussian sigma, offset) between the two.  Returns fp32 [B,canvas_h,canvas_w,out_channels]: 3 channels = the composite (needs a background),
        4 = straight RGBA; the default is 3 with a background and 4 without.  return_placement: also int32 [B,8] = per image {y0, x0, h, w, dy0, dx0, dh, dw}.
        The box is never read by the host on the way.  Needs no loaded weights.  `sdmatte_nodes.compose_canvas` is the same function in torch, equal to fp32
        rounding; `sdmatte_nodes.canvas_fit` gives the same placements exactly."""
        if fg_bhw3.dim() != 4 or fg_bhw3.shape[-1] != 3 or fg_bhw3.numel() == 0:
            raise ValueError(f"compose_canvas: fg must be a non-empty [B,H,W,3], got {tuple(fg_bhw3.shape)}")
        B, H, W, _ = (int(v) for v in fg_bhw3.shape)
        if tuple(alpha_bhw.shape) != (B, H, W):
            raise ValueError(f"compose_canvas: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha_bhw.shape)}")
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"compose_canvas: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        roi_threshold, _, _ = self._check_roi_params("compose_canvas", roi_threshold, 0, 0)
        canvas_h, canvas_w, fill_pct, valign, shadow_opacity, shadow_sigma, shadow_dy, shadow_dx = self._check_canvas_params(
            "compose_canvas", B, canvas_h, canvas_w, fill_pct, valign, shadow_opacity, shadow_sigma, shadow_dy, shadow_dx)
        bg_mode = 2 if bg_image is not None else (1 if bg_color is not None else 0)
        if out_channels is None:
            out_channels = 3 if bg_mode else 4
        if out_channels not in (3, 4) or (bg_mode == 0 and out_channels != 4):
            raise ValueError(f"compose_canvas: out_channels must be 4, or 3 with a background, got {out_channels!r}")
        rgb, bg_batch = None, 0
        if bg_mode == 1:
            rgb = np.ascontiguousarray(np.asarray(bg_color, np.float32).reshape(-1))
            if rgb.shape != (3, ):
                raise ValueError(f"compose_canvas: bg_color must be 3 numbers, got {bg_color!r}")
        fg_bhw3 = fg_bhw3.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        if bg_mode == 2:
            if bg_image.dim() != 4 or tuple(bg_image.shape[1:]) != (canvas_h, canvas_w, 3) or int(bg_image.shape[0]) not in (1, B):
                raise ValueError(f"compose_canvas: bg_image must be [1 or {B},{canvas_h},{canvas_w},3], got {tuple(bg_image.shape)}")
            bg_image = bg_image.float().contiguous()
            bg_batch = int(bg_image.shape[0])
        dev = fg_bhw3.device
        if out is None:
            out = torch.empty(B, canvas_h, canvas_w, out_channels, dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, canvas_h, canvas_w, out_channels):
            raise ValueError(f"compose_canvas: out must be a contiguous fp32 tensor {(B, canvas_h, canvas_w, out_channels)}")
        place = torch.empty(B, 8, dtype=torch.int32, device=dev) if return_placement else None
        stream = self._check_io("compose_canvas", fg_bhw3, alpha_bhw, bg_image, out, place)
        self._check(self.lib.sdm_compose_canvas(self.h, _ptr(fg_bhw3), _ptr(alpha_bhw), B, H, W, roi_threshold, canvas_h, canvas_w, fill_pct, valign, bg_mode,
                                                rgb.ctypes.data_as(C.c_void_p) if rgb is not None else None, _ptr(bg_image), bg_batch, shadow_opacity,
                                                shadow_sigma, shadow_dy, shadow_dx, _ptr(out), out_channels, _ptr(place), self._kind(fg_bhw3), stream),
                    "sdm_compose_canvas")
        if sync:
            self.synchronize()
        return (out, place) if return_placement else out

    DF_NONE = 2147483647         # SDM_DF_NONE (include/sdmatte.h)
    DF_MAX_OFFSET = 1024         # SDM_DF_MAX_OFFSET
    DF_MAX_FEATHER = 1024        # SDM_DF_MAX_FEATHER
    OUTLINE_MAX_WIDTH = 1024     # SDM_OUTLINE_MAX_WIDTH
    OUTLINE_POSITION = {"outside": 0, "center": 1, "inside": 2}

    @classmethod
    def _check_df_plane(cls, what, plane, threshold):
        """The limits every distance-field call shares; returns (B, H, W, threshold as it crosses the C ABI)."""
        if plane.dim() != 3 or plane.numel() == 0:
            raise ValueError(f"{what}: the plane must be a non-empty [B,H,W], got {tuple(plane.shape)}")
        B, H, W = (int(v) for v in plane.shape)
        if max(H, W) > cls.FG_MAX_SIDE or B * H * W > cls.FG_MAX_PIXELS:
            raise ValueError(f"{what}: {(B, H, W)} is too large (sides up to {cls.FG_MAX_SIDE}, {cls.FG_MAX_PIXELS} pixels in all)")
        threshold = float(threshold)
        if not (0.0 <= threshold < 1.0) or float(np.float32(threshold)) >= 1.0:
            raise ValueError(f"{what}: threshold must be in [0, 1), got {threshold!r}")
        return B, H, W, threshold

    @staticmethod
    def _check_f32_range(what, name, v, lo, hi, lo_open=False):
        """A finite number in [lo, hi] (or (lo, hi]) after rounding to fp32, which is what the C ABI sees."""
        import math
        if isinstance(v, str):
            raise ValueError(f"{what}: {name} must be a number, got {v!r}")
        v = C.c_float(float(v)).value
        if not math.isfinite(v) or v > hi or v < lo or (lo_open and v <= lo):
            raise ValueError(f"{what}: {name} must be a finite number in {'(' if lo_open else '['}{lo}, {hi}], got {v!r}")
        return v

    def distance_field(self, plane, threshold=0.5, out=None, sync=True):
        """The exact Euclidean distance transform on the GPU (sdm_distance_field): plane [B,H,W] -> int32 [B,H,W], +d2 for the pixels of
        `plane > threshold` and -d2 for the others, d2 the squared distance to the nearest pixel of the other class of the same image (DF_NONE where
        there is none).  Needs no loaded weights.  `sdmatte_nodes.distance_field` is the same function on CPU tensors, exactly."""
        B, H, W, threshold = self._check_df_plane("distance_field", plane, threshold)
        plane = plane.float().contiguous()
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.int32, device=plane.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or out.numel() != B * H * W:
            raise ValueError("distance_field: out must be a contiguous int32 tensor of B*H*W elements")
        stream = self._check_io("distance_field", plane, out)
        self._check(self.lib.sdm_distance_field(self.h, _ptr(plane), B, H, W, threshold, _ptr(out), self._kind(plane), stream), "sdm_distance_field")
        if sync:
            self.synchronize()
        return out

    def offset_mask(self, mask, offset_px=0.0, feather_px=1.0, threshold=0.5, out=None, sync=True):
        """Grow (offset_px > 0), shrink (< 0) and feather a mask on the GPU (sdm_offset_mask): mask [B,H,W] -> fp32 [B,H,W] =
        clamp((offset_px - sd) / feather_px + 0.5, 0, 1) with sd the signed distance to the silhouette of `mask > threshold` (negative inside).
        (0, 1) gives the binarised mask; an integer offset r with feather 1 is exactly 1.0 on the dilation by the closed disk of radius r.  Needs no
        loaded weights.  `sdmatte_nodes.offset_mask` is the same function on CPU tensors."""
        B, H, W, threshold = self._check_df_plane("offset_mask", mask, threshold)
        offset_px = self._check_f32_range("offset_mask", "offset_px", offset_px, -self.DF_MAX_OFFSET, self.DF_MAX_OFFSET)
        feather_px = self._check_f32_range("offset_mask", "feather_px", feather_px, 1, self.DF_MAX_FEATHER)
        mask = mask.float().contiguous()
        if out is None:
            out = torch.empty(B, H, W, dtype=torch.float32, device=mask.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * H * W:
            raise ValueError("offset_mask: out must be a contiguous fp32 tensor of B*H*W elements")
        stream = self._check_io("offset_mask", mask, out)
        self._check(self.lib.sdm_offset_mask(self.h, _ptr(mask), B, H, W, threshold, offset_px, feather_px, _ptr(out), self._kind(mask), stream),
                    "sdm_offset_mask")
        if sync:
            self.synchronize()
        return out

    def outline(self, fg_bhw3, alpha_bhw, width_px=8.0, color=(1.0, 1.0, 1.0), position="outside", softness_px=1.0, opacity=1.0, edge_threshold=0.5,
                out=None, sync=True):
        """An outline along the silhouette of a straight-alpha cut-out on the GPU (sdm_outline, defined in include/sdmatte.h): fg [B,H,W,3], alpha
        [B,H,W] -> (rgb [B,H,W,3], alpha [B,H,W]), straight again.  The silhouette is that of `alpha > edge_threshold`; position "outside" (the stroke
        lies under the subject), "center" or "inside" (over it), or 0 .. 2.  `out` is an (rgb, alpha) pair.  Needs no loaded weights.
        `sdmatte_nodes.outline_cutout` is the same function in torch, equal to fp32 rounding."""
        if fg_bhw3.dim() != 4 or fg_bhw3.shape[-1] != 3 or fg_bhw3.numel() == 0:
            raise ValueError(f"outline: fg must be a non-empty [B,H,W,3], got {tuple(fg_bhw3.shape)}")
        if tuple(alpha_bhw.shape) != tuple(fg_bhw3.shape[:3]):
            raise ValueError(f"outline: alpha must be [B,H,W] = {tuple(fg_bhw3.shape[:3])}, got {tuple(alpha_bhw.shape)}")
        B, H, W, edge_threshold = self._check_df_plane("outline", alpha_bhw, edge_threshold)
        position = self.OUTLINE_POSITION.get(position, position)
        if isinstance(position, str) or int(position) != position or not 0 <= int(position) <= 2:
            raise ValueError(f"outline: position must be one of {sorted(self.OUTLINE_POSITION)} or 0 .. 2, got {position!r}")
        width_px = self._check_f32_range("outline", "width_px", width_px, 0, self.OUTLINE_MAX_WIDTH, lo_open=True)
        softness_px = self._check_f32_range("outline", "softness_px", softness_px, 1, self.DF_MAX_FEATHER)
        opacity = self._check_f32_range("outline", "opacity", opacity, 0, 1)
        rgb = np.ascontiguousarray(np.asarray(color, np.float32).reshape(-1))
        if rgb.shape != (3, ) or not np.isfinite(rgb).all():
            raise ValueError(f"outline: color must be 3 finite numbers, got {color!r}")
        fg_bhw3 = fg_bhw3.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        dev = fg_bhw3.device
        if out is None:
            out = (torch.empty(B, H, W, 3, dtype=torch.float32, device=dev), torch.empty(B, H, W, dtype=torch.float32, device=dev))
        out_rgb, out_alpha = out
        for t, shape in ((out_rgb, (B, H, W, 3)), (out_alpha, (B, H, W))):
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"outline: out must be a pair of contiguous fp32 tensors {(B, H, W, 3)} and {(B, H, W)}")
        stream = self._check_io("outline", fg_bhw3, alpha_bhw, out_rgb, out_alpha)
        self._check(self.lib.sdm_outline(self.h, _ptr(fg_bhw3), _ptr(alpha_bhw), B, H, W, edge_threshold, int(position), width_px, softness_px,
                                         rgb.ctypes.data_as(C.c_void_p), opacity, _ptr(out_rgb), _ptr(out_alpha), self._kind(fg_bhw3), stream),
                    "sdm_outline")
        if sync:
            self.synchronize()
        return out_rgb, out_alpha

    # SDM_TS_* (include/sdmatte.h)
    TS_DEFAULTS = {"radius": 2, "patch": 1, "color_tolerance": 0.1, "strength": 1.0, "max_change": 1.0, "clip_len": 0}
    TS_MAX_RADIUS = 4
    TS_MAX_PATCH = 2

    @classmethod
    def _check_ts_params(cls, what, B, radius, patch, color_tolerance, strength, max_change, clip_len):
        """The argument limits of sdm_smooth_alpha_temporal; returns the values that cross the C ABI (the floats rounded to fp32)."""
        for name, v, lo, hi in (("radius", radius, 1, cls.TS_MAX_RADIUS), ("patch", patch, 0, cls.TS_MAX_PATCH), ("clip_len", clip_len, 0, B)):
            if isinstance(v, str) or int(v) != v or not lo <= int(v) <= hi:
                raise ValueError(f"{what}: {name} must be an integer in {lo} .. {hi}, got {v!r}")
        color_tolerance = cls._check_f32_range(what, "color_tolerance", color_tolerance, 1.0 / 1024.0, 1)
        strength = cls._check_f32_range(what, "strength", strength, 0, 1)
        max_change = cls._check_f32_range(what, "max_change", max_change, 0, 1)
        return int(radius), int(patch), color_tolerance, strength, max_change, int(clip_len)

    def smooth_alpha_temporal(self, image_bhwc, alpha_bhw, radius=2, patch=1, color_tolerance=0.1, strength=1.0, max_change=1.0, clip_len=0, sync=True):
        """The alpha [B,H,W] of B consecutive frames [B,H,W,3] filtered along time on the GPU (sdm_smooth_alpha_temporal, defined in include/sdmatte.h):
        a frame within `radius` contributes to a pixel as far as the `patch` neighbourhood of that pixel did not change between the two frames
        (`color_tolerance`); where it did, the weight is exactly 0.  `clip_len` > 0 cuts the batch into independent clips of that many frames.  Returns fp32
        [B,H,W] in [0,1] on the inputs' device.  One kernel launch.  Needs no loaded weights.  `sdmatte_nodes.temporal_smooth_alpha` is the same function
        in torch, equal to fp32 rounding."""
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"smooth_alpha_temporal: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if tuple(alpha_bhw.shape) != (B, H, W):
            raise ValueError(f"smooth_alpha_temporal: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha_bhw.shape)}")
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"smooth_alpha_temporal: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        radius, patch, color_tolerance, strength, max_change, clip_len = self._check_ts_params(
            "smooth_alpha_temporal", B, radius, patch, color_tolerance, strength, max_change, clip_len)
        image_bhwc = image_bhwc.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        out = torch.empty(B, H, W, dtype=torch.float32, device=image_bhwc.device)
        stream = self._check_io("smooth_alpha_temporal", image_bhwc, alpha_bhw, out)
        self._check(self.lib.sdm_smooth_alpha_temporal(self.h, _ptr(image_bhwc), _ptr(alpha_bhw), B, H, W, clip_len, radius, patch, color_tolerance,
                                                       strength, max_change, _ptr(out), self._kind(image_bhwc), stream), "sdm_smooth_alpha_temporal")
        if sync:
            self.synchronize()
        return out

    # SDM_TSM_* (include/sdmatte.h)
    TSM_DEFAULTS = dict(TS_DEFAULTS, search=4, motion_penalty=0.02)
    TSM_MAX_SEARCH = 8

    @classmethod
    def _check_tsm_params(cls, what, B, radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len):
        """The argument limits of sdm_smooth_alpha_motion; returns the values that cross the C ABI (the floats rounded to fp32)."""
        if isinstance(search, str) or int(search) != search or not 0 <= int(search) <= cls.TSM_MAX_SEARCH:
            raise ValueError(f"{what}: search must be an integer in 0 .. {cls.TSM_MAX_SEARCH}, got {search!r}")
        radius, patch, color_tolerance, strength, max_change, clip_len = cls._check_ts_params(what, B, radius, patch, color_tolerance, strength, max_change,
                                                                                              clip_len)
        motion_penalty = cls._check_f32_range(what, "motion_penalty", motion_penalty, 0, 1) if int(search) else 0.0
        return radius, patch, int(search), color_tolerance, motion_penalty, strength, max_change, clip_len

    def smooth_alpha_motion(self, image_bhwc, alpha_bhw, radius=2, patch=1, search=4, color_tolerance=0.1, motion_penalty=0.02, strength=1.0, max_change=1.0,
                            clip_len=0, sync=True):
        """`smooth_alpha_temporal` along the motion (sdm_smooth_alpha_motion, defined in include/sdmatte.h): every pixel looks for the patch around it in the
        neighbouring frame among the integer displacements within `search` (the cost is the patch distance plus `motion_penalty` * color_tolerance^2 per
        squared pixel of displacement) and is filtered with the alpha found there, so the soft edge of a moving subject is smoothed too.  search = 0 is
        `smooth_alpha_temporal`, bit for bit.  Returns fp32 [B,H,W] in [0,1] on the inputs' device.  One kernel launch.  Needs no loaded weights.
        `sdmatte_nodes.temporal_smooth_alpha_motion` is the same function in torch."""
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"smooth_alpha_motion: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if tuple(alpha_bhw.shape) != (B, H, W):
            raise ValueError(f"smooth_alpha_motion: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha_bhw.shape)}")
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"smooth_alpha_motion: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len = self._check_tsm_params(
            "smooth_alpha_motion", B, radius, patch, search, color_tolerance, motion_penalty, strength, max_change, clip_len)
        image_bhwc = image_bhwc.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        out = torch.empty(B, H, W, dtype=torch.float32, device=image_bhwc.device)
        stream = self._check_io("smooth_alpha_motion", image_bhwc, alpha_bhw, out)
        self._check(self.lib.sdm_smooth_alpha_motion(self.h, _ptr(image_bhwc), _ptr(alpha_bhw), B, H, W, clip_len, radius, patch, search, color_tolerance,
                                                     motion_penalty, strength, max_change, _ptr(out), self._kind(image_bhwc), stream),
                    "sdm_smooth_alpha_motion")
        if sync:
            self.synchronize()
        return out

    # SDM_DEFOCUS_* (include/sdmatte.h)
    DEFOCUS_DEFAULTS = {"radius_px": 16, "highlight_gain": 0.0, "highlight_threshold": 0.8}
    DEFOCUS_MAX_RADIUS = 64
    DEFOCUS_MAX_GAIN = 64

    @classmethod
    def _check_defocus_params(cls, what, radius_px, highlight_gain, highlight_threshold):
        """The argument limits of sdm_defocus_background; returns the values that cross the C ABI (the floats rounded to fp32)."""
        if isinstance(radius_px, str) or int(radius_px) != radius_px or not 1 <= int(radius_px) <= cls.DEFOCUS_MAX_RADIUS:
            raise ValueError(f"{what}: radius_px must be an integer in 1 .. {cls.DEFOCUS_MAX_RADIUS}, got {radius_px!r}")
        highlight_gain = cls._check_f32_range(what, "highlight_gain", highlight_gain, 0, cls.DEFOCUS_MAX_GAIN)
        highlight_threshold = cls._check_f32_range(what, "highlight_threshold", highlight_threshold, 0, 1)
        return int(radius_px), highlight_gain, highlight_threshold

    def defocus_background(self, image_bhwc, alpha_bhw, fg=None, bg=None, radius_px=16, highlight_gain=0.0, highlight_threshold=0.8, sync=True):
        """The subject over its own background out of focus (sdm_defocus_background, defined in include/sdmatte.h): the background colours (`bg` if given,
        else the image) are blurred by a disc of `radius_px` pixels with the weight 1 - alpha, so the blur is normalised and does not see the subject (no
        halo), highlights above `highlight_threshold` weigh `highlight_gain` times their excess more, and the foreground colours (`fg` if given, else the
        image) are composed over the result with the alpha.  `fg` and `bg` are the two planes of `estimate_foreground`.  Returns fp32 [B,H,W,3] on the
        inputs' device.  Two kernel launches.  Needs no loaded weights.  `sdmatte_nodes.defocus_background` is the same function in torch, equal to fp32
        rounding."""
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"defocus_background: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if tuple(alpha_bhw.shape) != (B, H, W):
            raise ValueError(f"defocus_background: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha_bhw.shape)}")
        for name, t in (("fg", fg), ("bg", bg)):
            if t is not None and tuple(t.shape) != (B, H, W, 3):
                raise ValueError(f"defocus_background: {name} must be [B,H,W,3] = {(B, H, W, 3)}, got {tuple(t.shape)}")
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"defocus_background: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        radius_px, highlight_gain, highlight_threshold = self._check_defocus_params("defocus_background", radius_px, highlight_gain, highlight_threshold)
        image_bhwc = image_bhwc.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        fg = fg.float().contiguous() if fg is not None else None
        bg = bg.float().contiguous() if bg is not None else None
        out = torch.empty(B, H, W, 3, dtype=torch.float32, device=image_bhwc.device)
        stream = self._check_io("defocus_background", image_bhwc, alpha_bhw, fg, bg, out)
        self._check(self.lib.sdm_defocus_background(self.h, _ptr(image_bhwc), _ptr(alpha_bhw), _ptr(fg), _ptr(bg), B, H, W, radius_px, highlight_gain,
                                                    highlight_threshold, _ptr(out), self._kind(image_bhwc), stream), "sdm_defocus_background")
        if sync:
            self.synchronize()
        return out

    # SDM_PLATE_* (include/sdmatte.h)
    PLATE_ALPHA_CUT = 0.0625
    PLATE_MIN_CUT = 2.0 ** -10

    @staticmethod
    def plate_launches(H, W):
        """(launches of plate_pull, plate_small, plate_push) of a fill_background call on H x W: the formula of include/sdmatte.h."""
        S = 0
        while max(-(-int(H) >> S), -(-int(W) >> S)) > 32:
            S += 1
        return (S + 2) // 3, 1, (S + 2) // 3

    def fill_background(self, image_bhwc, alpha_bhw, bg=None, hole=None, alpha_cut=PLATE_ALPHA_CUT, sync=True):
        """The photo without its subject (sdm_fill_background, defined in include/sdmatte.h): the background colours (`bg` if given, else the image)
        count with the weight clamp(1 - a / alpha_cut, 0, 1), a the alpha (or the larger of alpha and `hole`), and the rest is filled by push-pull:
        weighted averages down a pyramid, bilinear interpolation back up.  Pixels of weight 1 come back bit for bit, and the subject's colour never
        enters the plate.  `bg` is the background plane of `estimate_foreground`; with it alpha_cut = 1 is the natural value, without it the default
        1/16 keeps contaminated soft pixels out.  Returns fp32 [B,H,W,3] on the inputs' device.  `sum(plate_launches(H, W))` kernel launches.  Needs no
        loaded weights.  `sdmatte_nodes.clean_plate` is the same function in torch, equal to fp32 rounding."""
        if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3 or image_bhwc.numel() == 0:
            raise ValueError(f"fill_background: image must be a non-empty [B,H,W,3], got {tuple(image_bhwc.shape)}")
        B, H, W, _ = (int(v) for v in image_bhwc.shape)
        if tuple(alpha_bhw.shape) != (B, H, W):
            raise ValueError(f"fill_background: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha_bhw.shape)}")
        if bg is not None and tuple(bg.shape) != (B, H, W, 3):
            raise ValueError(f"fill_background: bg must be [B,H,W,3] = {(B, H, W, 3)}, got {tuple(bg.shape)}")
        if hole is not None and tuple(hole.shape) != (B, H, W):
            raise ValueError(f"fill_background: hole must be [B,H,W] = {(B, H, W)}, got {tuple(hole.shape)}")
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"fill_background: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        alpha_cut = self._check_f32_range("fill_background", "alpha_cut", alpha_cut, self.PLATE_MIN_CUT, 1)
        image_bhwc = image_bhwc.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        bg = bg.float().contiguous() if bg is not None else None
        hole = hole.float().contiguous() if hole is not None else None
        out = torch.empty(B, H, W, 3, dtype=torch.float32, device=image_bhwc.device)
        stream = self._check_io("fill_background", image_bhwc, alpha_bhw, bg, hole, out)
        self._check(self.lib.sdm_fill_background(self.h, _ptr(image_bhwc), _ptr(alpha_bhw), _ptr(bg), _ptr(hole), B, H, W, alpha_cut, _ptr(out),
                                                 self._kind(image_bhwc), stream), "sdm_fill_background")
        if sync:
            self.synchronize()
        return out

    # SDM_HZ_* (include/sdmatte.h)
    HARMONIZE_DEFAULTS = {"luma_strength": 0.6, "chroma_strength": 0.8, "contrast_strength": 0.5, "wrap_strength": 0.5, "wrap_sigma": 6.0}
    HARMONIZE_MAX_WRAP_SIGMA = 16

    @classmethod
    def _check_harmonize_params(cls, what, luma_strength, chroma_strength, contrast_strength, wrap_strength, wrap_sigma):
        """The argument limits of sdm_harmonize; returns the values that cross the C ABI (rounded to fp32).  wrap_sigma is not looked at without the
        wrap (it crosses as the default then)."""
        luma_strength = cls._check_f32_range(what, "luma_strength", luma_strength, 0, 1)
        chroma_strength = cls._check_f32_range(what, "chroma_strength", chroma_strength, 0, 1)
        contrast_strength = cls._check_f32_range(what, "contrast_strength", contrast_strength, 0, 1)
        wrap_strength = cls._check_f32_range(what, "wrap_strength", wrap_strength, 0, 1)
        if wrap_strength > 0:
            wrap_sigma = cls._check_f32_range(what, "wrap_sigma", wrap_sigma, 0, cls.HARMONIZE_MAX_WRAP_SIGMA, lo_open=True)
        else:
            wrap_sigma = cls.HARMONIZE_DEFAULTS["wrap_sigma"]
        return luma_strength, chroma_strength, contrast_strength, wrap_strength, wrap_sigma

    @staticmethod
    def _check_harmonize_shapes(what, fg, alpha, bg):
        if fg.dim() != 4 or fg.shape[-1] != 3 or fg.numel() == 0:
            raise ValueError(f"{what}: fg must be a non-empty [B,H,W,3], got {tuple(fg.shape)}")
        B, H, W, _ = (int(v) for v in fg.shape)
        if tuple(alpha.shape) != (B, H, W):
            raise ValueError(f"{what}: alpha must be [B,H,W] = {(B, H, W)}, got {tuple(alpha.shape)}")
        if bg.dim() != 4 or tuple(bg.shape[1:]) != (H, W, 3) or int(bg.shape[0]) not in (1, B):
            raise ValueError(f"{what}: bg must be [1 or {B},{H},{W},3], got {tuple(bg.shape)}")
        return B, H, W

    def harmonize(self, fg_bhw3, alpha_bhw, bg, luma_strength=0.6, chroma_strength=0.8, contrast_strength=0.5, wrap_strength=0.5, wrap_sigma=6.0,
                  return_fg=False, return_map=False, sync=True):
        """The cut-out in its new scene (sdm_harmonize, defined in include/sdmatte.h): the straight foreground colours `fg_bhw3` [B,H,W,3] are moved
        towards the colour statistics of the scene `bg` ([1 or B,H,W,3]) in opponent coordinates (mean by `luma_strength` / `chroma_strength`, spread by
        `contrast_strength` times them), the scene's visible light is wrapped over the subject's edge (a Gaussian of `wrap_sigma` pixels, `wrap_strength`),
        and the result is composed over the scene with the alpha.  Returns fp32 [B,H,W,3] on the inputs' device; with return_fg also the adjusted
        foreground colours [B,H,W,3], with return_map also the colour map [B,12] (M row-major, then t).  One to four kernel launches, by the stages that
        are on.  Needs no loaded weights.  `sdmatte_nodes.harmonize_cutout` / `harmonize_map` are the same function in torch, equal to fp32 rounding."""
        B, H, W = self._check_harmonize_shapes("harmonize", fg_bhw3, alpha_bhw, bg)
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"harmonize: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        params = self._check_harmonize_params("harmonize", luma_strength, chroma_strength, contrast_strength, wrap_strength, wrap_sigma)
        fg_bhw3 = fg_bhw3.float().contiguous()
        alpha_bhw = alpha_bhw.float().contiguous()
        bg = bg.float().contiguous()
        dev = fg_bhw3.device
        out = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        fg_out = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if return_fg else None
        map_out = torch.empty(B, 12, dtype=torch.float32, device=dev) if return_map else None
        stream = self._check_io("harmonize", fg_bhw3, alpha_bhw, bg, out)
        self._check(self.lib.sdm_harmonize(self.h, _ptr(fg_bhw3), _ptr(alpha_bhw), _ptr(bg), int(bg.shape[0]), B, H, W, *params, _ptr(out), _ptr(fg_out),
                                           _ptr(map_out), self._kind(fg_bhw3), stream), "sdm_harmonize")
        if sync:
            self.synchronize()
        res = (out, ) + ((fg_out, ) if return_fg else ()) + ((map_out, ) if return_map else ())
        return res[0] if len(res) == 1 else res

    # SDM_KEY_* (include/sdmatte.h)
    KEY_HINTS = {"any": 0, "green": 1, "blue": 2}
    KEY_DEFAULTS = {"clip_fg": 0.15, "clip_bg": 0.85, "sure_fg": 0.05, "sure_bg": 0.95, "erode_px": 10, "dilate_px": 10, "despill": 1.0}
    KEY_OUTPUTS = ("key", "trimap", "despilled")
    KEY_MIN_SUM, KEY_MIN_SAT, KEY_MIN_SEP, KEY_RUN = 0.15, 0.25, 1.0 / 64, 4096
    KEY_SCREEN_CUT = 0.25
    KEY_MAX_SLOTS = 65536

    @staticmethod
    def key_launches(want=KEY_OUTPUTS):
        """{launch name: count} of a chroma_key call that returns `want`: the counts of include/sdmatte.h."""
        return {"ck_key": 1, "trimap_cols": 1, "trimap_rows": 1, "ck_veto": 1} if "trimap" in want else {"ck_key": 1}

    SCREEN_COLOUR_LAUNCHES = {"ck_clear": 1, "ck_hist": 1, "ck_mode": 1, "ck_mean": 1, "ck_finalize": 1}

    @classmethod
    def _check_key_image(cls, what, image):
        if image.dim() != 4 or image.shape[-1] != 3 or image.numel() == 0:
            raise ValueError(f"{what}: image must be a non-empty [B,H,W,3], got {tuple(image.shape)}")
        B, H, W, _ = (int(v) for v in image.shape)
        if max(H, W) > cls.FG_MAX_SIDE or B * H * W > cls.FG_MAX_PIXELS:
            raise ValueError(f"{what}: {(B, H, W)} is too large (sides up to {cls.FG_MAX_SIDE}, {cls.FG_MAX_PIXELS} pixels in all)")
        return B, H, W

    @classmethod
    def _check_key_hint(cls, what, hint):
        if hint in cls.KEY_HINTS:
            return cls.KEY_HINTS[hint]
        if isinstance(hint, int) and not isinstance(hint, bool) and hint in cls.KEY_HINTS.values():
            return hint
        raise ValueError(f"{what}: hint must be one of {sorted(cls.KEY_HINTS)} (or 0, 1, 2), got {hint!r}")

    @classmethod
    def _check_key_params(cls, what, clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill):
        """The argument limits of sdm_chroma_key; returns the values that cross the C ABI (floats rounded to fp32)."""
        clip_fg = cls._check_f32_range(what, "clip_fg", clip_fg, 0, 1)
        if clip_fg >= 1:
            raise ValueError(f"{what}: clip_fg must be a finite number in [0, 1), got {clip_fg!r}")
        clip_bg = cls._check_f32_range(what, "clip_bg", clip_bg, clip_fg, 1, lo_open=True)
        sure_fg = cls._check_f32_range(what, "sure_fg", sure_fg, -1, 1)
        sure_bg = cls._check_f32_range(what, "sure_bg", sure_bg, sure_fg, 2)
        despill = cls._check_f32_range(what, "despill", despill, 0, 1)
        erode_px, dilate_px = cls._check_radii(what, erode_px, dilate_px)
        return clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill

    @classmethod
    def _check_key_want(cls, what, want):
        want = (want, ) if isinstance(want, str) else tuple(want)
        if not want or len(set(want)) != len(want) or any(w not in cls.KEY_OUTPUTS for w in want):
            raise ValueError(f"{what}: want must name one to three different outputs of {cls.KEY_OUTPUTS}, got {want!r}")
        return want

    @staticmethod
    def _check_key_screen(what, screen, B, H, W):
        """(screen as [B,3] or [B,H,W,3], is_plane): a colour per image ([B,3] or [B,1,1,3]) or a colour per pixel."""
        if screen.dim() == 2 and tuple(screen.shape) == (B, 3):
            return screen, 0
        if screen.dim() == 4 and tuple(screen.shape) == (B, 1, 1, 3):
            return screen.reshape(B, 3), 0
        if screen.dim() == 4 and tuple(screen.shape) == (B, H, W, 3):
            return screen, 1
        raise ValueError(f"{what}: screen must be [B,3], [B,1,1,3] or [B,H,W,3] with (B, H, W) = {(B, H, W)}, got {tuple(screen.shape)}")

    def screen_colour(self, image_bhwc, hint="green", share=False, return_info=False, sync=True):
        """The colour of the green or blue screen behind a subject (sdm_screen_colour, defined in include/sdmatte.h): the mode of a 64 x 64 histogram
        of the chromaticities of the saturated pixels (`hint`: "green", "blue" or "any"), then the mean colour of the pixels around the mode.  One screen
        per image, or one for the whole batch with `share` (a clip).  Returns fp32 [B,3] on the input's device; with return_info also int32 [B,4] =
        {eligible pixels, selected pixels, iu, iv} (no eligible pixel: colour 0 and {0, 0, -1, -1}).  Five kernel launches.  Needs no loaded weights.
        `sdmatte_nodes.screen_colour` is the same function in torch: the integers exactly, the colour to fp32 rounding."""
        B, H, W = self._check_key_image("screen_colour", image_bhwc)
        hint = self._check_key_hint("screen_colour", hint)
        if not share and B > self.KEY_MAX_SLOTS:
            raise ValueError(f"screen_colour: B = {B} is too large without share (at most {self.KEY_MAX_SLOTS} images, one histogram each)")
        image_bhwc = image_bhwc.float().contiguous()
        dev = image_bhwc.device
        screen = torch.empty(B, 3, dtype=torch.float32, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev) if return_info else None
        stream = self._check_io("screen_colour", image_bhwc, screen)
        self._check(self.lib.sdm_screen_colour(self.h, _ptr(image_bhwc), B, H, W, hint, 1 if share else 0, _ptr(screen), _ptr(info),
                                               self._kind(image_bhwc), stream), "sdm_screen_colour")
        if sync:
            self.synchronize()
        return (screen, info) if return_info else screen

    def chroma_key(self, image_bhwc, screen, clip_fg=0.15, clip_bg=0.85, sure_fg=0.05, sure_bg=0.95, erode_px=10, dilate_px=10, despill=1.0,
                   want=KEY_OUTPUTS, sync=True):
        """The colour-difference key of an image against its screen (sdm_chroma_key, defined in include/sdmatte.h).  `screen` is a colour per image
        ([B,3] or [B,1,1,3], from `screen_colour`) or a colour per pixel ([B,H,W,3], the plate of `fill_background`).  Outputs, those named in `want`
        in that order (one name: the tensor itself): "key" fp32 [B,H,W], 0 on the screen and 1 on the subject, linear between the clips; "trimap" fp32
        [B,H,W], the trimap of `make_trimap(key, 0.5, erode_px, dilate_px)` with every definite pixel whose own colour does not agree (`sure_fg`,
        `sure_bg`) set to 0.5; "despilled" fp32 [B,H,W,3], the image with the screen's excess taken out of its channel.  One kernel launch without the
        trimap, four with it.  Needs no loaded weights.  `sdmatte_nodes.chroma_key` is the same function in torch, bit for bit."""
        B, H, W = self._check_key_image("chroma_key", image_bhwc)
        screen, is_plane = self._check_key_screen("chroma_key", screen, B, H, W)
        params = self._check_key_params("chroma_key", clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill)
        want = self._check_key_want("chroma_key", want)
        image_bhwc = image_bhwc.float().contiguous()
        screen = screen.float().contiguous()
        dev = image_bhwc.device
        outs = {"key": torch.empty(B, H, W, dtype=torch.float32, device=dev) if "key" in want else None,
                "trimap": torch.empty(B, H, W, dtype=torch.float32, device=dev) if "trimap" in want else None,
                "despilled": torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if "despilled" in want else None}
        stream = self._check_io("chroma_key", image_bhwc, screen, *outs.values())
        self._check(self.lib.sdm_chroma_key(self.h, _ptr(image_bhwc), _ptr(screen), is_plane, B, H, W, *params, _ptr(outs["key"]), _ptr(outs["trimap"]),
                                            _ptr(outs["despilled"]), self._kind(image_bhwc), stream), "sdm_chroma_key")
        if sync:
            self.synchronize()
        res = tuple(outs[w] for w in want)
        return res[0] if len(res) == 1 else res

    def key_screen(self, image_bhwc, hint="green", share=False, screen_correction=True, screen_cut=KEY_SCREEN_CUT, clip_fg=0.15, clip_bg=0.85,
                   sure_fg=0.05, sure_bg=0.95, erode_px=10, dilate_px=10, despill=1.0, want=KEY_OUTPUTS, sync=True):
        """A green-screen shot in one call: `screen_colour`, then `chroma_key`.  With `screen_correction` (the "screen correction" pass of a keyer) a
        first key marks the subject, `fill_background(image, key, alpha_cut=screen_cut)` fills its hole with the screen around it, and the key is made
        again against the screen's colour at each pixel, so that uneven lighting and shadows on the screen key out.  Returns the outputs named in
        `want`, in that order, and then the screen: [B,3], or the plate [B,H,W,3] with screen_correction.  With device tensors the chain is queued
        without a host sync between the calls, and no tensor leaves the device."""
        self._check_key_image("key_screen", image_bhwc)
        params = self._check_key_params("key_screen", clip_fg, clip_bg, sure_fg, sure_bg, erode_px, dilate_px, despill)
        want = self._check_key_want("key_screen", want)
        screen_cut = self._check_f32_range("key_screen", "screen_cut", screen_cut, self.PLATE_MIN_CUT, 1)
        image_bhwc = image_bhwc.float().contiguous()
        chain_sync = image_bhwc.device.type != "cuda"       # host pointers are synchronous anyway
        screen = self.screen_colour(image_bhwc, hint, share, sync=chain_sync)
        if screen_correction:
            key = self.chroma_key(image_bhwc, screen, *params, want=("key", ), sync=chain_sync)
            screen = self.fill_background(image_bhwc, key, alpha_cut=screen_cut, sync=chain_sync)
        res = self.chroma_key(image_bhwc, screen, *params, want=want, sync=chain_sync)
        if sync:
            self.synchronize()
        return (res if isinstance(res, tuple) else (res, )) + (screen, )

    # SDM_MM_* (include/sdmatte.h)
    METRICS_GRAD_SIGMA = 1.4
    METRICS_KEYS = ("n", "sad", "mse", "grad", "conn", "max_abs", "sad_frame", "mse_frame")

    @staticmethod
    def metrics_from_raw(raw, hw):
        """The literature's units from the [B,8] raw sums of sdm_matte_metrics: SAD, Grad and Conn in thousands, the squared error as a mean (over the
        band for `mse`, 0 when the band is empty; over the `hw` pixels of the frame for `mse_frame`), n and max|e| as they are."""
        n = raw[:, 0]
        return {"n": n, "sad": raw[:, 1] / 1000.0, "mse": raw[:, 2] / torch.clamp(n, min=1.0), "grad": raw[:, 3] / 1000.0, "conn": raw[:, 4] / 1000.0,
                "max_abs": raw[:, 5], "sad_frame": raw[:, 6] / 1000.0, "mse_frame": raw[:, 7] / float(hw), "raw": raw}

    def matte_metrics(self, pred, gt, trimap=None, grad_sigma=1.4, conn=True, return_levels=False, sync=True):
        """Score a matte (sdm_matte_metrics, defined in include/sdmatte.h): SAD, MSE, Grad and Conn of `pred` against `gt` ([B,H,W] each) over the unknown
        band of `trimap` ([B,H,W], or None for the whole frame).  Returns a dict of fp64 tensors [B] on the inputs' device in the literature's units:
        `n` (pixels of the band), `sad`, `grad`, `conn` (sums / 1000), `mse` (squared error / max(n, 1)), `max_abs`, and over the whole frame `sad_frame`
        (/ 1000) and `mse_frame` (/ (H W)); `raw` holds the [B,8] sums as they cross the C ABI.  With return_levels (needs conn) `levels` is the int32
        [B,H,W] connectivity level map.  2 kernel launches without conn, 63 with it.  Needs no loaded weights.  `sdmatte_nodes.matte_metrics` is the
        same function in torch."""
        if pred.dim() != 3 or pred.numel() == 0:
            raise ValueError(f"matte_metrics: pred must be a non-empty [B,H,W], got {tuple(pred.shape)}")
        B, H, W = (int(v) for v in pred.shape)
        if tuple(gt.shape) != (B, H, W) or (trimap is not None and tuple(trimap.shape) != (B, H, W)):
            raise ValueError(f"matte_metrics: gt and trimap must be [B,H,W] = {(B, H, W)}, got {tuple(gt.shape)}"
                             + (f" and {tuple(trimap.shape)}" if trimap is not None else ""))
        if max(H, W) > self.FG_MAX_SIDE or B * H * W > self.FG_MAX_PIXELS:
            raise ValueError(f"matte_metrics: {(B, H, W)} is too large (sides up to {self.FG_MAX_SIDE}, {self.FG_MAX_PIXELS} pixels in all)")
        grad_sigma = self._check_f32_range("matte_metrics", "grad_sigma", grad_sigma, 0.25, 4.0)
        if return_levels and not conn:
            raise ValueError("matte_metrics: return_levels needs conn=True")
        pred = pred.float().contiguous()
        gt = gt.float().contiguous()
        trimap = trimap.float().contiguous() if trimap is not None else None
        raw = torch.empty(B, 8, dtype=torch.float64, device=pred.device)
        levels = torch.empty(B, H, W, dtype=torch.int32, device=pred.device) if return_levels else None
        stream = self._check_io("matte_metrics", pred, gt, trimap, raw, levels)
        self._check(self.lib.sdm_matte_metrics(self.h, _ptr(pred), _ptr(gt), _ptr(trimap), B, H, W, grad_sigma, 1 if conn else 0, _ptr(raw), _ptr(levels),
                                               self._kind(pred), stream), "sdm_matte_metrics")
        if sync:
            self.synchronize()
        res = self.metrics_from_raw(raw, H * W)
        if return_levels:
            res["levels"] = levels
        return res

    def synchronize(self):
        self._check(self.lib.sdm_synchronize(self.h), "sdm_synchronize")

    def last_forward_ms(self):
        return float(self.lib.sdm_last_forward_ms(self.h))

    def resident_bytes(self):
        """Device memory held by the engine (weights + activation arena + I/O staging), invisible to torch's allocator."""
        return int(self.lib.sdm_resident_bytes(self.h))

    def weight_bytes(self):
        """The weight part of resident_bytes(): canonical blob + derived kernel layouts (stays resident across release_memory())."""
        return int(self.lib.sdm_weight_bytes(self.h))

    def release_memory(self):
        """Free the activation arena and staging buffers (weights stay); the next call re-allocates what it needs."""
        self._check(self.lib.sdm_release_memory(self.h), "sdm_release_memory")

    def profile(self, on: bool):
        self.lib.sdm_profile_enable(self.h, 1 if on else 0)

    def profile_results(self):
        res = {}
        for i in range(self.lib.sdm_profile_count(self.h)):
            name, ms, n, fl, by = C.c_char_p(), C.c_float(), C.c_int64(), C.c_double(), C.c_double()
            self.lib.sdm_profile_get(self.h, i, C.byref(name), C.byref(ms), C.byref(n), C.byref(fl), C.byref(by))
            res[name.value.decode()] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}
        return res

    def profile_dump(self):
        return self.lib.sdm_profile_dump(self.h).decode()

    # ---- single operators (parity tests) ---------------------------------------------------------
    def op_conv(self, x0, w, bias=None, x1=None, stride=1, pad_mode=0, up=0, res=None, geglu=False, out_f32=False, out_scale=1.0,
                tile_cfg=-1, split=False, gn=None, cmask=None):
        """x0/x1: NHWC fp16|fp32 tensors; w: fp32 OIHW or [O,I]; returns NHWC.  split=True: split-fp16 operands (fp32 inputs);
        gn=(gamma, beta, eps, groups, silu): GroupNorm(+SiLU) of the input fused into the conv's operand staging.
        cmask (test hook): uint8 [N,H,W] class plane of x0 (0 = nothing known, 1..4 = pixels of one constant region class)."""
        N, H, W_, C0 = x0.shape
        C1 = x1.shape[-1] if x1 is not None else 0
        ntaps = 9 if (w.dim() == 4 and w.shape[-1] == 3) else 1
        O = w.shape[0]
        Ho, Wo = (H << up), (W_ << up)
        if stride == 2:
            Ho, Wo = Ho // 2, Wo // 2
        Creal = O // 2 if geglu else O
        Cst = (Creal + 3) // 4 * 4          # rows are stored with 4-channel vector stores
        out = torch.empty(N, Ho, Wo, Cst, dtype=torch.float32 if out_f32 else torch.float16, device=x0.device)
        w = w.float().contiguous()
        b = bias.float().contiguous() if bias is not None else None
        gam = gn[0].float().contiguous() if gn is not None else None
        bet = gn[1].float().contiguous() if gn is not None else None
        if cmask is not None:
            cmask = cmask.to(torch.uint8).contiguous()
            self._check(self.lib.sdm_debug_set_input_cmask(self.h, _ptr(cmask)), "sdm_debug_set_input_cmask")
        self._check(self.lib.sdm_op_conv_ex(self.h, _ptr(x0), _ptr(x1), C0, C1, int(x0.dtype == torch.float32), N, H, W_, up, stride,
                                            pad_mode, ntaps, _ptr(w), _ptr(b), O, _ptr(out), int(out_f32), _ptr(res),
                                            int(res is not None and res.dtype == torch.float32), int(geglu), float(out_scale), tile_cfg,
                                            int(split), _ptr(gam), _ptr(bet), float(gn[2]) if gn is not None else 0.0,
                                            int(gn[3]) if gn is not None else 32, int(gn[4]) if gn is not None else 0),
                    "sdm_op_conv_ex")
        return out[..., :Creal]

    def op_conv_stats(self, x0, w, bias=None, x1=None, stride=1, pad_mode=0, up=0, res=None, out_f32=False, out_scale=1.0, tile_cfg=-1, split=False,
                      gn=None, cmask=None, in_stats=None):
        """Test hook: op_conv that also returns the partial {sum, sumsq} rows the conv's epilogue writes for the next GroupNorm -> (out NHWC,
        stats [N,srows,Cst,2] with Cst = O rounded up to 4; channels >= O unspecified).  in_stats = (st0,) or (st0, st1), with gn: the fused GroupNorm's
        scale | shift table comes from these partial rows of the input(s) (gn_partials_scale_shift_kernel, the model's path), not from the stand-alone
        statistics kernel."""
        N, H, W_, C0 = x0.shape
        C1 = x1.shape[-1] if x1 is not None else 0
        ntaps = 9 if (w.dim() == 4 and w.shape[-1] == 3) else 1
        O = w.shape[0]
        Ho, Wo = (H << up), (W_ << up)
        if stride == 2:
            Ho, Wo = Ho // 2, Wo // 2
        Cst = (O + 3) // 4 * 4
        out = torch.empty(N, Ho, Wo, Cst, dtype=torch.float32 if out_f32 else torch.float16, device=x0.device)
        w = w.float().contiguous()
        b = bias.float().contiguous() if bias is not None else None
        gam = gn[0].float().contiguous() if gn is not None else None
        bet = gn[1].float().contiguous() if gn is not None else None
        st0 = in_stats[0].float().contiguous() if in_stats is not None else None
        st1 = in_stats[1].float().contiguous() if in_stats is not None and len(in_stats) > 1 else None
        # one row per 32 output pixels at most (the 4 x 32 tile on four wave rows, the 8 x 8 tile on two), tiles counted per dimension; the phase path's own bound
        cap = max(4 * ((Ho + 3) // 4) * ((Wo + 7) // 8), 4 * ((Ho * Wo + 63) // 64), 8 * (((H + 2) * (W_ + 2) + 63) // 64))
        stats = torch.zeros(N * cap * Cst * 2, dtype=torch.float32, device=x0.device)
        srows = C.c_int(0)
        if cmask is not None:
            cmask = cmask.to(torch.uint8).contiguous()
            self._check(self.lib.sdm_debug_set_input_cmask(self.h, _ptr(cmask)), "sdm_debug_set_input_cmask")
        self._check(self.lib.sdm_op_conv_stats(self.h, _ptr(x0), _ptr(x1), C0, C1, int(x0.dtype == torch.float32), N, H, W_, up, stride,
                                               pad_mode, ntaps, _ptr(w), _ptr(b), O, _ptr(out), int(out_f32), _ptr(res),
                                               int(res is not None and res.dtype == torch.float32), 0, float(out_scale), tile_cfg,
                                               int(split), _ptr(gam), _ptr(bet), float(gn[2]) if gn is not None else 0.0,
                                               int(gn[3]) if gn is not None else 32, int(gn[4]) if gn is not None else 0,
                                               _ptr(st0), st0.shape[1] if st0 is not None else 0, _ptr(st1), st1.shape[1] if st1 is not None else 0,
                                               _ptr(stats), cap, C.byref(srows)), "sdm_op_conv_stats")
        return out[..., :O], stats[:N * srows.value * Cst * 2].view(N, srows.value, Cst, 2)

    def op_gn_partials(self, st0, gamma, beta, eps, HW, groups=32, st1=None):
        """Test hook: the reducer of the fused GroupNorm statistics alone.  st0 [N,rows0,C0,2] (+ st1 [N,rows1,C1,2], the second concat source) partial rows
        of images of HW pixels -> (scale [N,C0+C1], shift [N,C0+C1])."""
        st0 = st0.float().contiguous()
        st1 = st1.float().contiguous() if st1 is not None else None
        N, rows0, C0, _ = st0.shape
        rows1, C1 = (st1.shape[1], st1.shape[2]) if st1 is not None else (0, 0)
        gamma, beta = gamma.float().contiguous(), beta.float().contiguous()
        scale = torch.empty(N, C0 + C1, dtype=torch.float32, device=st0.device)
        shift = torch.empty(N, C0 + C1, dtype=torch.float32, device=st0.device)
        self._check(self.lib.sdm_op_gn_partials(self.h, _ptr(st0), rows0, _ptr(st1), rows1, C0, C1, N, int(HW), groups, _ptr(gamma), _ptr(beta), float(eps),
                                                _ptr(scale), _ptr(shift)), "sdm_op_gn_partials")
        return scale, shift

    def op_gn_tables(self, x0, gamma, beta, eps, groups=32, x1=None):
        """Test hook: the stand-alone GroupNorm statistics alone (gn_stats_kernel + gn_finalize_kernel) on x0 [N,H,W,C0] (+ x1, the second concat source),
        fp32 or fp16 -> (scale [N,C0+C1], shift [N,C0+C1])."""
        x0 = x0.contiguous()
        x1 = x1.contiguous() if x1 is not None else None
        N, H, W_, C0 = x0.shape
        C1 = x1.shape[-1] if x1 is not None else 0
        gamma, beta = gamma.float().contiguous(), beta.float().contiguous()
        scale = torch.empty(N, C0 + C1, dtype=torch.float32, device=x0.device)
        shift = torch.empty(N, C0 + C1, dtype=torch.float32, device=x0.device)
        self._check(self.lib.sdm_op_gn_tables(self.h, _ptr(x0), _ptr(x1), C0, C1, int(x0.dtype == torch.float32), N, H * W_, groups, _ptr(gamma), _ptr(beta),
                                              float(eps), _ptr(scale), _ptr(shift)), "sdm_op_gn_tables")
        return scale, shift

    def op_conv_up_stats(self, x, w, bias=None):
        """Test hook: Upsample2D (nearest x2 + 3x3 conv, split precision) on x fp32 [N,H,W,C] with the consumer's GroupNorm statistics, as the model's
        up-sampling layers run it -> (out fp32 [N,2H,2W,O], stats [N,srows,O,2] partial {sum, sumsq} rows)."""
        N, H, W_, Cin = x.shape
        O = w.shape[0]
        x = x.float().contiguous(); w = w.float().contiguous()
        b = bias.float().contiguous() if bias is not None else None
        out = torch.empty(N, 2 * H, 2 * W_, O, dtype=torch.float32, device=x.device)
        srows_max = 8 * (((H + 2) * (W_ + 2) + 63) // 64) + 4 * ((H + 1) // 2) * ((W_ + 3) // 4)      # phase path; any 3x3 tile (conv_up_phase = 0)
        stats = torch.zeros(N * srows_max * O * 2, dtype=torch.float32, device=x.device)
        srows = C.c_int(0)
        self._check(self.lib.sdm_op_conv_up_stats(self.h, _ptr(x), N, H, W_, Cin, _ptr(w), _ptr(b), O, _ptr(out), _ptr(stats), C.byref(srows)),
                    "sdm_op_conv_up_stats")
        return out, stats[:N * srows.value * O * 2].view(N, srows.value, O, 2)

    def op_gemm_p3(self, x, w, bias=None, mode=0, res=None, ln=None, lo_cols=-1):
        """Test hook: the plane-fed GEMM (k_gemm.h) on x fp32 [N,H,W,K].  mode 0 fp32 (+res), 1 GEGLU, 3 planes (+res), 4 fp32 + statistics -> (out, stats[N,srows,O,2]),
        2 -> (hi fp16 [N,H,W,O], pair uint8 [N,H,W,O,2]); ln = (gamma, beta, eps): LayerNorm with plane output in front."""
        N, H, W_, K = x.shape
        O = w.shape[0]
        x = x.float().contiguous(); w = w.float().contiguous()
        b = bias.float().contiguous() if bias is not None else None
        r = res.float().contiguous() if res is not None else None
        gam = ln[0].float().contiguous() if ln is not None else None
        bet = ln[1].float().contiguous() if ln is not None else None
        Cst = O // 2 if mode == 1 else O
        if mode == 2:
            out = torch.zeros(2 * N * H * W_ * O, dtype=torch.float16, device=x.device)
        else:
            out = torch.empty(N, H, W_, Cst, dtype=torch.float32, device=x.device)
        srows_max = 2 * ((H * W_ + 63) // 64)
        stats = torch.zeros(N * srows_max * O * 2, dtype=torch.float32, device=x.device) if mode == 4 else None
        srows = C.c_int(0)
        self._check(self.lib.sdm_op_gemm_p3(self.h, _ptr(x), N, H, W_, K, _ptr(w), _ptr(b), O, mode, _ptr(r), _ptr(gam), _ptr(bet),
                                            float(ln[2]) if ln is not None else 0.0, lo_cols, _ptr(out), _ptr(stats), C.byref(srows)), "sdm_op_gemm_p3")
        if mode == 2:
            n = N * H * W_ * O
            return out[:n].view(N, H, W_, O), out[n:].view(torch.uint8).view(N, H, W_, O, 2)
        if mode == 4:
            return out, stats[:N * srows.value * O * 2].view(N, srows.value, O, 2)
        return out

    def debug_run_layer(self, name, x_nhwc, cout):
        """Test hook: one packed layer of the loaded model on an fp32 NHWC input -> fp32 NHWC [N,H,W,cout]."""
        N, H, W_, _ = x_nhwc.shape
        x = x_nhwc.float().contiguous()
        out = torch.empty(N, H, W_, cout, dtype=torch.float32, device=x.device)
        self._check(self.lib.sdm_debug_run_layer(self.h, name.encode(), _ptr(x), N, H, W_, _ptr(out), cout), "sdm_debug_run_layer")
        return out

    def debug_temb_row(self, index, is_trans, coords, cout):
        """Test hook: folded conv1 bias row of the index-th time-embedded ResBlock for one (is_trans, box) conditioning."""
        out = np.zeros(cout, np.float32)
        co = None if coords is None else np.ascontiguousarray(np.asarray(coords, np.float32).reshape(4))
        self._check(self.lib.sdm_debug_temb_row(self.h, index, int(is_trans), co.ctypes.data_as(C.c_void_p) if co is not None else None,
                                                out.ctypes.data_as(C.c_void_p), cout), "sdm_debug_temb_row")
        return torch.from_numpy(out)

    def bench_conv(self, N, H, W, Cin, Cout, ntaps=9, stride=1, in_f32=0, tile_cfg=-1, ablate=0, iters=10):
        return float(self.lib.sdm_bench_conv(self.h, N, H, W, Cin, Cout, ntaps, stride, in_f32, tile_cfg, ablate, iters))

    def bench_gemm_p3(self, M, K, O, epi=0, res=False, iters=10):
        return float(self.lib.sdm_bench_gemm_p3(self.h, M, K, O, epi | (256 if res else 0), iters))

    def bench_attn(self, B, heads, Lq, Lk, qt=1, ablate=0, iters=10):
        return float(self.lib.sdm_bench_attn(self.h, B, heads, Lq, Lk, qt, ablate, iters))

    def op_groupnorm(self, x0, gamma, beta, eps, silu, groups=32, x1=None):
        N, H, W_, C0 = x0.shape
        C1 = x1.shape[-1] if x1 is not None else 0
        out = torch.empty(N, H, W_, C0 + C1, dtype=torch.float16, device=x0.device)
        self._check(self.lib.sdm_op_groupnorm(self.h, _ptr(x0), _ptr(x1), C0, C1, int(x0.dtype == torch.float32), N, H * W_, groups,
                                              _ptr(gamma), _ptr(beta), float(eps), int(silu), _ptr(out)), "sdm_op_groupnorm")
        return out

    def op_layernorm(self, x, gamma, beta, eps):
        rows, Cc = x.numel() // x.shape[-1], x.shape[-1]
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
        self._check(self.lib.sdm_op_layernorm(self.h, _ptr(x), int(x.dtype == torch.float32), rows, Cc, _ptr(gamma), _ptr(beta),
                                              float(eps), _ptr(out)), "sdm_op_layernorm")
        return out

    def op_attention(self, q, k, v, heads, bias=None):
        """q [B,Lq,h*D], k/v [B,Lk,h*D] fp16 (may be views with a row stride); bias fp32 [B,Lk] or None."""
        B, Lq, HD = q.shape
        Lk = k.shape[1]
        D = HD // heads
        out = torch.empty(B, Lq, HD, dtype=torch.float16, device=q.device)
        self._check(self.lib.sdm_op_attention(self.h, _ptr(q), q.stride(1), _ptr(k), k.stride(1), _ptr(v), v.stride(1), _ptr(bias), B,
                                              heads, Lq, Lk, D, _ptr(out), HD), "sdm_op_attention")
        return out

    def op_attention_f32(self, q, k, v, heads):
        """op_attention without a bias and with an fp32 result (head dim 512: the core as the precise-mode VAE runs it)."""
        B, Lq, HD = q.shape
        Lk = k.shape[1]
        out = torch.empty(B, Lq, HD, dtype=torch.float32, device=q.device)
        self._check(self.lib.sdm_op_attention_ex(self.h, _ptr(q), q.stride(1), _ptr(k), k.stride(1), _ptr(v), v.stride(1), B, heads, Lq, Lk, HD // heads, 1,
                                                 _ptr(out), HD), "sdm_op_attention_ex")
        return out

    def op_attention_split(self, q, k, v, heads, bias=None, out_p3=0, tiles=None, planes=False):
        """Split-precision attention cores (head dim 64): q [B,Lq,h*64], k / v [B,Lk,h*64] fp32; the C side splits them into the operand
        planes the producing GEMM epilogues write in the engine (fp16 high parts + fp8 residual pairs for Q.K^T); fp32 output.
        Through sdm_op_attention_split_ex when one of these is given: tiles int32 [B, ceil(Lk/64) + 1] = count, then the ascending active
        64-key tiles of each image (needs the bias); out_p3 1 (True): the kernels write the P3 operand planes the engine's transformer blocks
        consume, 2: the fp32 result through to_p3_kernel - both decoded to fp32; planes=True (out_p3 != 0): also the raw plane bytes ->
        (out, uint8 [ceil(B*Lq/32)*32 * h*64 * 3])."""
        B, Lq, HD = q.shape
        Lk = k.shape[1]
        qf, kf, vf = q.float().contiguous(), k.float().contiguous(), v.float().contiguous()
        out = torch.empty(B, Lq, HD, dtype=torch.float32, device=q.device)
        if not out_p3 and tiles is None:
            self._check(self.lib.sdm_op_attention_split(self.h, _ptr(qf), _ptr(kf), _ptr(vf), _ptr(bias), B, heads, Lq, Lk, _ptr(out)), "sdm_op_attention_split")
            return out
        tl = tiles.to(torch.int32).contiguous() if tiles is not None else None
        raw = torch.zeros(((B * Lq + 31) // 32) * 32 * HD * 3, dtype=torch.uint8, device=q.device) if (planes and out_p3) else None
        self._check(self.lib.sdm_op_attention_split_ex(self.h, _ptr(qf), _ptr(kf), _ptr(vf), _ptr(bias), _ptr(tl), B, heads, Lq, Lk, int(out_p3),
                                                       _ptr(out), _ptr(raw)), "sdm_op_attention_split_ex")
        return (out, raw) if raw is not None else out

    def op_cross_patch_planes(self, uin, ones_rows=False):
        """Test hook: the shared cross-attention operand of a U-Net input tensor uin fp32 [B,H,W,16] (trimap latent at channels 4..7) ->
        (k_hi fp16 [B,H*W,64], k_pair uint8 [B,H*W,64,2], vt fp16 [B,64,ceil(H*W/64)*64]).  ones_rows: with 1.0 in vt rows 59 and 63 for the
        keys < H*W, as the engine builds it under the option cross_narrow."""
        B, H, W_, _ = uin.shape
        L = H * W_
        ldvt = (L + 63) // 64 * 64
        x = uin.float().contiguous()
        k_hi = torch.full((B, L, 64), 7.0, dtype=torch.float16, device=x.device)
        k_pair = torch.full((B, L, 64, 2), 7, dtype=torch.uint8, device=x.device)
        vt = torch.full((B, 64, ldvt), 7.0, dtype=torch.float16, device=x.device)
        self._check(self.lib.sdm_op_cross_patch_planes_ex(self.h, _ptr(x), B, H, W_, _ptr(k_hi), _ptr(k_pair), _ptr(vt), int(ones_rows)),
                    "sdm_op_cross_patch_planes_ex")
        return k_hi, k_pair, vt

    def op_attention_shared(self, q, ks, vs, heads, q_prescaled=False):
        """Test hook: op_attention_split on ONE key / value operand ks / vs fp32 [B,Lk,64] for every head (head stride 0 for K and V^T)."""
        B, Lq, HD = q.shape
        Lk = ks.shape[1]
        qf, kf, vf = q.float().contiguous(), ks.float().contiguous(), vs.float().contiguous()
        out = torch.empty(B, Lq, HD, dtype=torch.float32, device=q.device)
        self._check(self.lib.sdm_op_attention_shared(self.h, _ptr(qf), _ptr(kf), _ptr(vf), B, heads, Lq, Lk, int(q_prescaled), _ptr(out)), "sdm_op_attention_shared")
        return out

    def debug_cross_attention(self, block, x_nhwc, uin):
        """Test hook: the cross-attention of one transformer block of the loaded model under the current options: x fp32 [B,H,W,C] = the output of norm2,
        uin fp32 [B,h,w,16] the U-Net input tensor -> to_out(attention) fp32 [B,H,W,C] (no residual)."""
        B, H, W_, Cc = x_nhwc.shape
        x, u = x_nhwc.float().contiguous(), uin.float().contiguous()
        out = torch.empty(B, H, W_, Cc, dtype=torch.float32, device=x.device)
        self._check(self.lib.sdm_debug_cross_attention(self.h, block.encode(), _ptr(x), B, H, W_, _ptr(u), u.shape[1], u.shape[2], _ptr(out)), "sdm_debug_cross_attention")
        return out

    def op_cross_core(self, q, uin, heads):
        """Test hook: the attention core of a cross-attention on the engine's own shared operand, any number of heads: q fp32 [B,Lq,heads*64] (pre-scaled,
        columns 36..63 of every head zero) and uin fp32 [B,h,w,16] -> fp32 [B,Lq,heads*64] under the current options (cross_narrow)."""
        B, Lq, HD = q.shape
        qf, u = q.float().contiguous(), uin.float().contiguous()
        out = torch.empty(B, Lq, HD, dtype=torch.float32, device=qf.device)
        self._check(self.lib.sdm_op_cross_core(self.h, _ptr(qf), _ptr(u), B, heads, Lq, u.shape[1], u.shape[2], _ptr(out)), "sdm_op_cross_core")
        return out

    def op_resize_aa(self, planes, Hout, Wout):
        P, Hin, Win = planes.shape
        out = torch.empty(P, Hout, Wout, dtype=torch.float32, device=planes.device)
        self._check(self.lib.sdm_op_resize_aa(self.h, _ptr(planes), P, Hin, Win, _ptr(out), Hout, Wout), "sdm_op_resize_aa")
        return out

    def patch_token_map(self, H, W_):
        """Test hook: the engine's own helper pair of the patch token order for one H x W image -> (takes the order, token_of_pixel [H*W], pixel_of_token [H*W])."""
        t_of_p = np.zeros(H * W_, np.int32); p_of_t = np.zeros(H * W_, np.int32)
        rc = self.lib.sdm_debug_patch_token_map(H, W_, t_of_p.ctypes.data_as(C.c_void_p), p_of_t.ctypes.data_as(C.c_void_p))
        if rc < 0:
            raise RuntimeError("sdm_debug_patch_token_map: bad arguments")
        return bool(rc), t_of_p, p_of_t

    def op_groupnorm_p3(self, x, gamma, beta, eps, groups=32, silu=False, tokens=True):
        """Test hook: GroupNorm of x fp32 [N,H,W,C] as the operand planes of proj_in, from ONE statistics pass -> (row-major planes, patch-order planes or None),
        each uint8 [ceil(N*H*W/32)*32 * C * 3] (fp16 hi plane, then the xl plane); in the patch-order planes row t of an image is token t."""
        N, H, W_, Cc = x.shape
        x = x.float().contiguous()
        rows_pad = (N * H * W_ + 31) // 32 * 32
        a = torch.full((rows_pad * Cc * 3,), 0x5A, dtype=torch.uint8, device=x.device)
        b = torch.full((rows_pad * Cc * 3,), 0x5A, dtype=torch.uint8, device=x.device) if tokens else None
        self._check(self.lib.sdm_op_groupnorm_p3(self.h, _ptr(x), N, H, W_, Cc, groups, _ptr(gamma.float().contiguous()), _ptr(beta.float().contiguous()), float(eps),
                                                 int(silu), _ptr(a), _ptr(b)), "sdm_op_groupnorm_p3")
        return a, b

    def op_gemm_p3_tokens(self, x, w, bias=None, mode=0, res=None, patch_tokens=False, out=None):
        """Test hook: the plane-fed GEMM mode 0 / 4 on x fp32 [N,H,W,K] whose rows are tokens; out / res are pixel-order [N,H,W,O] (patch_tokens) or plain rows.
        out: an fp32 [N,H,W,O] tensor to write into (may be a view inside a larger buffer: guard rows).  -> out, or (out, stats [N,srows,O,2]) for mode 4."""
        N, H, W_, K = x.shape
        O = w.shape[0]
        x = x.float().contiguous(); w = w.float().contiguous()
        b = bias.float().contiguous() if bias is not None else None
        r = res.float().contiguous() if res is not None else None
        if out is None:
            out = torch.empty(N, H, W_, O, dtype=torch.float32, device=x.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == N * H * W_ * O
        srows_max = 2 * ((H * W_ + 63) // 64)
        stats = torch.zeros(N * srows_max * O * 2, dtype=torch.float32, device=x.device) if mode == 4 else None
        srows = C.c_int(0)
        self._check(self.lib.sdm_op_gemm_p3_tokens(self.h, _ptr(x), N, H, W_, K, _ptr(w), _ptr(b), O, mode, _ptr(r), int(patch_tokens), _ptr(out), _ptr(stats),
                                                   C.byref(srows)), "sdm_op_gemm_p3_tokens")
        if mode == 4:
            return out, stats[:N * srows.value * O * 2].view(N, srows.value, O, 2)
        return out

    def op_mask_bias_tokens(self, plane, level, patch_tokens=True):
        """Test hook: the key bias of U-Net level `level` from the trimap plane fp32 [B,SH,SW] as the self-attentions get it (log2 domain) -> (fp32 [B, hk*wk],
        written in patch order?)."""
        B, SH, SW = plane.shape
        hk, wk = (SH // 8) >> level, (SW // 8) >> level
        out = torch.empty(B, hk * wk, dtype=torch.float32, device=plane.device)
        rc = self.lib.sdm_op_mask_bias_tokens(self.h, _ptr(plane.float().contiguous()), B, SH, SW, level, int(patch_tokens), _ptr(out))
        if rc < 0:
            self._check(rc, "sdm_op_mask_bias_tokens")
        return out, bool(rc)

    def op_active_tiles(self, bias):
        """Test hook: the engine's list of active 64-key tiles of a key bias fp32 [B,Lk] -> int32 [B, ceil(Lk/64) + 1] (count, then ascending tile indices)."""
        B, Lk = bias.shape
        out = torch.full((B, (Lk + 63) // 64 + 1), -1, dtype=torch.int32, device=bias.device)
        self._check(self.lib.sdm_op_active_tiles(self.h, _ptr(bias.float().contiguous()), B, Lk, _ptr(out)), "sdm_op_active_tiles")
        return out

    def op_mask_bias(self, plane_bss, level):
        B, S, _ = plane_bss.shape
        lk = (S // 8) >> level
        out = torch.empty(B, lk * lk, dtype=torch.float32, device=plane_bss.device)
        self._check(self.lib.sdm_op_mask_bias(self.h, _ptr(plane_bss), B, S, level, _ptr(out)), "sdm_op_mask_bias")
        return out
