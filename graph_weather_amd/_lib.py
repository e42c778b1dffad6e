"""ctypes binding of ``libgw_amd.so`` (C ABI declared in ``include/gw_amd.h``).

There is deliberately no fallback: if the shared library is missing or a call fails, a
``RuntimeError`` is raised - the product path never computes on the CPU or through torch ops.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libgw_amd.so")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-shared", "-fPIC"]

ABI_VERSION = 19
DTYPE_F32, DTYPE_BF16, DTYPE_BF16X3 = 0, 1, 2
LAYOUT_ROWS_F32, LAYOUT_EDGE_TILES_BF16, LAYOUT_ROWS_F16, LAYOUT_ROWS_BF16K = 0, 1, 2, 3
EDGE_DETERMINISTIC, EDGE_SEGMENT_TILES, EDGE_AGG_BF16K, EDGE_SEGMENT_SPLIT = 1, 2, 4, 8

EXPORTS = [
    "gw_version", "gw_last_error", "gw_debug_timestamps", "gw_packed_floats", "gw_pack_linear", "gw_packed_bytes_bf16",
    "gw_pack_linear_bf16", "gw_packed_bytes_bf16x3", "gw_pack_linear_bf16x3", "gw_padded_n", "gw_pad_vector", "gw_pack_many", "gw_mlp_chain_backward", "gw_mlp_chain_backward_bf16x3", "gw_mlp_ln_chain_backward",
    "gw_mlp_forward", "gw_mlp_post_forward", "gw_project_forward", "gw_edge_update_forward", "gw_edge_update_workspace_bytes", "gw_edge_tiles_bytes",
    "gw_edge_rows_to_tiles", "gw_node_update_forward", "gw_node_update_row_split_groups", "gw_node_update_head_forward",
    "gw_normalized_mse_forward", "gw_gemm_f32", "gw_relu_backward", "gw_layernorm_backward", "gw_gather_rows",
    "gw_segment_sum_rows", "gw_normalized_mse_backward", "gw_adamw_step", "gw_nudging_forward", "gw_nudging_backward",
    "gw_linear_forward", "gw_linear_gather_forward", "gw_layernorm_forward", "gw_add_rows", "gw_gather_rows_wide", "gw_segment_sum_rows_wide",
    "gw_constraint_workspace_bytes", "gw_constraint_forward", "gw_constraint_backward",
    "gw_thermal_conv_forward", "gw_thermal_conv_wgrad_workspace_bytes", "gw_thermal_conv_wgrad", "gw_thermal_colsum_workspace_bytes",
    "gw_thermal_colsum", "gw_thermal_groupnorm_workspace_bytes", "gw_thermal_groupnorm_forward", "gw_thermal_groupnorm_backward",
    "gw_thermal_maxpool_forward", "gw_thermal_maxpool_backward", "gw_thermal_resize_forward", "gw_thermal_resize_backward",
    "gw_thermal_rows",
    "gw_amse_mmax", "gw_amse_dft_rows", "gw_amse_legendre_floats", "gw_amse_coeff_floats", "gw_amse_workspace_bytes",
    "gw_amse_forward", "gw_amse_backward",
    "gw_modulate_workspace_bytes", "gw_sdl_forward", "gw_sdl_backward", "gw_film_forward", "gw_film_backward",
    "gw_attention_forward", "gw_attention_backward", "gw_knn_interpolate_forward", "gw_knn_interpolate_backward",
    "gw_gelu_forward", "gw_gelu_backward",
    "gw_attention_axial_forward", "gw_attention_axial_backward",
    "gw_patch_workspace_bytes", "gw_patch_embed_forward", "gw_patch_embed_backward", "gw_patch_expand_forward",
    "gw_patch_expand_backward",
    "gw_attention_masked_forward", "gw_attention_masked_backward",
    "gw_earth_loss_workspace_bytes", "gw_earth_loss_forward", "gw_earth_loss_backward",
    "gw_token_mean_forward", "gw_token_mean_backward", "gw_relu_forward", "gw_row_scale",
    "gw_conv3d_workspace_bytes", "gw_conv3d_forward", "gw_conv3d_backward",
    "gw_gemm_tn_ordered_workspace_bytes", "gw_gemm_tn_ordered", "gw_layernorm_backward_ordered_workspace_bytes",
    "gw_layernorm_backward_ordered",
    "gw_encoder_fused_forward",
    "gw_graph_attention_forward", "gw_graph_attention_backward", "gw_cond_layernorm_forward", "gw_cond_layernorm_backward",
    "gw_beta_gate_forward", "gw_beta_gate_workspace_bytes", "gw_beta_gate_backward", "gw_silu_forward", "gw_silu_backward",
    "gw_fourier_forward", "gw_fourier_backward",
    "gw_graph_attention_batched_forward", "gw_graph_attention_batched_backward", "gw_cond_layernorm_grouped_forward",
    "gw_cond_layernorm_grouped_workspace_bytes", "gw_cond_layernorm_grouped_backward", "gw_gencast_precond_input_forward",
    "gw_gencast_precond_input_backward", "gw_gencast_precond_output_forward", "gw_gencast_precond_output_backward",
    "gw_isht_lmax", "gw_isht_legendre_floats", "gw_isht_workspace_bytes", "gw_isht_forward",
    "gw_gencast_sampler_combine", "gw_gencast_weighted_mse_workspace_bytes", "gw_gencast_weighted_mse_forward",
    "gw_gencast_weighted_mse_backward",
    "gw_cond_layernorm_fanout_forward", "gw_cond_layernorm_fanout_workspace_bytes", "gw_cond_layernorm_fanout_backward",
    "gw_linear_gather_grouped_forward", "gw_segment_sum_rows_grouped",
    "gw_ensemble_crps_workspace_bytes", "gw_ensemble_crps_forward", "gw_ensemble_crps_backward",
    "gw_genda_input_forward", "gw_genda_input_backward", "gw_genda_guided_output_forward", "gw_genda_guided_output_backward",
    "gw_sparse_attention_forward", "gw_sparse_attention_backward",
    "gw_na3d_forward", "gw_na3d_backward",
    "gw_convnd_workspace_bytes", "gw_convnd_forward", "gw_convnd_dgrad", "gw_convnd_wgrad", "gw_convnd_bn_stats",
    "gw_convnd_tail_forward", "gw_convnd_tail_backward", "gw_convnd_upsample2x",
]

GEMM_NN, GEMM_TN, GEMM_TN_BF16X3 = 0, 1, 2


class GwOperand(Structure):
    _fields_ = [("ptr", c_void_p), ("index", c_void_p), ("rows_per_batch", c_int32), ("ld", c_int32), ("k", c_int32),
                ("projected", c_int32), ("layout", c_int32)]


class GwMlpWeights(Structure):
    _fields_ = [("w1", c_void_p * 3), ("b1", c_void_p), ("w_mid", c_void_p), ("b_mid", c_void_p), ("w_out", c_void_p),
                ("b_out", c_void_p), ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("hidden", c_int32),
                ("n_mid", c_int32), ("n_out", c_int32), ("weight_dtype", c_int32), ("ln_width", c_int32), ("k_in", c_int32),
                ("out_rows", c_int32)]


PACK_MAX_ITEMS = 16


class GwPackItem(Structure):  # include/gw_amd.h: gw_pack_item
    _fields_ = [("w", c_void_p), ("stride_f", c_int64), ("stride_k", c_int64), ("n_out", c_int32), ("kseg", c_int32),
                ("rows", c_int32), ("reserved", c_int32), ("out", c_void_p)]


CONSTRAINT_TYPES = {"additive": 1, "multiplicative": 2, "softmax": 3}  # GW_CONSTRAINT_*


class GwConstraintArgs(Structure):  # include/gw_amd.h: gw_constraint_args
    _fields_ = [("type", c_int32), ("batch", c_int32), ("nodes", c_int32), ("channels", c_int32), ("cells", c_int32),
                ("f", c_int32), ("grid_h", c_int32), ("grid_w", c_int32), ("graph_rows", c_int32), ("exp_factor", c_float),
                ("hr", c_void_p), ("ld_hr", c_int32), ("lr", c_void_p), ("ld_lr", c_int32), ("map", c_void_p),
                ("inv_ptr", c_void_p), ("inv_idx", c_void_p)]


ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2  # GW_ACT_*
CRPS_MEAN, CRPS_NONE = 0, 1  # GW_CRPS_*

CONVND_A_PLAIN, CONVND_A_BN_GELU = 0, 1  # GW_CONVND_A_*
THERMAL_MAX_TAPS = 7  # GW_THERMAL_MAX_TAPS
THERMAL_A_PLAIN, THERMAL_A_GN_RELU, THERMAL_A_DIFFUSE = 0, 1, 2  # GW_THERMAL_A_*
THERMAL_E_STORE, THERMAL_E_DIFFUSE = 0, 1  # GW_THERMAL_E_*
THERMAL_ROWS_FINALIZE, THERMAL_ROWS_SCALE, THERMAL_ROWS_AXPY = 0, 1, 2  # GW_THERMAL_ROWS_*


class GwThermalTaps(Structure):  # include/gw_amd.h: gw_thermal_taps
    _fields_ = [("n", c_int32), ("in_off", c_int32 * THERMAL_MAX_TAPS), ("w_idx", c_int32 * THERMAL_MAX_TAPS)]


class GwThermalConvArgs(Structure):  # include/gw_amd.h: gw_thermal_conv_args
    _fields_ = [("batch", c_int32), ("in_h", c_int32), ("in_w", c_int32), ("out_h", c_int32), ("out_w", c_int32), ("q_h", c_int32),
                ("q_w", c_int32), ("in_scale_h", c_int32), ("in_scale_w", c_int32), ("out_scale_h", c_int32),
                ("out_scale_w", c_int32), ("out_off_h", c_int32), ("out_off_w", c_int32), ("ty", GwThermalTaps),
                ("tx", GwThermalTaps), ("cin", c_int32), ("cout", c_int32), ("a_mode", c_int32), ("e_mode", c_int32),
                ("a", c_void_p), ("ld_a", c_int32), ("features", c_int32), ("a_scale", c_void_p), ("a_shift", c_void_p),
                ("w", c_void_p), ("w_stride_y", c_int64), ("w_stride_x", c_int64), ("w_stride_ci", c_int64),
                ("w_stride_co", c_int64), ("bias", c_void_p), ("out", c_void_p), ("ld_out", c_int32), ("ld_x", c_int32),
                ("x", c_void_p), ("eps", c_void_p), ("sa", c_float), ("s1", c_float)]


class GwPadItem(Structure):  # include/gw_amd.h: gw_pad_item
    _fields_ = [("v", c_void_p), ("n", c_int32), ("n_out", c_int32), ("out", c_void_p)]


class GwActivationSave(Structure):
    _fields_ = [("hidden", c_void_p), ("hidden_stride", c_int64), ("hidden_ld", c_int32), ("pre_norm", c_void_p)]


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into csrc/libgw_amd.so (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    deps.append(os.path.join(os.path.dirname(_HERE), "include", "gw_amd.h"))
    # GW_TUNING=1 builds the A/B knobs in (env-selected kernel variants, skip switches that give wrong results - used by
    # scripts/gpu_tune.sh and GW_TUNING=1 scripts/gpu_run.sh only; GW_HIPCC_EXTRA adds flags such as -DGW_LAYER_ABL=1); the shipped library is built without them.  The flag set is recorded beside
    # the library so that switching modes rebuilds.
    flags = HIPCC_FLAGS + (["-DGW_TUNING"] + os.environ.get("GW_HIPCC_EXTRA", "").split() if os.environ.get("GW_TUNING") == "1" else [])
    stamp = LIB_PATH + ".flags"
    want = " ".join(flags)
    try:
        have = open(stamp).read()
    except OSError:
        have = want if "-DGW_TUNING" not in want else ""
    if (not force and os.path.exists(LIB_PATH) and have == want
            and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps)):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + flags + srcs + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    with open(stamp, "w") as f:
        f.write(want)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "graph_weather_amd: %s is missing - the HIP extension must be built (python -c 'import __graft_entry__ as g; "
            "g.build()'); there is no CPU/torch fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    L.gw_version.restype = c_int
    L.gw_last_error.restype = c_char_p
    L.gw_debug_timestamps.restype = c_int
    L.gw_debug_timestamps.argtypes = [c_void_p, c_int, c_int]
    L.gw_packed_floats.restype = c_size_t
    L.gw_packed_floats.argtypes = [c_int, c_int, c_int]
    L.gw_pack_linear.restype = c_int
    L.gw_pack_linear.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    L.gw_packed_bytes_bf16.restype = c_size_t
    L.gw_packed_bytes_bf16.argtypes = [c_int, c_int, c_int]
    L.gw_pack_linear_bf16.restype = c_int
    L.gw_pack_linear_bf16.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    L.gw_packed_bytes_bf16x3.restype = c_size_t
    L.gw_packed_bytes_bf16x3.argtypes = [c_int, c_int, c_int]
    L.gw_pack_linear_bf16x3.restype = c_int
    L.gw_pack_linear_bf16x3.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    L.gw_padded_n.restype = c_int
    L.gw_padded_n.argtypes = [c_int]
    L.gw_pad_vector.restype = c_int
    L.gw_pad_vector.argtypes = [c_void_p, c_int, c_void_p, c_void_p]
    L.gw_mlp_chain_backward.restype = c_int
    L.gw_mlp_chain_backward.argtypes = [c_int64, c_void_p, c_int32, c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                        c_int32, POINTER(c_void_p), POINTER(c_void_p), c_void_p]
    L.gw_mlp_chain_backward_bf16x3.restype = c_int
    L.gw_mlp_chain_backward_bf16x3.argtypes = L.gw_mlp_chain_backward.argtypes
    L.gw_mlp_ln_chain_backward.restype = c_int
    L.gw_mlp_ln_chain_backward.argtypes = [c_int32, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_void_p,
                                           c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_int32, ctypes.c_uint32, c_void_p]
    L.gw_pack_many.restype = c_int
    L.gw_pack_many.argtypes = [c_int32, c_int32, POINTER(GwPackItem), c_int32, POINTER(GwPadItem), c_void_p]
    L.gw_mlp_forward.restype = c_int
    L.gw_mlp_forward.argtypes = [c_int64, c_int32, POINTER(GwOperand), POINTER(GwMlpWeights), POINTER(GwOperand),
                                 c_void_p, c_int32, POINTER(GwActivationSave), c_void_p]
    L.gw_mlp_post_forward.restype = c_int
    L.gw_mlp_post_forward.argtypes = [c_int64, c_int32, POINTER(GwOperand), POINTER(GwMlpWeights), c_void_p, c_int32, c_int32,
                                      POINTER(c_void_p), POINTER(c_void_p), c_int32, c_void_p]
    L.gw_edge_update_forward.restype = c_int
    L.gw_edge_update_forward.argtypes = [c_int32, c_int32, c_void_p, c_void_p, POINTER(GwOperand), POINTER(GwOperand),
                                         POINTER(GwOperand), POINTER(GwOperand), POINTER(GwMlpWeights), c_void_p, c_int32, c_void_p,
                                         c_int32, POINTER(GwActivationSave), c_void_p, c_size_t, c_int32, c_void_p]
    L.gw_encoder_fused_forward.restype = c_int
    L.gw_encoder_fused_forward.argtypes = [c_int32, c_int32, c_void_p, c_void_p, POINTER(GwOperand), POINTER(GwMlpWeights),
                                           POINTER(GwOperand), POINTER(GwOperand), POINTER(GwOperand), POINTER(GwMlpWeights), c_void_p,
                                           c_int32, POINTER(GwActivationSave), c_int32, c_void_p]
    L.gw_edge_tiles_bytes.restype = c_size_t
    L.gw_edge_tiles_bytes.argtypes = [c_int32, c_int32]
    L.gw_edge_rows_to_tiles.restype = c_int
    L.gw_edge_rows_to_tiles.argtypes = [c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]
    L.gw_edge_update_workspace_bytes.restype = c_size_t
    L.gw_edge_update_workspace_bytes.argtypes = [c_int32, c_int32, POINTER(GwOperand), POINTER(GwOperand), POINTER(GwOperand),
                                                 POINTER(GwMlpWeights), c_int32]
    L.gw_node_update_forward.restype = c_int
    L.gw_node_update_forward.argtypes = [c_int64, c_int32, POINTER(GwOperand), POINTER(GwOperand), POINTER(GwOperand),
                                         POINTER(GwMlpWeights), c_void_p, c_int32, POINTER(GwActivationSave), c_int32,
                                         POINTER(c_void_p), POINTER(c_void_p), c_int32, c_void_p, c_void_p]
    L.gw_node_update_row_split_groups.restype = c_int
    L.gw_node_update_row_split_groups.argtypes = [c_int64]
    L.gw_node_update_head_forward.restype = c_int
    L.gw_node_update_head_forward.argtypes = [c_int64, c_int32, POINTER(GwOperand), POINTER(GwOperand), POINTER(GwMlpWeights),
                                              POINTER(GwMlpWeights), POINTER(GwOperand), c_void_p, c_int32, c_void_p]
    L.gw_project_forward.restype = c_int
    L.gw_project_forward.argtypes = [c_int64, c_int32, POINTER(GwOperand), c_int32, POINTER(c_void_p), POINTER(c_void_p),
                                     c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    L.gw_normalized_mse_forward.restype = c_int
    L.gw_normalized_mse_forward.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                            c_void_p, c_void_p]
    L.gw_gemm_f32.restype = c_int
    L.gw_gemm_f32.argtypes = [c_int32, c_int64, c_int32, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p,
                              c_void_p]
    L.gw_relu_backward.restype = c_int
    L.gw_relu_backward.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]
    L.gw_layernorm_backward.restype = c_int
    L.gw_layernorm_backward.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                        c_void_p, c_void_p]
    L.gw_gather_rows.restype = c_int
    L.gw_gather_rows.argtypes = [c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_segment_sum_rows.restype = c_int
    L.gw_segment_sum_rows.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_normalized_mse_backward.restype = c_int
    L.gw_normalized_mse_backward.argtypes = [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                             c_void_p, c_void_p, c_void_p]
    L.gw_adamw_step.restype = c_int
    L.gw_adamw_step.argtypes = [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_float,
                                c_int32, c_void_p]
    L.gw_nudging_forward.restype = c_int
    L.gw_nudging_forward.argtypes = [c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p]
    L.gw_nudging_backward.restype = c_int
    L.gw_nudging_backward.argtypes = [c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_linear_forward.restype = c_int
    L.gw_linear_forward.argtypes = [c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                    c_void_p]
    L.gw_layernorm_forward.restype = c_int
    L.gw_layernorm_forward.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int64, c_void_p,
                                       c_int32, c_void_p]
    L.gw_linear_gather_forward.restype = c_int
    L.gw_linear_gather_forward.argtypes = [c_int64, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                           POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int32), POINTER(c_int32), c_int32, c_void_p,
                                           c_int32, c_void_p]
    L.gw_linear_gather_grouped_forward.restype = c_int
    L.gw_linear_gather_grouped_forward.argtypes = [c_int64, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                                   POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int32), POINTER(c_int32),
                                                   POINTER(c_int32), c_int32, c_void_p, c_int32, c_void_p]
    L.gw_segment_sum_rows_grouped.restype = c_int
    L.gw_segment_sum_rows_grouped.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                              c_int32, c_void_p]
    L.gw_add_rows.restype = c_int
    L.gw_add_rows.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]
    L.gw_gather_rows_wide.restype = c_int
    L.gw_gather_rows_wide.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_segment_sum_rows_wide.restype = c_int
    L.gw_segment_sum_rows_wide.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                           c_int32, c_void_p]
    L.gw_constraint_workspace_bytes.restype = c_size_t
    L.gw_constraint_workspace_bytes.argtypes = [POINTER(GwConstraintArgs)]
    L.gw_constraint_forward.restype = c_int
    L.gw_constraint_forward.argtypes = [POINTER(GwConstraintArgs), c_void_p, c_size_t, c_void_p, c_int32, c_void_p]
    L.gw_constraint_backward.restype = c_int
    L.gw_constraint_backward.argtypes = [POINTER(GwConstraintArgs), c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_int32, c_void_p,
                                         c_int32, c_void_p]
    L.gw_thermal_conv_forward.restype = c_int
    L.gw_thermal_conv_forward.argtypes = [POINTER(GwThermalConvArgs), c_void_p]
    L.gw_thermal_conv_wgrad_workspace_bytes.restype = c_size_t
    L.gw_thermal_conv_wgrad_workspace_bytes.argtypes = [POINTER(GwThermalConvArgs)]
    L.gw_thermal_conv_wgrad.restype = c_int
    L.gw_thermal_conv_wgrad.argtypes = [POINTER(GwThermalConvArgs), c_void_p, c_size_t, c_void_p, c_void_p]
    L.gw_thermal_colsum_workspace_bytes.restype = c_size_t
    L.gw_thermal_colsum_workspace_bytes.argtypes = [c_int64, c_int32]
    L.gw_thermal_colsum.restype = c_int
    L.gw_thermal_colsum.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_void_p]
    L.gw_thermal_groupnorm_workspace_bytes.restype = c_size_t
    L.gw_thermal_groupnorm_workspace_bytes.argtypes = [c_int32, c_int32, c_int32, c_int32]
    L.gw_thermal_groupnorm_forward.restype = c_int
    L.gw_thermal_groupnorm_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_float,
                                               c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_thermal_groupnorm_backward.restype = c_int
    L.gw_thermal_groupnorm_backward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_thermal_maxpool_forward.restype = c_int
    L.gw_thermal_maxpool_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                             c_int32, c_void_p, c_void_p]
    L.gw_thermal_maxpool_backward.restype = c_int
    L.gw_thermal_maxpool_backward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32,
                                              c_void_p, c_void_p]
    L.gw_thermal_resize_forward.restype = c_int
    L.gw_thermal_resize_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                            c_void_p]
    L.gw_thermal_resize_backward.restype = c_int
    L.gw_thermal_resize_backward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p,
                                             c_void_p]
    L.gw_thermal_rows.restype = c_int
    L.gw_thermal_rows.argtypes = [c_int32, c_int64, c_int32, c_float, c_float, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                  c_void_p, c_int32, c_void_p]
    L.gw_amse_mmax.restype = c_int32
    L.gw_amse_mmax.argtypes = [c_int32, c_int32]
    L.gw_amse_dft_rows.restype = c_int32
    L.gw_amse_dft_rows.argtypes = [c_int32, c_int32]
    L.gw_amse_legendre_floats.restype = c_size_t
    L.gw_amse_legendre_floats.argtypes = [c_int32, c_int32]
    L.gw_amse_coeff_floats.restype = c_size_t
    L.gw_amse_coeff_floats.argtypes = [c_int32, c_int32, c_int32]
    L.gw_amse_workspace_bytes.restype = c_size_t
    L.gw_amse_workspace_bytes.argtypes = [c_int32, c_int32, c_int32, c_int32]
    L.gw_amse_forward.restype = c_int
    L.gw_amse_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  ctypes.c_double, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_amse_backward.restype = c_int
    L.gw_amse_backward.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                   c_void_p, c_void_p]
    L.gw_isht_lmax.restype = c_int32
    L.gw_isht_lmax.argtypes = [c_int32, c_int32]
    L.gw_isht_legendre_floats.restype = c_size_t
    L.gw_isht_legendre_floats.argtypes = [c_int32, c_int32]
    L.gw_isht_workspace_bytes.restype = c_size_t
    L.gw_isht_workspace_bytes.argtypes = [c_int32, c_int32, c_int32]
    L.gw_isht_forward.restype = c_int
    L.gw_isht_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_size_t,
                                  c_void_p, c_void_p]
    L.gw_modulate_workspace_bytes.restype = c_size_t
    L.gw_modulate_workspace_bytes.argtypes = [c_int64, c_int64]
    L.gw_sdl_forward.restype = c_int
    L.gw_sdl_forward.argtypes = [c_int64, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_sdl_backward.restype = c_int
    L.gw_sdl_backward.argtypes = [c_int64, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                  c_void_p, c_void_p, c_void_p]
    L.gw_film_forward.restype = c_int
    L.gw_film_forward.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_film_backward.restype = c_int
    L.gw_film_backward.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                   c_void_p]
    L.gw_attention_forward.restype = c_int
    L.gw_attention_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_void_p,
                                       c_int32, c_void_p, c_void_p]
    L.gw_attention_backward.restype = c_int
    L.gw_attention_backward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_void_p,
                                        c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_knn_interpolate_forward.restype = c_int
    L.gw_knn_interpolate_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                             c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p]
    L.gw_knn_interpolate_backward.restype = c_int
    L.gw_knn_interpolate_backward.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                              c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p]
    L.gw_gelu_forward.restype = c_int
    L.gw_gelu_forward.argtypes = [c_int64, c_void_p, c_void_p, c_void_p]
    L.gw_gelu_backward.restype = c_int
    L.gw_gelu_backward.argtypes = [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_attention_axial_forward.restype = c_int
    L.gw_attention_axial_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, POINTER(c_int64),
                                             c_float, c_void_p, POINTER(c_int64), c_void_p, c_void_p]
    L.gw_attention_axial_backward.restype = c_int
    L.gw_attention_axial_backward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, POINTER(c_int64),
                                              c_float, c_void_p, POINTER(c_int64), c_void_p, POINTER(c_int64), c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_void_p]
    L.gw_patch_workspace_bytes.restype = c_size_t
    L.gw_patch_workspace_bytes.argtypes = [c_int32] * 6
    L.gw_patch_embed_forward.restype = c_int
    L.gw_patch_embed_forward.argtypes = [c_int32] * 6 + [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_patch_embed_backward.restype = c_int
    L.gw_patch_embed_backward.argtypes = [c_int32] * 6 + [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_void_p,
                                                          c_void_p, c_void_p]
    L.gw_patch_expand_forward.restype = c_int
    L.gw_patch_expand_forward.argtypes = [c_int32] * 6 + [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_patch_expand_backward.restype = c_int
    L.gw_patch_expand_backward.argtypes = [c_int32] * 6 + [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int32,
                                                           c_void_p, c_void_p, c_void_p]
    L.gw_attention_masked_forward.restype = c_int
    L.gw_attention_masked_forward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, POINTER(c_int64),
                                              c_void_p, c_float, c_void_p, POINTER(c_int64), c_void_p, c_void_p]
    L.gw_attention_masked_backward.restype = c_int
    L.gw_attention_masked_backward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, POINTER(c_int64),
                                               c_void_p, c_float, c_void_p, POINTER(c_int64), c_void_p, POINTER(c_int64), c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_void_p]
    L.gw_earth_loss_workspace_bytes.restype = c_size_t
    L.gw_earth_loss_workspace_bytes.argtypes = [c_int32, c_int32, c_int32]
    L.gw_earth_loss_forward.restype = c_int
    L.gw_earth_loss_forward.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_float,
                                        c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_earth_loss_backward.restype = c_int
    L.gw_earth_loss_backward.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float, c_float,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_token_mean_forward.restype = c_int
    L.gw_token_mean_forward.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]
    L.gw_token_mean_backward.restype = c_int
    L.gw_token_mean_backward.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p]
    L.gw_relu_forward.restype = c_int
    L.gw_relu_forward.argtypes = [c_int64, c_void_p, c_void_p, c_void_p]
    L.gw_row_scale.restype = c_int
    L.gw_row_scale.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_conv3d_workspace_bytes.restype = c_size_t
    L.gw_conv3d_workspace_bytes.argtypes = [c_int32] * 7
    L.gw_conv3d_forward.restype = c_int
    L.gw_conv3d_forward.argtypes = [c_int32] * 7 + [c_void_p, POINTER(c_int64), c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_void_p]
    L.gw_conv3d_backward.restype = c_int
    L.gw_conv3d_backward.argtypes = [c_int32] * 7 + [c_void_p, POINTER(c_int64), c_void_p, c_void_p, POINTER(c_int64), c_void_p, c_size_t,
                                                     c_void_p, POINTER(c_int64), c_void_p, c_void_p, c_void_p]
    L.gw_gemm_tn_ordered_workspace_bytes.restype = c_size_t
    L.gw_gemm_tn_ordered_workspace_bytes.argtypes = [c_int32, c_int32, c_int64]
    L.gw_gemm_tn_ordered.restype = c_int
    L.gw_gemm_tn_ordered.argtypes = [c_int32, c_int32, c_int64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_size_t, c_void_p, c_int32,
                                     c_void_p, c_void_p]
    L.gw_layernorm_backward_ordered_workspace_bytes.restype = c_size_t
    L.gw_layernorm_backward_ordered_workspace_bytes.argtypes = [c_int64, c_int32]
    L.gw_layernorm_backward_ordered.restype = c_int
    L.gw_layernorm_backward_ordered.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_size_t,
                                                c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    L.gw_graph_attention_forward.restype = c_int
    L.gw_graph_attention_forward.argtypes = [c_int32] * 5 + [c_void_p, c_void_p, c_void_p] + [c_void_p, c_int32] * 4 + [
        c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]
    L.gw_graph_attention_backward.restype = c_int
    L.gw_graph_attention_backward.argtypes = [c_int32] * 5 + [c_void_p] * 6 + [c_void_p, c_int32] * 4 + [
        c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p] + [c_void_p, c_int32] * 4 + [c_void_p]
    L.gw_graph_attention_batched_forward.restype = c_int
    L.gw_graph_attention_batched_forward.argtypes = [c_int32, c_int64] + L.gw_graph_attention_forward.argtypes
    L.gw_graph_attention_batched_backward.restype = c_int
    L.gw_graph_attention_batched_backward.argtypes = [c_int32, c_int64] + L.gw_graph_attention_backward.argtypes
    L.gw_cond_layernorm_grouped_forward.restype = c_int
    L.gw_cond_layernorm_grouped_forward.argtypes = [c_int64, c_int32, c_int32, c_int64] + [c_void_p, c_int32] * 4 + [c_void_p]
    L.gw_cond_layernorm_grouped_workspace_bytes.restype = c_size_t
    L.gw_cond_layernorm_grouped_workspace_bytes.argtypes = [c_int64, c_int32, c_int64]
    L.gw_cond_layernorm_grouped_backward.restype = c_int
    L.gw_cond_layernorm_grouped_backward.argtypes = [c_int64, c_int32, c_int32, c_int64] + [c_void_p, c_int32] * 4 + [
        c_void_p, c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_cond_layernorm_fanout_forward.restype = c_int
    L.gw_cond_layernorm_fanout_forward.argtypes = [c_int64, c_int32, c_int32, c_int64, c_int32] + [c_void_p, c_int32] * 4 + [c_void_p]
    L.gw_cond_layernorm_fanout_workspace_bytes.restype = c_size_t
    L.gw_cond_layernorm_fanout_workspace_bytes.argtypes = [c_int64, c_int32, c_int64, c_int32]
    L.gw_cond_layernorm_fanout_backward.restype = c_int
    L.gw_cond_layernorm_fanout_backward.argtypes = [c_int64, c_int32, c_int32, c_int64, c_int32] + [c_void_p, c_int32] * 4 + [
        c_void_p, c_size_t, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_gencast_precond_input_forward.restype = c_int
    L.gw_gencast_precond_input_forward.argtypes = [c_int32, c_int64, c_int32, c_int32, c_int32, c_float, c_void_p] + [
        c_void_p, c_int32] * 4 + [c_void_p, c_void_p]
    L.gw_gencast_precond_input_backward.restype = c_int
    L.gw_gencast_precond_input_backward.argtypes = [c_int32, c_int64, c_int32, c_int32, c_float, c_void_p] + [c_void_p, c_int32] * 3 + [
        c_void_p]
    L.gw_gencast_precond_output_forward.restype = c_int
    L.gw_gencast_precond_output_forward.argtypes = [c_int32, c_int64, c_int32, c_float, c_void_p] + [c_void_p, c_int32] * 3 + [c_void_p]
    L.gw_gencast_precond_output_backward.restype = c_int
    L.gw_gencast_precond_output_backward.argtypes = [c_int32, c_int64, c_int32, c_float, c_void_p] + [c_void_p, c_int32] * 3 + [c_void_p]
    L.gw_gencast_sampler_combine.restype = c_int
    L.gw_gencast_sampler_combine.argtypes = [c_int64, c_float, c_void_p, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p]
    L.gw_gencast_weighted_mse_workspace_bytes.restype = c_size_t
    L.gw_gencast_weighted_mse_workspace_bytes.argtypes = [c_int32] * 4
    L.gw_gencast_weighted_mse_forward.restype = c_int
    L.gw_gencast_weighted_mse_forward.argtypes = [c_int32] * 4 + [c_float] + [c_void_p] * 6 + [c_size_t, c_void_p, c_void_p, c_void_p]
    L.gw_gencast_weighted_mse_backward.restype = c_int
    L.gw_gencast_weighted_mse_backward.argtypes = [c_int32] * 4 + [c_float] + [c_void_p] * 8
    L.gw_cond_layernorm_forward.restype = c_int
    L.gw_cond_layernorm_forward.argtypes = [c_int64, c_int32, c_int32] + [c_void_p, c_int32] * 4 + [c_void_p]
    L.gw_cond_layernorm_backward.restype = c_int
    L.gw_cond_layernorm_backward.argtypes = [c_int64, c_int32, c_int32] + [c_void_p, c_int32] * 5 + [c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_beta_gate_forward.restype = c_int
    L.gw_beta_gate_forward.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_void_p]
    L.gw_beta_gate_workspace_bytes.restype = c_size_t
    L.gw_beta_gate_workspace_bytes.argtypes = [c_int64, c_int32]
    L.gw_beta_gate_backward.restype = c_int
    L.gw_beta_gate_backward.argtypes = [c_int64, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                        c_void_p, c_size_t, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]
    L.gw_silu_forward.restype = c_int
    L.gw_silu_forward.argtypes = [c_int64, c_void_p, c_void_p, c_void_p]
    L.gw_silu_backward.restype = c_int
    L.gw_silu_backward.argtypes = [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_fourier_forward.restype = c_int
    L.gw_fourier_forward.argtypes = [c_int64, c_int32, c_float, c_void_p, c_void_p, c_int32, c_void_p]
    L.gw_fourier_backward.restype = c_int
    L.gw_fourier_backward.argtypes = [c_int64, c_int32, c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]
    L.gw_ensemble_crps_workspace_bytes.restype = c_size_t
    L.gw_ensemble_crps_workspace_bytes.argtypes = [c_int32] * 5
    L.gw_ensemble_crps_forward.restype = c_int
    L.gw_ensemble_crps_forward.argtypes = [c_int32] * 5 + [ctypes.c_double, c_int32] + [c_void_p] * 5 + [c_size_t, c_void_p, c_void_p]
    L.gw_ensemble_crps_backward.restype = c_int
    L.gw_ensemble_crps_backward.argtypes = [c_int32] * 5 + [ctypes.c_double, c_int32] + [c_void_p] * 7
    L.gw_genda_input_forward.restype = c_int
    L.gw_genda_input_forward.argtypes = [c_int32, c_int64] + [c_int32] * 5 + [c_float, c_void_p] + [c_void_p, c_int32] * 6 + [
        c_void_p, c_void_p]
    L.gw_genda_input_backward.restype = c_int
    L.gw_genda_input_backward.argtypes = [c_int32, c_int64] + [c_int32] * 5 + [c_float, c_void_p] + [c_void_p, c_int32] * 5 + [c_void_p]
    L.gw_genda_guided_output_forward.restype = c_int
    L.gw_genda_guided_output_forward.argtypes = [c_int32, c_int64, c_int32, c_float, c_float, c_void_p] + [c_void_p, c_int32] * 3 + [c_void_p]
    L.gw_genda_guided_output_backward.restype = c_int
    L.gw_genda_guided_output_backward.argtypes = [c_int32, c_int64, c_int32, c_float, c_float, c_void_p] + [c_void_p, c_int32] * 3 + [c_void_p]
    L.gw_sparse_attention_forward.restype = c_int
    L.gw_sparse_attention_forward.argtypes = [c_int32] * 6 + [c_float, c_void_p, c_void_p] + [c_void_p, c_int32] * 4 + [c_void_p, c_void_p]
    L.gw_sparse_attention_backward.restype = c_int
    L.gw_sparse_attention_backward.argtypes = [c_int32] * 6 + [c_float] + [c_void_p] * 5 + [c_void_p, c_int32] * 5 + [
        c_void_p, c_void_p] + [c_void_p, c_int32] * 3 + [c_void_p]
    L.gw_na3d_forward.restype = c_int
    L.gw_na3d_forward.argtypes = [c_int32] * 9 + [c_float] + [c_void_p, c_int32] * 4 + [c_void_p, c_void_p]
    L.gw_na3d_backward.restype = c_int
    L.gw_na3d_backward.argtypes = [c_int32] * 9 + [c_float] + [c_void_p, c_int32] * 5 + [c_void_p, c_void_p] + [c_void_p, c_int32] * 3 + [
        c_void_p]
    i64p, i32p = POINTER(c_int64), POINTER(c_int32)
    L.gw_convnd_workspace_bytes.restype = c_size_t
    L.gw_convnd_workspace_bytes.argtypes = [i32p]
    L.gw_convnd_forward.restype = c_int
    L.gw_convnd_forward.argtypes = [i32p, c_int32, c_void_p, i64p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, i64p, c_void_p]
    L.gw_convnd_dgrad.restype = c_int
    L.gw_convnd_dgrad.argtypes = [i32p, c_void_p, i64p, c_void_p, c_void_p, i64p, c_int32, c_void_p]
    L.gw_convnd_wgrad.restype = c_int
    L.gw_convnd_wgrad.argtypes = [i32p, c_int32, c_void_p, i64p, c_void_p, c_void_p, c_void_p, i64p, c_void_p, c_size_t, c_void_p,
                                  c_void_p, c_void_p]
    L.gw_convnd_bn_stats.restype = c_int
    L.gw_convnd_bn_stats.argtypes = [c_int32, c_int32, c_int64, c_int32, c_void_p, i64p, c_void_p, c_void_p, c_float, c_float,
                                     c_void_p, c_void_p, c_void_p, c_void_p]
    L.gw_convnd_tail_forward.restype = c_int
    L.gw_convnd_tail_forward.argtypes = [c_int32, c_int32, c_int64, c_void_p, i64p, c_void_p, c_void_p, i64p, c_void_p, c_void_p, i64p,
                                         c_void_p]
    L.gw_convnd_tail_backward.restype = c_int
    L.gw_convnd_tail_backward.argtypes = [c_int32, c_int32, c_int64, c_int32, c_void_p, i64p, c_void_p, i64p, c_void_p, c_void_p, i64p,
                                          c_void_p, c_void_p, c_void_p, i64p, c_void_p, i64p, c_void_p]
    L.gw_convnd_upsample2x.restype = c_int
    L.gw_convnd_upsample2x.argtypes = [c_int32] * 6 + [c_void_p, i64p, c_void_p, i64p, c_void_p]
    if L.gw_version() != ABI_VERSION:
        raise RuntimeError("graph_weather_amd: libgw_amd.so ABI version mismatch")
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().gw_last_error().decode(errors="replace")
        raise RuntimeError("graph_weather_amd: %s failed (%d): %s" % (what, rc, msg))
