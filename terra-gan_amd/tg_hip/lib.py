"""ctypes loader for libterragan_hip.so -- one entry per declaration in include/terragan_hip.h."""
import ctypes as C
import os

# torch MUST be imported before the library is dlopen'ed: the torch wheel bundles its own ROCm runtime
# (libamdhip64.so.7, libhsa-runtime64) and libterragan_hip.so has to bind to THAT copy -- the same
# SONAME under /opt/rocm is a different build, and two HIP runtimes in one process cannot share streams.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# TG_HIP_LIB: another build of the SAME library (timing probes of kernel variants, tools/); never a different implementation
LIB_PATH = os.environ.get("TG_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libterragan_hip.so")


class TgConv(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "Cin", "Ho", "Wo", "Cout", "k", "stride", "pad", "precision")]


TG_MASK_PYRAMID_MAX = 24


class TgMaskOp(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "H", "W", "Ho", "Wo", "k", "stride", "pad")] + \
               [(n, C.c_void_p) for n in ("in_", "in2", "out", "out2")]


class TgMaskPyramid(C.Structure):
    _fields_ = [("nops", C.c_int32), ("_pad", C.c_int32), ("op", TgMaskOp * TG_MASK_PYRAMID_MAX)]


class TgBnAct(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("mean", "rstd", "gamma", "beta")] + [("act", C.c_int32), ("slope", C.c_float)]


class TgSparseMap(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("bits", "list", "count", "pix")] + [(n, C.c_int32) for n in ("nb", "tiles_y", "tiles_x", "_pad")]


class TgRasterPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "wh", "ww", "overlap", "ny", "nx")]


TG_EVAL_MAX_CLASSES = 8


class TgAreaClasses(C.Structure):
    _fields_ = [("n_edges", C.c_int32), ("_pad", C.c_int32), ("px", C.c_int64 * (TG_EVAL_MAX_CLASSES - 1))]


TG_EDT_FAR, TG_EDT_MAX_SIDE, TG_DEPTH_MAX_CLASSES = 0x7fffffff, 32767, 8


class TgDepthClasses(C.Structure):
    _fields_ = [("n_edges", C.c_int32), ("_pad", C.c_int32), ("d2", C.c_int32 * (TG_DEPTH_MAX_CLASSES - 1))]


TG_FLOW_OUT, TG_FLOW_UNDECIDED, TG_FLOW_PIT, TG_FLOW_FAR, TG_FLOW_MAX_ROUNDS = 9, 254, 255, 0x7fffffff, 32
TG_FLOW_BASIN_COUNTS, TG_FLOW_COMPARE_COUNTS = 3, 19
TG_STREAM_HEAD, TG_STREAM_INTERIOR, TG_STREAM_JUNCTION, TG_STREAM_ORDER_BINS = 1, 2, 3, 15
TG_STREAM_ORDER_COUNTS = 1 + 2 * TG_STREAM_ORDER_BINS
TG_FLOOD_MAX_STAGES = 8
TG_FLOOD_COUNTS = 6 + 3 * TG_FLOOD_MAX_STAGES
TG_MFD_MAX_EXPONENT, TG_MFD_COUNTS = 8, 5
TG_TEX_OCTAVES, TG_TEX_SCALES, TG_TEX_NSUM = 5, 10, 3
TG_VGM_OCTAVES, TG_VGM_SCALES = 6, 12
TG_VGM_POWER, TG_VGM_EXPONENTIAL, TG_VGM_SPHERICAL = 0, 1, 2
TG_SIM_MAX_WAVES = 512


class TgFloodStages(C.Structure):
    _fields_ = [("s", C.c_float * TG_FLOOD_MAX_STAGES)]


class TgError(RuntimeError):
    pass


P, I, I64, F, SZ, D = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t, C.c_double
CP = C.POINTER(TgConv)
RP = C.POINTER(TgRasterPlan)

# name -> (restype, argtypes); mirrors include/terragan_hip.h line by line
SIGNATURES = {
    "tg_version": (I, []),
    "tg_last_error": (C.c_char_p, []),
    "tg_conv_fwd_ws_bytes": (SZ, [CP]),
    "tg_conv_fwd": (I, [CP, P, P, P, P, P, I, F, P, P, SZ, P]),
    "tg_conv_dgrad_ws_bytes": (SZ, [CP]),
    "tg_conv_dgrad": (I, [CP, P, P, P, P, I, P, SZ, P]),
    "tg_conv_dgrad_gated": (I, [CP, P, P, P, P, I, F, P, P, SZ, P]),
    "tg_set_cu_reserve": (I, [I]),
    "tg_set_work_stealing": (I, [I]),
    "tg_conv_wprep_bytes": (SZ, [CP, I]),
    "tg_conv_wprep": (I, [CP, I, P, P, P]),
    "tg_conv_wprep_item_bytes": (SZ, []),
    "tg_conv_wprep_item": (I, [CP, I, P, P, P]),
    "tg_conv_wprep_run": (I, [P, I, P]),
    "tg_conv_fwd_p": (I, [CP, P, P, P, P, P, P, I, F, P, P, SZ, P]),
    "tg_conv_fwd_pool": (I, [CP, P, P, P, P, P, P, I, F, P, P, P, SZ, P]),
    "tg_conv_pool_code_supported": (I, [CP]),
    "tg_conv_fwd_pool_code": (I, [CP, P, P, P, P, P, P, P, SZ, P]),
    "tg_maxpool2_bwd_code": (I, [P, P, I, I, I, I, P, P]),
    "tg_vgg_sparse_map_bytes": (SZ, [I, I, I, C.c_char_p]),
    "tg_vgg_sparse_map": (I, [P, P, I, I, I, C.c_char_p, P, SZ, P, C.POINTER(TgSparseMap), P]),
    "tg_conv_dgrad_sparse": (I, [CP, P, P, P, P, I, F, P, P, C.POINTER(TgSparseMap), P, SZ, P]),
    "tg_conv_dgrad_sparse_planned": (I, [CP, I, C.POINTER(TgSparseMap)]),
    "tg_maxpool2_bwd_code_sparse": (I, [P, P, I, I, I, I, P, C.POINTER(TgSparseMap), P]),
    "tg_conv_fwd_sparse": (I, [CP, P, P, P, P, I, F, P, P, P, C.POINTER(TgSparseMap), P, SZ, P]),
    "tg_conv_bnin_supported": (I, [CP, I]),
    "tg_conv_fwd_bnin": (I, [CP, P, C.POINTER(TgBnAct), P, P, I, F, P, P, SZ, P]),
    "tg_conv_wgrad_bnin": (I, [CP, P, C.POINTER(TgBnAct), P, P, P, P, SZ, P]),
    "tg_conv_dgrad_p": (I, [CP, P, P, P, P, P, I, F, P, I, P, SZ, P]),
    "tg_relu_gate_pack": (I, [P, I64, I, P, P]),
    "tg_conv_dgrad_gbits": (I, [CP, P, P, P, P, P, P, I, P, SZ, P]),
    "tg_conv_wgrad_ws_bytes": (SZ, [CP]),
    "tg_conv_wgrad": (I, [CP, P, P, P, P, P, P, SZ, P]),
    "tg_fold_cin": (I, [P, I, I, I, P, P]),
    "tg_mask_update": (I, [P, I, I, I, I, I, I, I, I, P, P, P]),
    "tg_mask_up_merge": (I, [P, P, I, I, I, I, I, P, P]),
    "tg_mask_pyramid": (I, [C.POINTER(TgMaskPyramid), I, P]),
    "tg_bn_ws_bytes": (SZ, [I64, I]),
    "tg_bn_stats": (I, [P, I64, I, F, F, P, P, P, P, P, P, SZ, P]),
    "tg_bn_eval_stats": (I, [P, P, I, F, P, P, P]),
    "tg_bn_act_fwd": (I, [P, I64, I, P, P, P, P, I, F, P, P]),
    "tg_bn_fwd": (I, [P, I64, I, F, F, P, P, I, F, P, P, P, P, P, P, P, SZ, P]),
    "tg_bn_act_bwd": (I, [P, P, I64, I, P, P, P, P, I, F, P, P, P, P, P, P, SZ, P]),
    "tg_bn_bwd_conv1_supported": (I, [I64, I]),
    "tg_bn_conv1_ws_bytes": (SZ, [I64, I]),
    "tg_bn_act_bwd_conv1": (I, [P, P, I, I, I, P, I, P, P, P, P, I, F, P, P, P, P, P, P, SZ, P]),
    "tg_act_bwd": (I, [P, P, I64, I, I, F, P, P, P]),
    "tg_upcat_fwd": (I, [P, P, P, I, I, I, I, I, I, I, P, P]),
    "tg_upcat_bn_supported": (I, [I, I, I, I, I, I, I]),
    "tg_upcat_fwd_bn": (I, [P, C.POINTER(TgBnAct), P, P, I, I, I, I, I, I, I, P, P]),
    "tg_upcat_bwd": (I, [P, I, I, I, I, I, I, I, P, P, P]),
    "tg_sigmoid_composite_fwd": (I, [P, P, P, I64, P, P]),
    "tg_sigmoid_composite_bwd": (I, [P, P, P, I64, P, P, P]),
    "tg_maxpool2_fwd": (I, [P, I, I, I, I, P, P]),
    "tg_maxpool2_bwd": (I, [P, P, I, I, I, I, I, P, P]),
    "tg_pixel_loss_ws_bytes": (SZ, [I, I, I]),
    "tg_pixel_losses": (I, [P, P, P, P, I, I, I, F, F, F, F, P, P, P, I, P, SZ, P]),
    "tg_reduce_ws_bytes": (SZ, [I64]),
    "tg_l1_mean": (I, [P, P, I64, F, P, P, P, P, SZ, P]),
    "tg_l1_mean_relu": (I, [P, P, I64, F, P, P, P, P, SZ, P]),
    "tg_bce_logits": (I, [P, I64, F, F, P, P, P, P, SZ, P]),
    "tg_adam": (I, [P, P, P, P, I64, D, D, D, D, I, F, P]),
    "tg_adam_multi": (I, [P, P, I, I, D, D, D, D, I, F, P]),
    "tg_adam_scalars": (I, [D, D, D, I, P]),
    "tg_write_floats": (I, [P, I, P, P]),
    "tg_adam_multi_s": (I, [P, P, I, I, D, D, D, P, F, P]),
    "tg_axpby": (I, [P, F, F, P, I64, P]),
    "tg_lincomb": (I, [P, F, P, F, P, I64, P]),
    "tg_mul": (I, [P, P, P, I64, P]),
    "tg_mul_keep": (I, [P, P, P, P, I64, P]),
    "tg_bn_running_update": (I, [P, P, I64, I, F, F, P, P, P, P]),
    "tg_bn_grouped_ws_bytes": (SZ, [I64, I, I]),
    "tg_bn_fwd_grouped": (I, [P, I64, I, I, F, P, P, I, F, P, P, P, P, SZ, P]),
    "tg_bn_act_bwd_grouped": (I, [P, P, I64, I, I, P, P, P, P, I, F, P, P, P, P, P, SZ, P]),
    "tg_bn_running_update_multi": (I, [P, P, I64, I, F, F, C.POINTER(C.c_int), I, P, P, P, P]),
    "tg_quality_metrics_ws_bytes": (SZ, [I64, I, I]),
    "tg_quality_metrics": (I, [P, P, P, I64, I, I, P, P, SZ, P]),
    "tg_u8_to_tiles": (I, [P, P, I64, P, P, P]),
    "tg_raster_window_stats": (I, [P, P, RP, I, F, P, P, P, P]),
    "tg_raster_gather": (I, [P, P, RP, I, F, P, P, P, I, P, P, P]),
    "tg_raster_blend": (I, [P, P, RP, I, F, P, P, P, P, I, P, P, P]),
    "tg_raster_gather_ops": (I, [P, P, RP, I, F, P, P, P, P, I, P, P, P]),
    "tg_raster_tta_reduce": (I, [P, P, I, I, I, I, P, P, P]),
    "tg_raster_blend_tta": (I, [P, P, RP, I, F, P, P, P, P, P, I, P, P, P, P]),
    "tg_hole_masks": (I, [P, P, I, I, P, P]),
    "tg_raster_sample": (I, [P, I64, I64, P, I, I, P, I, P, P, P, P]),
    "tg_objmask_known": (I, [P, P, I, I, I, F, P, P, P]),
    "tg_objmask_morph": (I, [P, P, I, I, I, I, P, P, P]),
    "tg_objmask_pmf_step": (I, [P, P, P, I, I, I, F, P, P, P, P, P]),
    "tg_objmask_components": (I, [P, I, I, P, P, P]),
    "tg_objmask_filter": (I, [P, P, P, I, I, I, I, P, P, P, P]),
    "tg_eval_holes": (I, [P, P, I, F, P, P, P, P, I, I, I, I, I, P, P, P, P]),
    "tg_hole_table": (I, [P, P, I, I, P, P, I, P, P]),
    "tg_terrain_errors_ws_bytes": (SZ, [I, I]),
    "tg_terrain_errors": (I, [P, P, P, I, F, P, P, P, P, P, I, I, I, D, C.POINTER(TgAreaClasses), P, P, P, P, SZ, P]),
    "tg_terrain_errors_finish": (I, [I, I, P, SZ, P, P]),
    "tg_select_f32_ws_bytes": (SZ, [I64, I]),
    "tg_select_f32": (I, [P, I64, P, I, P, P, SZ, P]),
    "tg_vfill_ws_bytes": (SZ, [I, I]),
    "tg_vfill_levels": (I, [I, I]),
    "tg_vfill_setup": (I, [P, P, I, F, I, I, P, SZ, P, P]),
    "tg_vfill_cycle": (I, [I, I, P, SZ, P, P]),
    "tg_vfill_finish": (I, [P, I, I, P, SZ, P, P]),
    "tg_vfill_pcg_ws_bytes": (SZ, [I, I]),
    "tg_vfill_pcg_start": (I, [I, I, P, SZ, P, SZ, P]),
    "tg_vfill_pcg_iter": (I, [I, I, P, SZ, P, SZ, P, P, P]),
    "tg_vfill_bih_ws_bytes": (SZ, [I, I]),
    "tg_vfill_bih_start": (I, [I, I, P, SZ, P, SZ, I, P]),
    "tg_vfill_bih_iter": (I, [I, I, P, SZ, P, SZ, I, P, P, P]),
    "tg_seam_delta": (I, [P, P, I, F, P, I, I, I, P, P, P]),
    "tg_seam_apply": (I, [P, P, I, F, P, P, I, I, P, P]),
    "tg_resample_area": (I, [P, P, I, F, I, I, I, I, I, I, P, P, I, F, I, I, P, P, P, P]),
    "tg_resample_interp": (I, [P, P, I, F, I, I, I, I, P, P, I, F, I, I, P, P, P, P]),
    "tg_edt_ws_bytes": (SZ, [I, I]),
    "tg_edt": (I, [P, I, I, C.c_int32, D, P, P, P, SZ, P]),
    "tg_depth_errors_ws_bytes": (SZ, [I, I]),
    "tg_depth_errors": (I, [P, P, P, P, I, I, I, C.POINTER(TgDepthClasses), P, P, P, P, SZ, P]),
    "tg_depth_errors_finish": (I, [I, I, P, SZ, P, P]),
    "tg_edt_nearest_ws_bytes": (SZ, [I, I]),
    "tg_edt_nearest": (I, [P, I, I, C.c_int32, P, P, P, SZ, P]),
    "tg_rayfill_ws_bytes": (SZ, [I, I]),
    "tg_rayfill": (I, [P, P, I, I, C.c_int32, D, P, P, P, P, P, P, SZ, P]),
    "tg_gather_fill": (I, [P, P, P, I, I, P, P, P]),
    "tg_void_smooth": (I, [P, P, I, I, P, P]),
    "tg_natural_fill_ws_bytes": (SZ, [I, I]),
    "tg_natural_tile_maxima": (I, [P, I, I, I, P, SZ, P]),
    "tg_natural_fill": (I, [P, P, P, I, I, I, C.c_int32, P, P, P, P, SZ, P]),
    "tg_depfill_ws_bytes": (SZ, [I, I]),
    "tg_depfill_init": (I, [P, P, I, I, I, P, P, SZ, P]),
    "tg_depfill_sweep": (I, [P, P, I, I, I, I, P, P, P, P, SZ, P]),
    "tg_depfill_stats": (I, [P, P, P, P, I, I, P, P, P, SZ, P]),
    "tg_depfill_finish": (I, [P, P, P, I, I, P, P, P, P]),
    "tg_flow_ws_bytes": (SZ, [I, I]),
    "tg_flow_slope": (I, [P, P, I, I, P, P, P, P, SZ, P]),
    "tg_flow_flat_sweep": (I, [P, I, I, I, P, P, P, P, SZ, P]),
    "tg_flow_flat_dir": (I, [P, P, I, I, P, P, P]),
    "tg_flow_accum_init": (I, [P, I, I, P, SZ, P]),
    "tg_flow_accum": (I, [I, I, I, I, P, P, SZ, P]),
    "tg_flow_accum_finish": (I, [I, I, I, P, P, P, SZ, P]),
    "tg_flow_basin_ws_bytes": (SZ, [I, I]),
    "tg_flow_basin_init": (I, [P, P, I, I, P, P, SZ, P]),
    "tg_flow_basin": (I, [I, I, I, I, P, P, SZ, P]),
    "tg_flow_basin_finish": (I, [I, I, I, D, P, P, P, P, P, P, SZ, P]),
    "tg_flow_compare": (I, [P, P, P, P, P, P, P, P, P, I, I, C.c_int32, C.c_int32, P, P]),
    "tg_stream_class": (I, [P, P, I, I, C.c_int32, P, P, P, P, SZ, P]),
    "tg_stream_order": (I, [P, P, P, P, I, I, I, I, P, P, P]),
    "tg_stream_order_finish": (I, [P, P, P, I, I, P, P, P]),
    "tg_hand": (I, [P, P, P, P, I, I, P, P, P, P]),
    "tg_flood_compare": (I, [P, P, P, I, I, TgFloodStages, I, P, P]),
    "tg_mfd_ws_bytes": (SZ, [I, I]),
    "tg_mfd_setup": (I, [P, P, P, I, I, I, D, P, P, P, SZ, P]),
    "tg_mfd_sweep": (I, [P, I, I, I, D, I, P, P, P, SZ, P]),
    "tg_mfd_finish": (I, [P, P, I, I, P, P, P, SZ, P]),
    "tg_terrain_slope": (I, [P, P, I, I, F, P, P]),
    "tg_wetness": (I, [P, P, P, I, I, F, F, P, P]),
    "tg_wetness_compare": (I, [P, P, P, I, I, P, P, P, SZ, P]),
    "tg_texture_ws_bytes": (SZ, [I, I]),
    "tg_texture_compare": (I, [P, P, P, P, I, I, I, P, P, P, SZ, P]),
    "tg_variogram_ws_bytes": (SZ, [I, I]),
    "tg_variogram": (I, [P, P, I, I, I, P, P, P, SZ, P]),
    "tg_krige": (I, [P, P, P, I, I, D, I, D, D, D, P, P, P, P, P, P]),
    "tg_sim_field": (I, [P, I, I, I64, I64, P, I, F, C.c_uint32, C.c_uint32, P]),
    "tg_sim_combine": (I, [P, P, P, P, P, P, P, P, I, I, P]),
    "tg_sim_stats": (I, [P, P, P, P, P, I, I, I, P]),
    "tg_prof_enable": (I, [I]),
    "tg_prof_summary": (I, [I, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "tg_prof_dump": (I, [C.c_char_p]),
    "tg_prof_tag": (I, [C.c_char_p]),
    "tg_nchw_to_nhwc": (I, [P, I, I, I, I, P, P]),
    "tg_nhwc_to_nchw": (I, [P, I, I, I, I, P, P]),
}

_lib = None


def load():
    """Load the HIP library; fail loudly if it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TgError(f"{LIB_PATH} is missing: build it with `python terra-gan_amd/build.py` "
                          "(or __graft_entry__.build()); this framework has no CPU / eager fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise TgError(f"{what} failed (rc={rc}): {load().tg_last_error().decode()}")
