"""ctypes binding of the C ABI in include/relu_field.h (thr3ed_atom_amd/csrc/librelu_field_hip.so).

The library is the product: there is NO fallback.  ``load()`` raises when the shared object is
missing and every wrapper raises ``RuntimeError`` on a non-zero return code.
"""
import ctypes as C
import os
import subprocess
from typing import Optional

CSRC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
LIB_NAME = "librelu_field_hip.so"
LIB_PATH = os.environ.get("RF_LIB_PATH") or os.path.join(CSRC_DIR, LIB_NAME)  # RF_LIB_PATH: development builds (tools/)
SOURCES = ["relu_field_kernels.hip", "grid_kernels.hip", "ray_walk_kernels.hip", "ray_grad_kernels.hip", "mesh_kernels.hip", "image_kernels.hip", "vq_kernels.hip", "component_kernels.hip", "mesh_simplify_kernels.hip", "texture_kernels.hip", "mesh_raster_kernels.hip", "texture_views_kernels.hip", "texture_fit_kernels.hip", "mesh_fit_kernels.hip", "fusion_kernels.hip", "mesh_distance_kernels.hip", "mesh_distance_grad_kernels.hip", "mesh_sign_kernels.hip"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]

ABI_VERSION = 4  # RF_ABI_VERSION of include/relu_field.h (4: compact records + compacted sample cache, x-slab-major keys, brick ranges)

# enums of relu_field.h
DENSITY_MODES = {"relu": 0, "softplus": 1, "abs": 2, "identity": 3}
LAYOUTS = {"reference": 0, "split": 1, "bricked": 2}
FLAG_WHITE_BKGD = 1
FLAG_RENDER_DIFFUSE = 2
FLAG_AABB_SAMPLING = 4
FLAG_OCCUPANCY_SKIP = 8
FLAG_JITTER_KEYED = 16
ERR_UNSUPPORTED = -3  # RF_ERR_UNSUPPORTED
SSIM_PADDINGS = {"valid": 0, "same": 1}  # RF_SSIM_*
SSIM_WINDOW = 11
VQ_MAX_DIM, VQ_MAX_CODES = 64, 65536  # rf_vq_assign / rf_vq_centroids
COMPONENT_TILE = 8  # kComponentTile of csrc/component_kernels.hip: edge of the node tiles rf_label_components labels in LDS
CONNECTIVITIES = (6, 18, 26)  # rf_label_components
MESH_PLACEMENTS = {"quadric": 0, "mean": 1}  # RF_MESH_PLACEMENT_*
MESH_MAX_CELLS = 1 << 20  # per axis (rf_mesh_cluster_keys)
MESH_CLUSTER_GROUP, MESH_CLUSTERS_PER_BLOCK, MESH_LONG_SEGMENT = 16, 16, 256  # kClusterGroup, kClustersPerBlock, kLongSegment of csrc/mesh_simplify_kernels.hip
TEXTURE_MIN_PATCH, TEXTURE_MAX_PATCH, TEXTURE_GUTTER, TEXTURE_MAX_SAMPLES, TEXTURE_MAX_EDGE = 2, 64, 4, 256, 16384  # rf_texture_bake (csrc/texture_kernels.hip; the edge: kMaxImageEdge of csrc/view_camera.h): block edge = patch + gutter
RASTER_CULL_BACKFACES = 32  # RF_RASTER_CULL_BACKFACES
RASTER_MAX_EDGE, RASTER_LANE_BOX = 16384, 8  # kMaxImageEdge of csrc/view_camera.h, kLaneBox of csrc/mesh_raster.h
TEXTURE_VIEWS_TWO_SIDED = 64  # RF_TEXTURE_VIEWS_TWO_SIDED
TEXTURE_VIEWS_MAX_VIEWS, TEXTURE_VIEWS_MAX_COS_POWER = 16, 8  # kMaxViews of csrc/view_camera.h, kMaxCosPower of csrc/texture_views_kernels.hip: views per rf_texture_project_views call
TEXTURE_FIT_LONG_SEGMENT, TEXTURE_NO_TAP = 16, 0xFFFF  # kLongSegment, kNoTap of csrc/texture_fit_kernels.hip: longer segments of rf_texture_sample_backward go to the wavefront
FUSE_CARVE = 128  # RF_FUSE_CARVE
FUSE_MAX_VIEWS, FUSE_MAX_DIM = 16, 4096  # kMaxViews of csrc/view_camera.h, kMaxDim of csrc/fusion_kernels.hip: views per rf_fuse_depth_views call, nodes per axis
MESH_DISTANCE_MAX_CELLS, MESH_DISTANCE_WIDE_FACE, MESH_DISTANCE_MAX_TABLE, MESH_DISTANCE_LANE_RINGS = 1024, 64, 1 << 25, 2  # kMaxGridCells, kWideFace, kMaxTable, kLaneRings of csrc/mesh_distance_kernels.hip: cells per axis, cells of a face box from which the wavefront writes its pairs, cells of a lattice, shells a lane walks before the wavefront takes its query
MESH_FIT_LONG_SEGMENT = 16  # kLongSegment of csrc/mesh_fit_kernels.hip: longer segments of rf_mesh_geometry_backward_gather go to the wavefront
SSIM_TILE = (16, 32)  # map rows x columns per workgroup of rf_ssim_forward (image rows x columns of rf_ssim_backward)
STEP_FORWARD = 1
STEP_EMIT = 2
STEP_BRICKS = 4
STEP_EMIT_SPECULAR = 8
STEP_EMIT_DIFFUSE = 16
STEP_SELECT_AND_DIFFUSE_FORWARD = 32
STEP_SPECULAR_FORWARD_AND_LOSSES = 64
STEP_DIFFUSE_CHAIN = 128  # selection + render_diffuse forward + its loss/offsets + its adjoint (reads the base tensor only)
STEP_SPECULAR_FORWARD = 256  # specular forward + its loss/offsets

EXPORTED_SYMBOLS = [
    "rf_abi_version",
    "rf_abi_struct_size",
    "rf_error_string",
    "rf_cast_rays",
    "rf_cast_selected_rays",
    "rf_select_rays_and_pixels",
    "rf_ray_aabb_bounds",
    "rf_render_forward",
    "rf_frame_render_kernel",
    "rf_render_backward",
    "rf_render_backward_emit",
    "rf_expand_records",
    "rf_expanded_record_floats",
    "rf_bin_offsets",
    "rf_render_backward_emit_direct",
    "rf_scatter_records",
    "rf_brick_accumulate",
    "rf_brick_accumulate_adam",
    "rf_brick_accumulate_adam_mirror",
    "rf_brick_accumulate_adam_range",
    "rf_brick_accumulate_adam_split",
    "rf_brick_split_scratch_bytes",
    "rf_grid_query",
    "rf_grid_query_backward",
    "rf_grid_query_backward_points",
    "rf_render_backward_rays",
    "rf_build_occupancy",
    "rf_upsample_grid",
    "rf_convert_grid",
    "rf_tv_grad",
    "rf_node_max_weight",
    "rf_prune_grid",
    "rf_node_bounds",
    "rf_resample_grid",
    "rf_distortion",
    "rf_render_geometry",
    "rf_l1_loss_grad",
    "rf_adam_step",
    "rf_train_step",
    "rf_render_forward_pair",
    "rf_l1_loss_grad_pair",
    "rf_bin_offsets_pair",
    "rf_render_backward_emit_direct_pair",
    "rf_step_kernel_specialised",
    "rf_mesh_tiles",
    "rf_mesh_count",
    "rf_mesh_emit",
    "rf_ssim_tiles",
    "rf_ssim_forward",
    "rf_ssim_backward",
    "rf_vq_assign",
    "rf_vq_centroids",
    "rf_label_components",
    "rf_mesh_cluster_keys",
    "rf_mesh_cluster_vertices",
    "rf_texture_bake",
    "rf_mesh_raster_visibility",
    "rf_mesh_raster_shade",
    "rf_texture_project_views",
    "rf_mesh_raster_taps",
    "rf_texture_sample",
    "rf_texture_sample_backward",
    "rf_mesh_raster_coverage",
    "rf_mesh_geometry_backward_pixels",
    "rf_mesh_geometry_backward_gather",
    "rf_fuse_depth_views",
    "rf_mesh_grid_pairs",
    "rf_mesh_closest_points",
    "rf_mesh_closest_gradients",
]

EXT_ABI_VERSION = 1  # RF_EXT_ABI_VERSION of include/relu_field_ext.h
# The list above is closed (include/relu_field.h is frozen with it): entry points added from here on are declared in
# include/relu_field_ext.h and listed here.
EXTENSION_SYMBOLS = [
    "rf_ext_abi_version",
    "rf_mesh_face_pseudonormals",
    "rf_mesh_signed_distance",
]


class RFGrid(C.Structure):
    _fields_ = [
        ("densities_dev", C.c_void_p),
        ("features_dev", C.c_void_p),
        ("dims", C.c_int32 * 3),
        ("num_features", C.c_int32),
        ("density_stride", C.c_int64),
        ("feature_stride", C.c_int64),
        ("aabb_min", C.c_float * 3),
        ("aabb_max", C.c_float * 3),
        ("norm_scale", C.c_float * 3),
        ("norm_bias", C.c_float * 3),
        ("density_scale", C.c_float),
        ("density_mode", C.c_int32),
        ("layout", C.c_int32),
        ("occupancy_dev", C.c_void_p),
    ]


class RFCamera(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("focal", C.c_float), ("pose", C.c_float * 12)]


class RFRayBatch(C.Structure):
    _fields_ = [
        ("origins_dev", C.c_void_p),
        ("directions_dev", C.c_void_p),
        ("num_rays", C.c_int64),
        ("num_samples", C.c_int32),
        ("near", C.c_float),
        ("far", C.c_float),
        ("t_vals_dev", C.c_void_p),
        ("t_rand_dev", C.c_void_p),
        ("jitter_key", C.c_uint64),
        ("first_ray", C.c_int64),
        ("camera", C.POINTER(RFCamera)),
    ]


class RFRenderOut(C.Structure):
    _fields_ = [
        ("colour_dev", C.c_void_p),
        ("depth_dev", C.c_void_p),
        ("acc_dev", C.c_void_p),
        ("disparity_dev", C.c_void_p),
        ("sample_cache_dev", C.c_void_p),
        ("trans_cache_dev", C.c_void_p),
        ("stop_cache_dev", C.c_void_p),
        ("chunk_mask_dev", C.c_void_p),
        ("key_hist_dev", C.c_void_p),
        ("brick_size", C.c_int32),
    ]


class RFRenderGrads(C.Structure):
    _fields_ = [
        ("grad_colour_dev", C.c_void_p),
        ("grad_depth_dev", C.c_void_p),
        ("grad_acc_dev", C.c_void_p),
    ]


class RFBrickList(C.Structure):
    _fields_ = [
        ("records_sorted_dev", C.c_void_p),
        ("offsets_dev", C.c_void_p),
        ("render_diffuse", C.c_int32),
    ]


class RFAdamState(C.Structure):
    _fields_ = [
        ("param_first_dev", C.c_void_p),
        ("param_second_dev", C.c_void_p),
        ("exp_avg_first_dev", C.c_void_p),
        ("exp_avg_second_dev", C.c_void_p),
        ("exp_avg_sq_first_dev", C.c_void_p),
        ("exp_avg_sq_second_dev", C.c_void_p),
        ("lr", C.c_float),
        ("beta1", C.c_float),
        ("beta2", C.c_float),
        ("eps", C.c_float),
        ("step", C.c_int32),
    ]


class RFRaySelection(C.Structure):
    _fields_ = [
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("focal", C.c_float),
        ("poses_dev", C.c_void_p),
        ("image_ids_dev", C.c_void_p),
        ("num_batch_images", C.c_int32),
        ("pixel_table_dev", C.c_void_p),
        ("key", C.c_uint64),
        ("first_index", C.c_int64),
    ]


class RFPassScratch(C.Structure):
    _fields_ = [
        ("out", RFRenderOut),
        ("grad_colour_dev", C.c_void_p),
        ("cursor_dev", C.c_void_p),
        ("offsets_dev", C.c_void_p),
        ("records_sorted_dev", C.c_void_p),
        ("t_rand_dev", C.c_void_p),
        ("jitter_key", C.c_uint64),
    ]


class RFTrainStep(C.Structure):
    _fields_ = [
        ("select", C.POINTER(RFRaySelection)),
        ("origins_dev", C.c_void_p),
        ("directions_dev", C.c_void_p),
        ("pixels_dev", C.c_void_p),
        ("num_rays", C.c_int64),
        ("num_samples", C.c_int32),
        ("near", C.c_float),
        ("far", C.c_float),
        ("t_vals_dev", C.c_void_p),
        ("flags", C.c_uint32),
        ("pass_", RFPassScratch * 2),
        ("loss_sums_dev", C.c_void_p),
        ("adam", C.POINTER(RFAdamState)),
        ("grad_first_dev", C.c_void_p),
        ("grad_second_dev", C.c_void_p),
        ("first_ray", C.c_int64),
        ("phases", C.c_uint32),
        ("loss_scale", C.c_float),
        ("timing_events", C.POINTER(C.c_void_p)),
    ]


class RFGeometryOut(C.Structure):
    _fields_ = [("normal_dev", C.c_void_p), ("quantile_depth_dev", C.c_void_p), ("acc_dev", C.c_void_p)]


class RFImage(C.Structure):
    _fields_ = [("data_dev", C.c_void_p), ("stride_h", C.c_int64), ("stride_w", C.c_int64), ("stride_c", C.c_int64)]


TRAIN_STEP_EVENTS = 11
def train_step_pairing():
    """(forward renders paired, emit launches paired): rf_train_step runs both renders of an iteration -- and both adjoints -- in ONE
    launch each unless $RF_FWD_PAIR / $RF_EMIT_PAIR say 0 (the library reads the same variables); the first slot of a pair then holds
    the launch and the second one is empty."""
    return os.environ.get("RF_FWD_PAIR", "1") != "0", os.environ.get("RF_EMIT_PAIR", "1") != "0"


TRAIN_STEP_EVENT_NAMES = ["select_rays_and_pixels", "render_forward[spec,save]", "(no launch: loss slot of the first render)", "render_forward[diffuse,save]",
                          "l1_loss_grad+bin_offsets[both]", "(no launch: offsets slot)", "render_backward_emit_direct[spec]",
                          "(no launch: offsets slot of the second list)", "render_backward_emit_direct[diffuse]", "brick_accumulate"]


# order of rf_abi_struct_size(which)
ABI_STRUCTS = [RFGrid, RFRayBatch, RFRenderOut, RFRenderGrads, RFBrickList, RFAdamState, RFCamera, RFRaySelection, RFPassScratch, RFTrainStep, RFGeometryOut, RFImage]


def build_inputs():
    """Every file whose modification makes the library stale: the units of SOURCES, every private header of csrc/, the two public headers."""
    headers = sorted(f for f in os.listdir(CSRC_DIR) if f.endswith(".h"))
    return [os.path.join(CSRC_DIR, f) for f in SOURCES + headers] + [os.path.join(INCLUDE_DIR, "relu_field.h"), os.path.join(INCLUDE_DIR, "relu_field_ext.h")]


def build(force: bool = False, verbose: bool = False) -> str:
    """Cross-compile the HIP sources for gfx950 into csrc/librelu_field_hip.so (hipcc needs no GPU)."""
    srcs = [os.path.join(CSRC_DIR, s) for s in SOURCES]
    if not force and os.path.exists(LIB_PATH):
        if os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(d) for d in build_inputs()):
            return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + HIPCC_FLAGS + ["-I", INCLUDE_DIR] + srcs + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


_LIB: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the HIP library; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP render library has not been built. "
            f"Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            f"There is no CPU fallback for the render path."
        )
    lib = C.CDLL(LIB_PATH)
    lib.rf_abi_version.restype = C.c_int
    lib.rf_error_string.restype = C.c_char_p
    lib.rf_error_string.argtypes = [C.c_int]
    vp, i32, i64, f32, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint32
    fp = C.POINTER(C.c_float)
    lib.rf_cast_rays.argtypes = [i32, i32, f32, fp, fp, vp, vp, vp]
    lib.rf_cast_selected_rays.argtypes = [i32, i32, f32, vp, i32, vp, i64, vp, vp, vp]
    lib.rf_select_rays_and_pixels.argtypes = [i32, i32, f32, vp, vp, i32, vp, C.c_uint64, i64, i64, vp, vp, vp, vp, vp]
    lib.rf_ray_aabb_bounds.argtypes = [vp, vp, i64, f32, f32, fp, fp, vp, vp, vp]
    lib.rf_render_forward.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), u32, C.POINTER(RFRenderOut), vp]
    lib.rf_frame_render_kernel.argtypes = [C.POINTER(RFGrid), C.POINTER(RFCamera), u32]
    lib.rf_render_backward.argtypes = [
        C.POINTER(RFGrid),
        C.POINTER(RFRayBatch),
        u32,
        C.POINTER(RFRenderOut),
        C.POINTER(RFRenderGrads),
        vp,
        vp,
        vp,
    ]
    lib.rf_render_backward_emit.argtypes = [
        C.POINTER(RFGrid), C.POINTER(RFRayBatch), u32, C.POINTER(RFRenderOut), C.POINTER(RFRenderGrads), i32, vp, vp, vp, vp,
    ]
    lib.rf_expand_records.argtypes = [C.POINTER(RFGrid), vp, vp, vp, i64, i32, vp, vp]
    lib.rf_expanded_record_floats.argtypes = [i32]
    lib.rf_expanded_record_floats.restype = i32
    lib.rf_bin_offsets.argtypes = [vp, i32, vp, vp, vp]
    lib.rf_render_backward_emit_direct.argtypes = [
        C.POINTER(RFGrid), C.POINTER(RFRayBatch), u32, C.POINTER(RFRenderOut), C.POINTER(RFRenderGrads), i32, vp, vp, vp, vp,
    ]
    lib.rf_scatter_records.argtypes = [C.POINTER(RFGrid), vp, vp, i64, vp, i32, vp, vp, i32, vp]
    lib.rf_brick_accumulate.argtypes = [C.POINTER(RFGrid), i32, C.POINTER(RFBrickList), i32, vp, vp, i32, vp]
    lib.rf_brick_accumulate_adam.argtypes = [C.POINTER(RFGrid), i32, C.POINTER(RFBrickList), i32, C.POINTER(RFAdamState), vp]
    lib.rf_brick_accumulate_adam_range.argtypes = [C.POINTER(RFGrid), i32, C.POINTER(RFBrickList), i32, C.POINTER(RFAdamState), i32, i32, vp]
    lib.rf_brick_accumulate_adam_mirror.argtypes = [C.POINTER(RFGrid), i32, C.POINTER(RFBrickList), i32, C.POINTER(RFAdamState), vp, vp, vp]
    lib.rf_brick_accumulate_adam_split.argtypes = [C.POINTER(RFGrid), i32, C.POINTER(RFBrickList), i32, C.POINTER(RFAdamState), i32, i32, i32, vp, i64, vp]
    lib.rf_brick_split_scratch_bytes.argtypes = [C.POINTER(RFGrid), i32, i32]
    lib.rf_train_step.argtypes = [C.POINTER(RFGrid), C.POINTER(RFTrainStep), vp]
    lib.rf_grid_query.argtypes = [C.POINTER(RFGrid), vp, i64, vp, vp]
    lib.rf_grid_query_backward.argtypes = [C.POINTER(RFGrid), vp, i64, vp, vp, vp, vp]
    lib.rf_grid_query_backward_points.argtypes = [C.POINTER(RFGrid), vp, i64, vp, vp, vp]
    lib.rf_render_backward_rays.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), u32, C.POINTER(RFRenderOut), C.POINTER(RFRenderGrads), vp, vp, vp]
    lib.rf_upsample_grid.argtypes = [C.POINTER(RFGrid), C.POINTER(RFGrid), vp]
    lib.rf_convert_grid.argtypes = [C.POINTER(RFGrid), C.POINTER(RFGrid), vp]
    lib.rf_tv_grad.argtypes = [C.POINTER(RFGrid), f32, f32, f32, vp, vp, vp, vp]
    lib.rf_node_max_weight.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), u32, vp, vp]
    lib.rf_prune_grid.argtypes = [C.POINTER(RFGrid), vp, f32, i32, f32, vp, vp, vp, vp]
    lib.rf_node_bounds.argtypes = [C.POINTER(RFGrid), f32, vp, vp, vp]
    lib.rf_resample_grid.argtypes = [C.POINTER(RFGrid), C.POINTER(RFGrid), fp, fp, f32, vp]
    lib.rf_distortion.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), u32, f32, vp, vp, vp, vp]
    lib.rf_render_geometry.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), u32, f32, C.POINTER(RFGeometryOut), vp]
    lib.rf_build_occupancy.argtypes = [C.POINTER(RFGrid), f32, vp, vp]
    lib.rf_l1_loss_grad.argtypes = [vp, vp, i64, f32, vp, vp, vp]
    lib.rf_adam_step.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, i32, i32, vp]
    # the paired entry points: every array argument holds two entries ([0] specular, [1] render_diffuse)
    lib.rf_render_forward_pair.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), C.POINTER(u32), C.POINTER(RFRenderOut), vp]
    lib.rf_l1_loss_grad_pair.argtypes = [C.POINTER(vp), vp, i64, f32, C.POINTER(vp), vp, vp, vp]
    lib.rf_bin_offsets_pair.argtypes = [C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(vp), vp]
    lib.rf_render_backward_emit_direct_pair.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), C.POINTER(u32), C.POINTER(RFPassScratch), vp]
    lib.rf_step_kernel_specialised.argtypes = [C.POINTER(RFGrid), C.POINTER(RFRayBatch), C.POINTER(u32)]
    # iso-surface extraction (csrc/mesh_kernels.hip)
    lib.rf_mesh_tiles.argtypes = [C.POINTER(RFGrid), i32]
    lib.rf_mesh_count.argtypes = [C.POINTER(RFGrid), i32, f32, vp, vp]
    lib.rf_mesh_emit.argtypes = [C.POINTER(RFGrid), i32, f32, vp, i64, i64, vp, vp, vp, vp, vp, vp]
    # image metrics (csrc/image_kernels.hip)
    lib.rf_ssim_tiles.argtypes = [i32, i32, i32, i32]
    lib.rf_ssim_forward.argtypes = [C.POINTER(RFImage), C.POINTER(RFImage), i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.rf_ssim_backward.argtypes = [C.POINTER(RFImage), C.POINTER(RFImage), i32, i32, i32, i32, vp, vp, C.POINTER(RFImage), vp]
    # vector quantisation (csrc/vq_kernels.hip)
    lib.rf_vq_assign.argtypes = [vp, i64, i32, i64, vp, i32, vp, vp, vp]
    lib.rf_vq_centroids.argtypes = [vp, i64, i32, vp, vp, vp, i32, vp, vp, vp]
    # connected components (csrc/component_kernels.hip)
    lib.rf_label_components.argtypes = [C.POINTER(RFGrid), f32, i32, vp, vp, vp]
    # mesh simplification (csrc/mesh_simplify_kernels.hip)
    i32p = C.POINTER(i32)
    lib.rf_mesh_cluster_keys.argtypes = [vp, i64, fp, f32, i32p, vp, vp, vp]
    lib.rf_mesh_cluster_vertices.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, fp, f32, i32p, i32, f32, vp, vp, vp, vp]
    # texture baking (csrc/texture_kernels.hip)
    lib.rf_texture_bake.argtypes = [C.POINTER(RFGrid), vp, i64, vp, i64, i32, i32, i32, f32, i32, u32, vp, vp, vp, vp]
    # mesh rasteriser (csrc/mesh_raster_kernels.hip)
    lib.rf_mesh_raster_visibility.argtypes = [C.POINTER(RFCamera), vp, i64, vp, i64, f32, u32, vp, vp, vp]
    lib.rf_mesh_raster_shade.argtypes = [C.POINTER(RFCamera), vp, i64, vp, i64, vp, vp, vp, i32, i32, vp, u32, vp, vp, vp, vp, vp]
    # texture baking from posed views (csrc/texture_views_kernels.hip)
    lib.rf_texture_project_views.argtypes = [vp, i64, vp, i64, i32, i32, i32, i32, C.POINTER(RFCamera), vp, vp, vp, f32, f32, f32, i32, f32, u32, vp, vp, vp, vp]
    # texture gradients of the mesh render (csrc/mesh_raster_kernels.hip, csrc/texture_fit_kernels.hip)
    lib.rf_mesh_raster_taps.argtypes = [C.POINTER(RFCamera), vp, i64, vp, i64, vp, vp, i32, i32, u32, vp, vp]
    lib.rf_texture_sample.argtypes = [vp, i64, vp, i32, i32, f32, u32, vp, vp, vp]
    lib.rf_texture_sample_backward.argtypes = [vp, i64, vp, vp, i64, i32, i32, i32, u32, vp, vp, vp]
    # geometry gradients of the mesh render (csrc/mesh_fit_kernels.hip)
    lib.rf_mesh_raster_coverage.argtypes = [C.POINTER(RFCamera), vp, i64, vp, i64, vp, u32, vp, vp, vp, vp]
    lib.rf_mesh_geometry_backward_pixels.argtypes = [C.POINTER(RFCamera), vp, i64, vp, i64, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.rf_mesh_geometry_backward_gather.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i64, i32, u32, vp, vp, vp, vp]
    # TSDF fusion of posed depth views (csrc/fusion_kernels.hip)
    lib.rf_fuse_depth_views.argtypes = [fp, fp, i32p, i32, C.POINTER(RFCamera), vp, vp, vp, f32, f32, f32, u32, vp, vp, vp, vp]
    # closest points on a mesh (csrc/mesh_distance_kernels.hip)
    lib.rf_mesh_grid_pairs.argtypes = [vp, i64, vp, i64, fp, f32, i32p, vp, i64, vp, vp, vp, vp]
    lib.rf_mesh_closest_points.argtypes = [vp, i64, vp, i64, fp, f32, i32p, vp, vp, i64, vp, vp, i64, f32, u32, vp, vp, vp, vp, vp, vp]
    # gradients of the distance to a mesh (csrc/mesh_distance_grad_kernels.hip)
    lib.rf_mesh_closest_gradients.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, u32, vp, vp, vp, vp, vp, vp]
    # the sign of the distance to a closed mesh (csrc/mesh_sign_kernels.hip; include/relu_field_ext.h)
    lib.rf_ext_abi_version.argtypes = []
    lib.rf_mesh_face_pseudonormals.argtypes = [vp, i64, vp, i64, u32, vp, vp, vp, vp]
    lib.rf_mesh_signed_distance.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, i64, u32, vp, vp, vp, vp, vp]
    for name in EXTENSION_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    if lib.rf_ext_abi_version() != EXT_ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: extension ABI version {lib.rf_ext_abi_version()} != {EXT_ABI_VERSION} (stale build? run __graft_entry__.build())")
    for name in EXPORTED_SYMBOLS:
        if name not in ("rf_error_string",):
            getattr(lib, name).restype = C.c_int64 if name in ("rf_brick_split_scratch_bytes", "rf_mesh_tiles", "rf_ssim_tiles") else C.c_int
    if lib.rf_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: ABI version {lib.rf_abi_version()} != {ABI_VERSION} (stale build? run __graft_entry__.build())")
    lib.rf_abi_struct_size.argtypes = [C.c_int]
    for which, mirror in enumerate(ABI_STRUCTS):
        if lib.rf_abi_struct_size(which) != C.sizeof(mirror):
            raise RuntimeError(f"{LIB_PATH}: sizeof({mirror.__name__}) is {lib.rf_abi_struct_size(which)} in the library, {C.sizeof(mirror)} in the binding")
    _LIB = lib
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().rf_error_string(code).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {code})")


def float3(values):
    return (C.c_float * 3)(*[float(v) for v in values])
