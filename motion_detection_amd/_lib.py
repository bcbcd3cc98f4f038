"""ctypes binding of libmdx.so (the C-ABI declared in include/mdx.h).

The library is built in-tree (motion_detection_amd/lib/libmdx.so) by
``motion_detection_amd.build()`` / ``__graft_entry__.build()``.  There is no CPU or
PyTorch fallback: if the library is missing, importing the compute API raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmdx.so")
# developer hook: load an alternative build (e.g. scripts/lk_variants.sh timing-only variants)
if os.environ.get("MDX_LIB_PATH"):
    LIB_PATH = os.environ["MDX_LIB_PATH"]
CSRC = os.path.join(_HERE, "csrc")

MDX_OK = 0
MDX_EINVAL = -1
MDX_EHIP = -2
MDX_ENOMEM = -3
MDX_EDEGENERATE = 1

FMT_GRAY8, FMT_RGB8, FMT_BGR8 = 0, 1, 2
FIT_FIRST4, FIT_EXTERNAL, FIT_RANSAC = 0, 1, 2
SUBSPACE_F64, SUBSPACE_F32 = 0, 1
CLUSTER_MAX_POINTS = 262144   # include/mdx.h MDX_CLUSTER_MAX_POINTS
REGIONS_OPEN3 = 1             # include/mdx.h MDX_REGIONS_OPEN3
VCLUSTER_ABS_INT = 1          # include/mdx.h MDX_VCLUSTER_ABS_INT
VCLUSTER_MAX_POINTS = 131072  # include/mdx.h MDX_VCLUSTER_MAX_POINTS
OUTLIERS_INCLUDE_ZEROS = 1    # include/mdx.h MDX_OUTLIERS_INCLUDE_ZEROS
OUTLIERS_MAX_POINTS = 131072  # include/mdx.h MDX_OUTLIERS_MAX_POINTS
HULL_MAX_SPAN = 8192          # include/mdx.h MDX_HULL_MAX_SPAN
REGION_NO_PARENT = -1         # include/mdx.h MDX_REGION_NO_PARENT
REGION_PARENT_UNKNOWN = -2    # include/mdx.h MDX_REGION_PARENT_UNKNOWN
BG_MAX_MIXTURES = 8           # include/mdx.h MDX_BG_MAX_MIXTURES
BG_MAX_FRAMES_PER_LAUNCH = 32  # include/mdx.h MDX_BG_MAX_FRAMES_PER_LAUNCH

# every symbol include/mdx.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "mdx_default_params", "mdx_grid_count", "mdx_create", "mdx_create_error", "mdx_destroy",
    "mdx_last_error", "mdx_set_params", "mdx_get_params", "mdx_stream", "mdx_device", "mdx_sync",
    "mdx_device_sync",
    "mdx_flow_warp_diff", "mdx_flow_warp_diff_batch_dev", "mdx_warp_diff_dev", "mdx_dev_alloc",
    "mdx_dev_free", "mdx_memcpy_h2d", "mdx_memcpy_d2h", "mdx_enable_timing", "mdx_timing_calls", "mdx_stage_ms",
    "mdx_synth_pair", "mdx_debug_copy", "mdx_band_flow_dev", "mdx_band_fit_warp_dev", "mdx_flow_trajectory",
    "mdx_srand", "mdx_rand", "mdx_fit_subspace", "mdx_device_pci", "mdx_build_info",
    "mdx_ring_push", "mdx_ring_trajectory", "mdx_ring_reset", "mdx_input_ready",
    "mdx_host_alloc", "mdx_host_free", "mdx_probe_stream3_dev", "mdx_lk_fallbacks",
    "mdx_debug_div32", "mdx_debug_warp_paths", "mdx_trajectory_layout", "mdx_abi_version", "mdx_params_size",
    "mdx_cluster_euclidean", "mdx_mask_regions_dev", "mdx_mask_regions", "mdx_cluster_vectors",
    "mdx_find_outliers", "mdx_half_size", "mdx_resize_half_dev", "mdx_resize_half", "mdx_ring_push_half",
    "mdx_cluster_hulls", "mdx_region_hulls_dev", "mdx_mask_region_hulls",
    "mdx_region_parents_dev", "mdx_mask_regions_tree", "mdx_region_outlines_dev", "mdx_mask_region_outlines",
    "mdx_bg_default_params", "mdx_bg_params_size", "mdx_bg_create", "mdx_bg_destroy", "mdx_bg_reset", "mdx_bg_frames",
    "mdx_bg_apply_dev", "mdx_bg_image_dev", "mdx_bg_apply", "mdx_bg_image", "mdx_bg_get_state", "mdx_bg_set_state",
]
ABI_VERSION = 11  # include/mdx.h MDX_ABI_VERSION

# csrc/Makefile STAMPED: the files whose bytes the library's provenance stamp hashes, in order
STAMPED = ["Makefile", "mdx_plan.h", "mdx_internal.h", "mdx_ctx.h", "mdx_dev.h", "mdx_api.cpp", "mdx_pair.cpp", "mdx_traj.cpp",
           "mdx_post.cpp", "mdx_bg_api.cpp", "mdx_front.hip", "mdx_lk_point.hip", "mdx_fit.hip", "mdx_lk.hip", "mdx_warp.hip",
           "mdx_subspace.hip", "mdx_cluster.hip", "mdx_vcluster.hip", "mdx_outliers.hip", "mdx_regions.hip", "mdx_resize.hip", "mdx_hull.hip", "mdx_outline.hip", "mdx_bg.hip", "synth.cpp", os.path.join("..", "..", "include", "mdx.h")]


class MdxBandCand(C.Structure):
    """mdx_band_cand (include/mdx.h): one row band's accepted count and first four accepted points."""
    _fields_ = [("count", C.c_int32), ("n", C.c_int32), ("idx", C.c_int32 * 4), ("src", C.c_float * 8),
                ("dst", C.c_float * 8), ("pad_", C.c_int32 * 2)]


class MdxRandState(C.Structure):
    """mdx_rand_state (include/mdx.h): glibc rand() generator state."""
    _fields_ = [("x", C.c_uint32 * 34), ("pos", C.c_int32)]


class MdxRegion(C.Structure):
    """mdx_region (include/mdx.h): one kept component of the labelled motion mask."""
    _fields_ = [(n, C.c_int32) for n in ("x", "y", "width", "height", "area", "seed_x", "seed_y", "id")]


class MdxOutlierStats(C.Structure):
    """mdx_outlier_stats (include/mdx.h): one field's counts and order statistics."""
    _fields_ = [("selected", C.c_int32), ("flagged_angle", C.c_int32), ("flagged_magnitude", C.c_int32),
                ("outliers", C.c_int32), ("median_angle", C.c_double), ("mad_angle", C.c_double),
                ("median_magnitude", C.c_double), ("mad_magnitude", C.c_double)]


class MdxBgParams(C.Structure):
    """mdx_bg_params (include/mdx.h): the mixture model's parameters, OpenCV 2.4's names."""
    _fields_ = [("history", C.c_int32), ("nmixtures", C.c_int32), ("var_threshold", C.c_float),
                ("var_threshold_gen", C.c_float), ("background_ratio", C.c_float), ("var_init", C.c_float),
                ("var_min", C.c_float), ("var_max", C.c_float), ("ct", C.c_float), ("detect_shadows", C.c_int32),
                ("shadow_value", C.c_int32), ("tau", C.c_float)]


BAND_CAND_BYTES = 96
assert C.sizeof(MdxBgParams) == 48
assert C.sizeof(MdxOutlierStats) == 48
assert C.sizeof(MdxRegion) == 32
assert C.sizeof(MdxBandCand) == BAND_CAND_BYTES


class MdxParams(C.Structure):
    _fields_ = [("win", C.c_int), ("max_level", C.c_int), ("max_iters", C.c_int), ("eps", C.c_double),
                ("min_eig", C.c_float), ("thresh", C.c_int), ("pixel_step", C.c_int),
                ("min_vector_size", C.c_double), ("fit_mode", C.c_int), ("subspace_precision", C.c_int),
                ("call_pipelining", C.c_int), ("ransac_iters", C.c_int), ("ransac_thresh", C.c_double),
                ("ransac_seed", C.c_uint32)]


class MdxError(RuntimeError):
    """Raised for every negative return code of the C-ABI."""


def build(force: bool = True) -> str:
    """Compile libmdx.so for gfx950 with hipcc (csrc/Makefile); force (default) rebuilds every
    object from the sources in the tree (make -B), up to 16 files at a time."""
    cmd = ["make", "-s", "-j%d" % min(16, os.cpu_count() or 1), "-C", CSRC] + (["-B"] if force else [])
    subprocess.run(cmd, check=True)
    return LIB_PATH


def source_sha256() -> str:
    """sha256 of the library's sources as csrc/Makefile stamps them into mdx_build_info()."""
    import hashlib
    h = hashlib.sha256()
    for f in STAMPED:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def build_info() -> dict:
    """The loaded library's provenance stamp, and whether it matches the sources in this tree."""
    raw = lib().mdx_build_info().decode()
    kv = dict(part.split("=", 1) for part in raw.split())
    kv["matches_tree"] = kv.get("src_sha256") == source_sha256()
    return kv


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MdxError(f"{LIB_PATH} is missing: build it with motion_detection_amd.build() "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u8p, f32p, f64p, i32p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    if hasattr(L, "mdx_abi_version"):
        L.mdx_abi_version.argtypes = []
        L.mdx_abi_version.restype = C.c_int
        L.mdx_params_size.argtypes = []
        L.mdx_params_size.restype = C.c_size_t
        if L.mdx_abi_version() != ABI_VERSION or L.mdx_params_size() != C.sizeof(MdxParams):
            raise MdxError(f"{LIB_PATH}: ABI {L.mdx_abi_version()} / mdx_params {L.mdx_params_size()} B, this binding "
                           f"expects ABI {ABI_VERSION} / {C.sizeof(MdxParams)} B (rebuild the library)")
    elif not os.environ.get("MDX_LIB_PATH"):
        # only developer A/B builds of older revisions (MDX_LIB_PATH) may predate ABI 4
        raise MdxError(f"{LIB_PATH} predates ABI 4 (no mdx_abi_version): rebuild the library")
    L.mdx_default_params.argtypes = [C.POINTER(MdxParams)]
    L.mdx_default_params.restype = None
    L.mdx_grid_count.argtypes = [C.c_int, C.c_int, C.c_int]
    L.mdx_grid_count.restype = C.c_int
    L.mdx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MdxParams)]
    L.mdx_create.restype = vp
    L.mdx_create_error.argtypes = []
    L.mdx_create_error.restype = C.c_char_p
    L.mdx_destroy.argtypes = [vp]
    L.mdx_destroy.restype = C.c_int
    L.mdx_last_error.argtypes = [vp]
    L.mdx_last_error.restype = C.c_char_p
    L.mdx_set_params.argtypes = [vp, C.POINTER(MdxParams)]
    L.mdx_set_params.restype = C.c_int
    L.mdx_get_params.argtypes = [vp, C.POINTER(MdxParams)]
    L.mdx_get_params.restype = C.c_int
    L.mdx_stream.argtypes = [vp]
    L.mdx_stream.restype = vp
    L.mdx_device.argtypes = [vp]
    L.mdx_device.restype = C.c_int
    L.mdx_sync.argtypes = [vp]
    L.mdx_sync.restype = C.c_int
    L.mdx_device_pci.argtypes = [vp, C.c_char_p, C.c_int]
    L.mdx_device_pci.restype = C.c_int
    L.mdx_build_info.argtypes = []
    L.mdx_build_info.restype = C.c_char_p
    L.mdx_device_sync.argtypes = [vp]
    L.mdx_device_sync.restype = C.c_int
    if hasattr(L, "mdx_input_ready"):      # (absent from variant builds of older sources: A/B runs)
        L.mdx_input_ready.argtypes = [vp, vp]
        L.mdx_input_ready.restype = C.c_int
    L.mdx_flow_warp_diff.argtypes = [vp, u8p, u8p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, u8p, f64p, u8p,
                                     f64p, f64p, C.POINTER(C.c_int)]
    L.mdx_flow_warp_diff.restype = C.c_int
    L.mdx_flow_warp_diff_batch_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                               vp, vp, vp, vp, vp, vp, vp]
    L.mdx_flow_warp_diff_batch_dev.restype = C.c_int
    L.mdx_warp_diff_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp]
    L.mdx_warp_diff_dev.restype = C.c_int
    if hasattr(L, "mdx_debug_div32"):
        L.mdx_debug_div32.argtypes = [vp, vp, vp, C.c_int]
        L.mdx_debug_div32.restype = C.c_int
    if hasattr(L, "mdx_debug_warp_paths"):
        L.mdx_debug_warp_paths.argtypes = [vp, vp, C.c_int]
        L.mdx_debug_warp_paths.restype = C.c_int
    if hasattr(L, "mdx_lk_fallbacks"):
        L.mdx_lk_fallbacks.argtypes = [vp, C.POINTER(C.c_longlong)]
        L.mdx_lk_fallbacks.restype = C.c_int
    if hasattr(L, "mdx_trajectory_layout"):
        L.mdx_trajectory_layout.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.mdx_trajectory_layout.restype = C.c_size_t
    if hasattr(L, "mdx_host_alloc"):
        L.mdx_host_alloc.argtypes = [C.c_size_t]
        L.mdx_host_alloc.restype = vp
        L.mdx_host_free.argtypes = [vp]
        L.mdx_host_free.restype = C.c_int
    if hasattr(L, "mdx_probe_stream3_dev"):
        L.mdx_probe_stream3_dev.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_int]
        L.mdx_probe_stream3_dev.restype = C.c_int
    L.mdx_dev_alloc.argtypes = [vp, C.c_size_t]
    L.mdx_dev_alloc.restype = vp
    L.mdx_dev_free.argtypes = [vp, vp]
    L.mdx_dev_free.restype = C.c_int
    L.mdx_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.mdx_memcpy_h2d.restype = C.c_int
    L.mdx_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.mdx_memcpy_d2h.restype = C.c_int
    L.mdx_enable_timing.argtypes = [vp, C.c_int]
    L.mdx_enable_timing.restype = C.c_int
    L.mdx_timing_calls.argtypes = [vp]
    L.mdx_timing_calls.restype = C.c_int
    L.mdx_stage_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.mdx_stage_ms.restype = C.c_int
    L.mdx_debug_copy.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.mdx_debug_copy.restype = C.c_int
    L.mdx_synth_pair.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, u8p, u8p, f64p, C.c_int]
    L.mdx_synth_pair.restype = C.c_int
    L.mdx_band_flow_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.mdx_band_flow_dev.restype = C.c_int
    L.mdx_band_fit_warp_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp]
    L.mdx_band_fit_warp_dev.restype = C.c_int
    L.mdx_flow_trajectory.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp,
                                      C.POINTER(C.c_int)]
    L.mdx_flow_trajectory.restype = C.c_int
    L.mdx_ring_push.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.mdx_ring_push.restype = C.c_int
    L.mdx_ring_push_half.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.mdx_ring_push_half.restype = C.c_int
    L.mdx_half_size.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mdx_half_size.restype = C.c_int
    L.mdx_resize_half_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, vp, C.c_int,
                                      C.c_size_t]
    L.mdx_resize_half_dev.restype = C.c_int
    L.mdx_resize_half.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    L.mdx_resize_half.restype = C.c_int
    L.mdx_ring_trajectory.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.mdx_ring_trajectory.restype = C.c_int
    L.mdx_ring_reset.argtypes = [vp]
    L.mdx_ring_reset.restype = C.c_int
    L.mdx_srand.argtypes = [C.POINTER(MdxRandState), C.c_uint32]
    L.mdx_srand.restype = None
    L.mdx_rand.argtypes = [C.POINTER(MdxRandState)]
    L.mdx_rand.restype = C.c_int
    L.mdx_fit_subspace.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(MdxRandState), vp, vp, vp,
                                   vp, C.POINTER(C.c_int)]
    L.mdx_fit_subspace.restype = C.c_int
    L.mdx_cluster_euclidean.argtypes = [vp, vp, C.c_int, C.c_double, C.c_int, vp, C.POINTER(C.c_int), vp, vp, C.c_int,
                                        C.POINTER(C.c_int)]
    L.mdx_cluster_euclidean.restype = C.c_int
    L.mdx_cluster_vectors.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.mdx_cluster_vectors.restype = C.c_int
    L.mdx_cluster_hulls.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.mdx_cluster_hulls.restype = C.c_int
    L.mdx_find_outliers.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.mdx_find_outliers.restype = C.c_int
    L.mdx_mask_regions_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, vp,
                                       C.c_int, vp, vp, vp, vp]
    L.mdx_mask_regions_dev.restype = C.c_int
    L.mdx_mask_regions.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp]
    L.mdx_mask_regions.restype = C.c_int
    L.mdx_region_hulls_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.mdx_region_hulls_dev.restype = C.c_int
    L.mdx_mask_region_hulls.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.mdx_mask_region_hulls.restype = C.c_int
    L.mdx_region_parents_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.mdx_region_parents_dev.restype = C.c_int
    L.mdx_mask_regions_tree.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int), vp, vp,
                                        C.c_int, C.POINTER(C.c_int)]
    L.mdx_mask_regions_tree.restype = C.c_int
    L.mdx_region_outlines_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp]
    L.mdx_region_outlines_dev.restype = C.c_int
    L.mdx_mask_region_outlines.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int), vp, vp,
                                           C.c_int, C.POINTER(C.c_int)]
    L.mdx_mask_region_outlines.restype = C.c_int
    L.mdx_bg_default_params.argtypes = [C.POINTER(MdxBgParams)]
    L.mdx_bg_default_params.restype = None
    L.mdx_bg_params_size.argtypes = []
    L.mdx_bg_params_size.restype = C.c_size_t
    L.mdx_bg_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MdxBgParams), C.POINTER(vp)]
    L.mdx_bg_create.restype = C.c_int
    for name in ("mdx_bg_destroy", "mdx_bg_reset", "mdx_bg_frames"):
        getattr(L, name).argtypes = [vp, vp]
        getattr(L, name).restype = C.c_int
    L.mdx_bg_apply_dev.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_double, vp]
    L.mdx_bg_apply_dev.restype = C.c_int
    L.mdx_bg_image_dev.argtypes = [vp, vp, vp]
    L.mdx_bg_image_dev.restype = C.c_int
    L.mdx_bg_apply.argtypes = [vp, vp, u8p, C.c_int, C.c_double, u8p]
    L.mdx_bg_apply.restype = C.c_int
    L.mdx_bg_image.argtypes = [vp, vp, u8p]
    L.mdx_bg_image.restype = C.c_int
    L.mdx_bg_get_state.argtypes = [vp, vp, C.c_int, f32p, f32p, f32p, u8p, C.POINTER(C.c_int)]
    L.mdx_bg_get_state.restype = C.c_int
    L.mdx_bg_set_state.argtypes = [vp, vp, C.c_int, f32p, f32p, f32p, u8p, C.c_int]
    L.mdx_bg_set_state.restype = C.c_int
    _lib = L
    return L


def default_params(**overrides) -> MdxParams:
    p = MdxParams()
    lib().mdx_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown parameter {k!r}")
        setattr(p, k, v)
    return p


def bg_default_params(**overrides) -> MdxBgParams:
    p = MdxBgParams()
    lib().mdx_bg_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown parameter {k!r}")
        setattr(p, k, v)
    return p
