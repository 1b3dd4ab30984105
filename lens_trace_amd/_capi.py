"""ctypes binding of liblenstrace-hip.so (include/lenstrace_hip.h).  There is NO fallback: if the library is
missing or a call fails, this raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LT_HIP_LIBRARY") or os.path.join(_HERE, "lib", "liblenstrace-hip.so")

(LT_OK, LT_ERR_INVALID_ARGUMENT, LT_ERR_NO_DEVICE, LT_ERR_HIP, LT_ERR_NO_SCENE, LT_ERR_BAD_SCENE,
 LT_ERR_BUFFER_TOO_SMALL, LT_ERR_UNKNOWN_PROGRAM) = range(8)
STATUS_NAMES = ["LT_OK", "LT_ERR_INVALID_ARGUMENT", "LT_ERR_NO_DEVICE", "LT_ERR_HIP", "LT_ERR_NO_SCENE",
                "LT_ERR_BAD_SCENE", "LT_ERR_BUFFER_TOO_SMALL", "LT_ERR_UNKNOWN_PROGRAM"]

PROGRAM_BASIC, PROGRAM_BASIC_LIGHTING, PROGRAM_ACCUMULATOR, PROGRAM_GLOBAL_ILLUMINATION, PROGRAM_GLOBAL_ILLUMINATION_25 = range(5)
PROGRAM_CUSTOM_OPENCL = 5
KERNEL_MODE_LINEAR, KERNEL_MODE_TILE = 0, 1
RENDER_FLAG_STATS = 1
RENDER_FLAG_PIXEL_COUNTERS = 2
RENDER_FLAG_DEVICE_LIBM = 4      # ignored (ABI 2 name of RENDER_FLAG_STRICT_MATH)
RENDER_FLAG_PORTABLE_MATH = 8
RENDER_FLAG_STRICT_MATH = 16
RENDER_FLAG_NO_WALK_TIMING = 32
TRACE_CLOSEST, TRACE_ANY = 0, 1      # lt_hip_trace_desc::kind
TRACE_FLAG_COHERENT = 0x100          # runs of 64 consecutive rays are coherent: walked as packets
TRACE_FIRST_K, TRACE_COUNT = 0, 1    # lt_hip_multihit_desc::kind (lt_hip_trace_hits only)
TRACE_MAX_HITS = 8                   # LT_TRACE_MAX_HITS
TRACE_LIST_FLAG_FILL_ONLY = 0x200    # lt_hip_hits_list_desc::flags: offsets is input, only items is written
NEAREST_FIRST_K, NEAREST_COUNT = 0, 1   # lt_hip_nearest_k_desc::kind
NEAREST_MAX_K = 8                    # LT_NEAREST_MAX_K
OVERLAP_FIRST_K, OVERLAP_COUNT, OVERLAP_ANY = 0, 1, 2   # lt_hip_overlap_desc::kind
OVERLAP_MAX_K = 8                    # LT_OVERLAP_MAX_K
OVERLAP_LIST_FLAG_FILL_ONLY = 1      # lt_hip_overlap_list_desc::flags: offsets is input, only items is written
NEAREST_LIST_FLAG_FILL_ONLY = 1      # lt_hip_nearest_list_desc::flags: the same
SURFACE_LIGHT = 1                    # lt_hip_surface::flags: the primitive is in the light list

# every symbol include/lenstrace_hip.h declares
EXPORTS = ["lt_hip_abi_version", "lt_hip_create", "lt_hip_destroy", "lt_hip_last_error", "lt_hip_program_from_path",
           "lt_hip_resolve_program",
           "lt_hip_set_scene", "lt_hip_output_floats", "lt_hip_render", "lt_hip_render_scene", "lt_hip_render_device", "lt_hip_untile",
           "lt_hip_synchronize", "lt_hip_get_stats", "lt_hip_own_hierarchy", "lt_hip_own_wide", "lt_hip_read_scene_structure",
           "lt_hip_set_triangles", "lt_hip_set_triangles_device", "lt_hip_build_scene_host", "lt_hip_read_scene_buffer",
           "lt_hip_trace_rays", "lt_hip_trace_rays_device", "lt_hip_trace_hits", "lt_hip_trace_hits_device",
           "lt_hip_trace_hits_list", "lt_hip_trace_hits_list_device",
           "lt_hip_shade_rays", "lt_hip_shade_rays_device", "lt_hip_shade_paths", "lt_hip_shade_paths_device",
           "lt_hip_trace_surface", "lt_hip_trace_surface_device", "lt_hip_surface_at", "lt_hip_surface_at_device",
           "lt_hip_nearest_points", "lt_hip_nearest_points_device", "lt_hip_nearest_points_host",
           "lt_hip_nearest_k", "lt_hip_nearest_k_device", "lt_hip_nearest_k_host",
           "lt_hip_nearest_list", "lt_hip_nearest_list_device", "lt_hip_nearest_list_host",
           "lt_hip_overlap_boxes", "lt_hip_overlap_boxes_device", "lt_hip_overlap_boxes_host",
           "lt_hip_overlap_tris", "lt_hip_overlap_tris_device", "lt_hip_overlap_tris_host",
           "lt_hip_overlap_boxes_list", "lt_hip_overlap_boxes_list_device", "lt_hip_overlap_boxes_list_host",
           "lt_hip_overlap_tris_list", "lt_hip_overlap_tris_list_device", "lt_hip_overlap_tris_list_host",
           "lt_hip_entry_cut_counts", "lt_hip_entry_cut_test_host",
           "lt_hip_entry_cut_leaf_counts", "lt_hip_entry_cut_triangle_test_host",
           "lt_hip_entry_cut_chunk_counts", "lt_hip_entry_cut_chunks_test_host", "lt_hip_read_entry_cuts",
           "lt_hip_entry_cut_pruned_test_host", "lt_hip_clear_item_counts", "lt_hip_clear_items_test_host",
           "lt_hip_clear_square_counts", "lt_hip_random_fast_test_host"]
# (lt_hip_camera_hit_passes returns a uint64_t count, not a status: bound in load() beside these)


class RenderDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("program", ctypes.c_int32), ("kernel_mode", ctypes.c_int32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth", ctypes.c_uint32),
                ("camera", ctypes.c_uint8 * 28),
                ("frame_first", ctypes.c_uint32), ("frame_count", ctypes.c_uint32), ("accumulate", ctypes.c_uint32),
                ("accumulate_base", ctypes.c_uint32),
                ("tile_w", ctypes.c_uint32), ("tile_h", ctypes.c_uint32), ("tile_first", ctypes.c_uint32),
                ("tile_stride", ctypes.c_uint32),
                ("gi_max_depth", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_uint64), ("shadow_rays", ctypes.c_uint64), ("node_visits", ctypes.c_uint64),
                ("tri_tests", ctypes.c_uint64), ("pixels", ctypes.c_uint64), ("frames", ctypes.c_uint32),
                ("kernel_launches", ctypes.c_uint32), ("kernel_ms", ctypes.c_float), ("total_ms", ctypes.c_float),
                ("render_ms", ctypes.c_float), ("shadow_packets", ctypes.c_int32),
                ("scene_uploads", ctypes.c_uint32), ("scene_reused", ctypes.c_uint32),
                ("own_tree_height", ctypes.c_int32), ("own_tree_ms", ctypes.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TraceRay(ctypes.Structure):   # lt_hip_ray
    _fields_ = [("origin", ctypes.c_float * 3), ("tmax", ctypes.c_float), ("direction", ctypes.c_float * 3), ("ignore", ctypes.c_int32)]


class TraceHit(ctypes.Structure):   # lt_hip_hit
    _fields_ = [("t", ctypes.c_float), ("prim", ctypes.c_int32), ("u", ctypes.c_float), ("v", ctypes.c_float)]


class TraceDesc(ctypes.Structure):   # lt_hip_trace_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("program", ctypes.c_int32), ("kind", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class MultiHitDesc(ctypes.Structure):   # lt_hip_multihit_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("program", ctypes.c_int32), ("kind", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("max_hits", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ShadeRay(ctypes.Structure):   # lt_hip_shade_ray
    _fields_ = [("origin", ctypes.c_float * 3), ("film_x", ctypes.c_float), ("direction", ctypes.c_float * 3), ("film_y", ctypes.c_float)]


class ShadeResult(ctypes.Structure):   # lt_hip_shade
    _fields_ = [("rgb", ctypes.c_float * 3), ("prim", ctypes.c_int32)]


class ShadeDesc(ctypes.Structure):   # lt_hip_shade_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("program", ctypes.c_int32), ("kernel_mode", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("frame_first", ctypes.c_uint32), ("frame_count", ctypes.c_uint32)]


class PathsDesc(ctypes.Structure):   # lt_hip_paths_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("program", ctypes.c_int32), ("kernel_mode", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("frame_first", ctypes.c_uint32), ("frame_count", ctypes.c_uint32), ("gi_max_depth", ctypes.c_int32),
                ("reserved", ctypes.c_uint32)]


class Surface(ctypes.Structure):   # lt_hip_surface
    _fields_ = [("t", ctypes.c_float), ("prim", ctypes.c_int32), ("u", ctypes.c_float), ("v", ctypes.c_float),
                ("position", ctypes.c_float * 3), ("material", ctypes.c_int32), ("normal", ctypes.c_float * 3), ("flags", ctypes.c_uint32)]


class SurfaceDesc(ctypes.Structure):   # lt_hip_surface_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class Point(ctypes.Structure):   # lt_hip_point
    _fields_ = [("p", ctypes.c_float * 3), ("max_d2", ctypes.c_float)]


class NearestDesc(ctypes.Structure):   # lt_hip_nearest_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class NearestKDesc(ctypes.Structure):   # lt_hip_nearest_k_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("kind", ctypes.c_int32), ("max_k", ctypes.c_uint32)]


class Box(ctypes.Structure):   # lt_hip_box
    _fields_ = [("lo", ctypes.c_float * 3), ("pad0", ctypes.c_uint32), ("hi", ctypes.c_float * 3), ("pad1", ctypes.c_uint32)]


class Tri(ctypes.Structure):   # lt_hip_tri
    _fields_ = [("a", ctypes.c_float * 3), ("pad0", ctypes.c_uint32), ("b", ctypes.c_float * 3), ("pad1", ctypes.c_uint32),
                ("c", ctypes.c_float * 3), ("pad2", ctypes.c_uint32)]


class OverlapDesc(ctypes.Structure):   # lt_hip_overlap_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("kind", ctypes.c_int32), ("max_k", ctypes.c_uint32)]


class OverlapListDesc(ctypes.Structure):   # lt_hip_overlap_list_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class NearestListDesc(ctypes.Structure):   # lt_hip_nearest_list_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class HitsListDesc(ctypes.Structure):   # lt_hip_hits_list_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("program", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class TrianglesDesc(ctypes.Structure):   # lt_hip_triangles_desc
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n", ctypes.c_uint64),
                ("positions", ctypes.c_void_p), ("normals", ctypes.c_void_p), ("material_indices", ctypes.c_void_p),
                ("materials", ctypes.c_void_p), ("material_bytes", ctypes.c_uint64)]


def _np_dtypes():
    import numpy as np
    ray = np.dtype([("origin", "<f4", (3,)), ("tmax", "<f4"), ("direction", "<f4", (3,)), ("ignore", "<i4")])
    hit = np.dtype([("t", "<f4"), ("prim", "<i4"), ("u", "<f4"), ("v", "<f4")])
    return ray, hit


RAY_DTYPE, HIT_DTYPE = _np_dtypes()   # numpy views of lt_hip_ray (32 bytes) and lt_hip_hit (16 bytes)


def _np_shade_dtypes():
    import numpy as np
    ray = np.dtype([("origin", "<f4", (3,)), ("film_x", "<f4"), ("direction", "<f4", (3,)), ("film_y", "<f4")])
    out = np.dtype([("rgb", "<f4", (3,)), ("prim", "<i4")])
    return ray, out


SHADE_RAY_DTYPE, SHADE_DTYPE = _np_shade_dtypes()   # numpy views of lt_hip_shade_ray (32 bytes) and lt_hip_shade (16 bytes)


def _np_surface_dtype():
    import numpy as np
    return np.dtype([("t", "<f4"), ("prim", "<i4"), ("u", "<f4"), ("v", "<f4"), ("position", "<f4", (3,)), ("material", "<i4"),
                     ("normal", "<f4", (3,)), ("flags", "<u4")])


SURFACE_DTYPE = _np_surface_dtype()   # numpy view of lt_hip_surface (48 bytes)


def _np_point_dtype():
    import numpy as np
    return np.dtype([("p", "<f4", (3,)), ("max_d2", "<f4")])


POINT_DTYPE = _np_point_dtype()   # numpy view of lt_hip_point (16 bytes)


def _np_box_dtype():
    import numpy as np
    return np.dtype([("lo", "<f4", (3,)), ("pad0", "<u4"), ("hi", "<f4", (3,)), ("pad1", "<u4")])


BOX_DTYPE = _np_box_dtype()   # numpy view of lt_hip_box (32 bytes)


def _np_tri_dtype():
    import numpy as np
    return np.dtype([("a", "<f4", (3,)), ("pad0", "<u4"), ("b", "<f4", (3,)), ("pad1", "<u4"), ("c", "<f4", (3,)), ("pad2", "<u4")])


TRI_DTYPE = _np_tri_dtype()   # numpy view of lt_hip_tri (48 bytes)


class LensTraceError(RuntimeError):
    def __init__(self, code, text):
        self.code = code
        name = STATUS_NAMES[code] if 0 <= code < len(STATUS_NAMES) else str(code)
        super().__init__("%s: %s" % (name, text))


_lib = None


def load():
    """Loads liblenstrace-hip.so; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as the
    # system one).  Importing torch first makes this library bind to the copy torch uses, so device pointers,
    # streams and RCCL buffers are shared; loaded the other way round, the process ends up with two runtimes
    # and torch reports "No HIP GPUs are available".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: the HIP extension is not built (run __graft_entry__.build()); "
                          "there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.lt_hip_abi_version.restype = i32
    L.lt_hip_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.lt_hip_destroy.argtypes = [vp]
    L.lt_hip_last_error.argtypes = [vp]
    L.lt_hip_last_error.restype = ctypes.c_char_p
    L.lt_hip_program_from_path.argtypes = [ctypes.c_char_p, ctypes.POINTER(i32)]
    L.lt_hip_resolve_program.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32)]
    L.lt_hip_set_scene.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64]
    L.lt_hip_output_floats.argtypes = [ctypes.POINTER(RenderDesc), ctypes.POINTER(u64)]
    L.lt_hip_render.argtypes = [vp, ctypes.POINTER(RenderDesc), vp, u64]
    if hasattr(L, "lt_hip_render_scene"):
        L.lt_hip_render_scene.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, ctypes.POINTER(RenderDesc), vp, u64]
    L.lt_hip_render_device.argtypes = [vp, ctypes.POINTER(RenderDesc), vp, u64, vp]
    L.lt_hip_untile.argtypes = [vp, vp, u64, u32, u32, u32, u32, u32, u32, vp, vp]
    L.lt_hip_synchronize.argtypes = [vp, vp]
    L.lt_hip_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    if hasattr(L, "lt_hip_trace_rays"):
        L.lt_hip_trace_rays.argtypes = [vp, ctypes.POINTER(TraceDesc), vp, u64, vp, u64]
        L.lt_hip_trace_rays_device.argtypes = [vp, ctypes.POINTER(TraceDesc), vp, u64, vp, u64, vp]
    if hasattr(L, "lt_hip_trace_hits"):
        L.lt_hip_trace_hits.argtypes = [vp, ctypes.POINTER(MultiHitDesc), vp, u64, vp, u64]
        L.lt_hip_trace_hits_device.argtypes = [vp, ctypes.POINTER(MultiHitDesc), vp, u64, vp, u64, vp]
    if hasattr(L, "lt_hip_shade_rays"):
        L.lt_hip_shade_rays.argtypes = [vp, ctypes.POINTER(ShadeDesc), vp, u64, vp, u64]
        L.lt_hip_shade_rays_device.argtypes = [vp, ctypes.POINTER(ShadeDesc), vp, u64, vp, u64, vp]
    if hasattr(L, "lt_hip_shade_paths"):
        L.lt_hip_shade_paths.argtypes = [vp, ctypes.POINTER(PathsDesc), vp, u64, vp, u64]
        L.lt_hip_shade_paths_device.argtypes = [vp, ctypes.POINTER(PathsDesc), vp, u64, vp, u64, vp]
    if hasattr(L, "lt_hip_trace_surface"):
        L.lt_hip_trace_surface.argtypes = [vp, ctypes.POINTER(TraceDesc), vp, u64, vp, u64]
        L.lt_hip_trace_surface_device.argtypes = [vp, ctypes.POINTER(TraceDesc), vp, u64, vp, u64, vp]
        L.lt_hip_surface_at.argtypes = [vp, ctypes.POINTER(SurfaceDesc), vp, u64, vp, u64]
        L.lt_hip_surface_at_device.argtypes = [vp, ctypes.POINTER(SurfaceDesc), vp, u64, vp, u64, vp]
    if hasattr(L, "lt_hip_nearest_points"):
        L.lt_hip_nearest_points.argtypes = [vp, ctypes.POINTER(NearestDesc), vp, u64, vp, u64]
        L.lt_hip_nearest_points_device.argtypes = [vp, ctypes.POINTER(NearestDesc), vp, u64, vp, u64, vp]
        L.lt_hip_nearest_points_host.argtypes = [vp, u64, vp, u64, vp, u64, vp, u64]
    if hasattr(L, "lt_hip_nearest_k"):
        L.lt_hip_nearest_k.argtypes = [vp, ctypes.POINTER(NearestKDesc), vp, u64, vp, u64]
        L.lt_hip_nearest_k_device.argtypes = [vp, ctypes.POINTER(NearestKDesc), vp, u64, vp, u64, vp]
        L.lt_hip_nearest_k_host.argtypes = [vp, u64, vp, u64, ctypes.POINTER(NearestKDesc), vp, u64, vp, u64]
    if hasattr(L, "lt_hip_overlap_boxes"):
        L.lt_hip_overlap_boxes.argtypes = [vp, ctypes.POINTER(OverlapDesc), vp, u64, vp, u64]
        L.lt_hip_overlap_boxes_device.argtypes = [vp, ctypes.POINTER(OverlapDesc), vp, u64, vp, u64, vp]
        L.lt_hip_overlap_boxes_host.argtypes = [vp, u64, vp, u64, ctypes.POINTER(OverlapDesc), vp, u64, vp, u64]
    if hasattr(L, "lt_hip_overlap_tris"):
        L.lt_hip_overlap_tris.argtypes = [vp, ctypes.POINTER(OverlapDesc), vp, u64, vp, u64]
        L.lt_hip_overlap_tris_device.argtypes = [vp, ctypes.POINTER(OverlapDesc), vp, u64, vp, u64, vp]
        L.lt_hip_overlap_tris_host.argtypes = [vp, u64, vp, u64, ctypes.POINTER(OverlapDesc), vp, u64, vp, u64]
    if hasattr(L, "lt_hip_overlap_boxes_list"):
        for shape in ("boxes", "tris"):
            lists = "lt_hip_overlap_%s_list" % shape
            getattr(L, lists).argtypes = [vp, ctypes.POINTER(OverlapListDesc), vp, u64, vp, u64, vp, u64]
            getattr(L, lists + "_device").argtypes = [vp, ctypes.POINTER(OverlapListDesc), vp, u64, vp, u64, vp, u64, vp]
            getattr(L, lists + "_host").argtypes = [vp, u64, vp, u64, ctypes.POINTER(OverlapListDesc), vp, u64, vp, u64, vp, u64]
    if hasattr(L, "lt_hip_trace_hits_list"):
        L.lt_hip_trace_hits_list.argtypes = [vp, ctypes.POINTER(HitsListDesc), vp, u64, vp, u64, vp, u64]
        L.lt_hip_trace_hits_list_device.argtypes = [vp, ctypes.POINTER(HitsListDesc), vp, u64, vp, u64, vp, u64, vp]
    if hasattr(L, "lt_hip_nearest_list"):
        L.lt_hip_nearest_list.argtypes = [vp, ctypes.POINTER(NearestListDesc), vp, u64, vp, u64, vp, u64]
        L.lt_hip_nearest_list_device.argtypes = [vp, ctypes.POINTER(NearestListDesc), vp, u64, vp, u64, vp, u64, vp]
        L.lt_hip_nearest_list_host.argtypes = [vp, u64, vp, u64, ctypes.POINTER(NearestListDesc), vp, u64, vp, u64, vp, u64]
    if hasattr(L, "lt_hip_set_triangles"):
        L.lt_hip_set_triangles.argtypes = [vp, ctypes.POINTER(TrianglesDesc)]
        L.lt_hip_set_triangles_device.argtypes = [vp, ctypes.POINTER(TrianglesDesc), vp]
        L.lt_hip_build_scene_host.argtypes = [ctypes.POINTER(TrianglesDesc), vp, u64, vp, u64, vp]
        L.lt_hip_read_scene_buffer.argtypes = [vp, i32, vp, u64, ctypes.POINTER(u64)]
    if hasattr(L, "lt_hip_camera_hit_passes"):
        L.lt_hip_camera_hit_passes.argtypes = [vp]
        L.lt_hip_camera_hit_passes.restype = u64
    if hasattr(L, "lt_hip_entry_cut_counts"):
        L.lt_hip_entry_cut_counts.argtypes = [vp, ctypes.POINTER(u64)]
        L.lt_hip_entry_cut_counts.restype = i32
        L.lt_hip_entry_cut_test_host.argtypes = [vp, vp, vp, u64, vp]
        L.lt_hip_entry_cut_test_host.restype = i32
    if hasattr(L, "lt_hip_entry_cut_leaf_counts"):
        L.lt_hip_entry_cut_leaf_counts.argtypes = [vp, ctypes.POINTER(u64)]
        L.lt_hip_entry_cut_leaf_counts.restype = i32
        L.lt_hip_entry_cut_triangle_test_host.argtypes = [vp, vp, vp, u64, vp]
        L.lt_hip_entry_cut_triangle_test_host.restype = i32
    if hasattr(L, "lt_hip_entry_cut_chunk_counts"):
        L.lt_hip_entry_cut_chunk_counts.argtypes = [vp, ctypes.POINTER(u64)]
        L.lt_hip_entry_cut_chunk_counts.restype = i32
        L.lt_hip_entry_cut_chunks_test_host.argtypes = [vp, vp, vp, vp, u64, vp]
        L.lt_hip_entry_cut_chunks_test_host.restype = i32
    if hasattr(L, "lt_hip_read_entry_cuts"):
        L.lt_hip_read_entry_cuts.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
        L.lt_hip_read_entry_cuts.restype = i32
    if hasattr(L, "lt_hip_entry_cut_pruned_test_host"):
        L.lt_hip_entry_cut_pruned_test_host.argtypes = [vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
        L.lt_hip_entry_cut_pruned_test_host.restype = i32
    if hasattr(L, "lt_hip_clear_item_counts"):
        L.lt_hip_clear_item_counts.argtypes = [vp, ctypes.POINTER(u64)]
        L.lt_hip_clear_item_counts.restype = i32
        L.lt_hip_clear_items_test_host.argtypes = [vp, vp] + [ctypes.c_uint32] * 5 + [vp, vp]
        L.lt_hip_clear_items_test_host.restype = i32
    if hasattr(L, "lt_hip_clear_square_counts"):
        L.lt_hip_clear_square_counts.argtypes = [vp, ctypes.POINTER(u64)]
        L.lt_hip_clear_square_counts.restype = i32
    if hasattr(L, "lt_hip_random_fast_test_host"):
        L.lt_hip_random_fast_test_host.argtypes = [i32, vp, vp, u64, vp, vp, vp, vp, vp]
        L.lt_hip_random_fast_test_host.restype = i32
    for name in EXPORTS:
        if not hasattr(L, name) and os.environ.get("LT_HIP_LIBRARY"):
            continue      # (an older build of the library loaded for an A/B measurement, tests/tools/ab_libs.sh)
        if name not in ("lt_hip_last_error",):
            getattr(L, name).restype = i32
    if L.lt_hip_abi_version() != 4:
        raise ImportError("liblenstrace-hip.so ABI version mismatch")
    _lib = L
    return L


def program_from_path(path):
    out = ctypes.c_int(0)
    rc = load().lt_hip_program_from_path(path.encode(), ctypes.byref(out))
    if rc:
        raise LensTraceError(rc, "no built-in program for kernel file %r" % path)
    return out.value


def own_hierarchy(nodes, n_prims=0, height_slack=2, want_ranks=False):
    """lt_hip_own_hierarchy (host only): (height, nodes of the backend's own hierarchy as a NODE_DTYPE array, rank8 or None);
    height -1 and no arrays when the scene gets none."""
    import numpy as np
    from . import scene as sc
    nodes = np.ascontiguousarray(nodes)
    leaves = int((nodes["primitiveCount"] != 0).sum())
    out = np.zeros(max(1, 2 * leaves - 1), dtype=sc.NODE_DTYPE)
    ranks = np.zeros((max(1, n_prims), 8), dtype=np.uint32) if want_ranks else None
    h = load().lt_hip_own_hierarchy(nodes.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(nodes.nbytes), ctypes.c_int(height_slack),
                                    out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.nbytes),
                                    ranks.ctypes.data_as(ctypes.c_void_p) if want_ranks else None, ctypes.c_uint32(n_prims))
    if h < 0:
        return -1, None, None
    return h, out, ranks


OWN16_DTYPE = [("q", "<u2", (6,)), ("link", "<u4")]   # a child slot: lo.x lo.y lo.z hi.x hi.y hi.z on the grid; the child's group or 0x80000000 | leaf record


def own_wide(own_nodes, n_prims):
    """lt_hip_own_wide (host only): (height of the group tree, origin[3], step[3], slots as an OWN16_DTYPE array of shape (groups, 4))."""
    import numpy as np
    own_nodes = np.ascontiguousarray(own_nodes)
    frame = np.zeros(6, dtype=np.float32)
    out = np.zeros((max(1, len(own_nodes) // 2), 4), dtype=OWN16_DTYPE)
    assert out.dtype.itemsize == 16
    groups = ctypes.c_uint32(0)
    h = load().lt_hip_own_wide(own_nodes.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(own_nodes.nbytes), ctypes.c_uint32(n_prims),
                               frame.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(out.nbytes),
                               ctypes.byref(groups))
    if h < 0:
        raise LensTraceError(LT_ERR_BAD_SCENE, "lt_hip_own_wide failed")
    return h, frame[:3].copy(), frame[3:].copy(), out[:groups.value].copy()
