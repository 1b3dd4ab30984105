"""Python mirror of the renderer plugin surface for this path
(/root/reference/include/lens_trace/renderer.h:5-9, structures.h:51-79, src/opencl/renderer_opencl.cpp:56-153):
RendererHIP.render(RenderPropertiesHIP) fills a caller-owned float buffer, synchronously.  Everything goes
through the C ABI of liblenstrace-hip.so; there is no other compute path."""
import ctypes
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _capi as C
from .scene import Scene

KERNEL_MODE_LINEAR, KERNEL_MODE_TILE = C.KERNEL_MODE_LINEAR, C.KERNEL_MODE_TILE
THREAD_ORGANIZATION_MODE_MAX_FIT, THREAD_ORGANIZATION_MODE_CUSTOM = 0, 1


@dataclass
class ThreadOrganizationHIP:
    """Accepted for API parity with ThreadOrganizationCUDA (structures.h:45-49); pixels never depend on the
    launch decomposition (the reference's CustomBlockSize test), and this backend picks its own."""
    blockSize: tuple = (0, 0)


@dataclass
class RenderPropertiesHIP:
    kernelFilePath: str
    imageDimensions: tuple                       # (W, H, depth)
    pOutputBuffer: np.ndarray                    # float32, >= W*H*depth elements, caller-owned
    pAccelerationStructureExplicit: Scene        # provides node / primitive / light buffers
    pModel: Optional[Scene] = None               # provides the material buffer (defaults to the same Scene)
    pCamera: bytes = b""                         # 28-byte camera buffer
    kernelMode: int = KERNEL_MODE_LINEAR
    threadOrganizationMode: int = THREAD_ORGANIZATION_MODE_MAX_FIT
    threadOrganization: ThreadOrganizationHIP = field(default_factory=ThreadOrganizationHIP)
    # extensions (the reference's unused pNext slot): progressive rendering on the device
    frameFirst: int = 0
    frameCount: int = 0
    accumulate: bool = False
    accumulateBase: int = 0
    giMaxDepth: int = 0
    collectStats: bool = False
    pixelCounters: bool = False                  # diagnostic: per-pixel work counters instead of colour (depth >= 4)
    # Floating-point flavour.  Default: the reference's kernel files as RendererOpenCL builds them on this
    # GPU (clBuildProgram with NULL options) -- bit-identical to them.  strictMath: the same kernels built with
    # -ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt.  portableMath: strict, with the device library's approximate
    # leaf functions (rsqrt, sqrt, sinf, cosf, clamp) in correctly rounded forms -- what the CPU oracle computes.
    portableMath: bool = False
    strictMath: bool = False
    # 0: every render() hands the scene buffers to lt_hip_set_scene, which hashes them in full and uploads only when the
    # content changed (the reference uploads on every call).  != 0: the caller versions its scene; the buffers are looked at
    # again only when the objects or this number change.
    sceneVersion: int = 0


def make_desc(program, W, H, depth, camera28, kernel_mode=KERNEL_MODE_LINEAR, frame_first=0, frame_count=0,
              accumulate=False, accumulate_base=0, tile=None, gi_max_depth=0, stats=False, pixel_counters=False, portable_math=False, strict_math=False):
    d = C.RenderDesc()
    d.struct_size = ctypes.sizeof(C.RenderDesc)
    d.program, d.kernel_mode = program, kernel_mode
    d.width, d.height, d.depth = W, H, depth
    cam = bytes(camera28)
    if len(cam) != 28:
        raise ValueError("camera buffer must be 28 bytes")
    ctypes.memmove(d.camera, cam, 28)
    d.frame_first, d.frame_count = frame_first, frame_count
    d.accumulate, d.accumulate_base = int(bool(accumulate)), accumulate_base
    if tile is not None:
        d.tile_w, d.tile_h, d.tile_first, d.tile_stride = tile
    d.gi_max_depth = gi_max_depth
    d.flags = ((C.RENDER_FLAG_STATS if stats else 0) | (C.RENDER_FLAG_PIXEL_COUNTERS if pixel_counters else 0) |
               (C.RENDER_FLAG_PORTABLE_MATH if portable_math else 0) | (C.RENDER_FLAG_STRICT_MATH if strict_math else 0))
    return d


FLT_MAX = float(np.finfo(np.float32).max)   # the reference's payload start (acc.cl: RayPayload.t = FLT_MAX)
RAY_DTYPE, HIT_DTYPE = C.RAY_DTYPE, C.HIT_DTYPE
SURFACE_DTYPE = C.SURFACE_DTYPE


def make_rays(origins, directions, tmax=FLT_MAX, ignore=-1):
    """Packs rays for RendererHIP.trace_rays: (n, 3) origins and directions, tmax and ignore (the primitive a ray starts on,
    -1 = none) as scalars or (n,) arrays, into an (n, 8) float32 array of lt_hip_ray records (ignore's int32 bits in column 7)."""
    o = np.asarray(origins, dtype=np.float32)
    d = np.asarray(directions, dtype=np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("origins and directions must both have shape (n, 3)")
    n = o.shape[0]
    t = np.asarray(tmax, dtype=np.float32)
    ig = np.asarray(ignore)
    if t.shape not in ((), (n,)) or ig.shape not in ((), (n,)):
        raise ValueError("tmax and ignore must be scalars or have shape (n,)")
    if ig.size and (not np.issubdtype(ig.dtype, np.integer) or ig.min() < -2 ** 31 or ig.max() >= 2 ** 31):
        raise ValueError("ignore must hold int32 primitive indices")
    out = np.empty((n, 8), dtype=np.float32)
    out[:, 0:3] = o
    out[:, 3] = t
    out[:, 4:7] = d
    out[:, 7] = np.broadcast_to(ig.astype(np.int32), (n,)).view(np.float32)
    return out


SHADE_RAY_DTYPE, SHADE_DTYPE = C.SHADE_RAY_DTYPE, C.SHADE_DTYPE


def make_shade_rays(origins, directions, film_x, film_y):
    """Packs rays for RendererHIP.shade_rays: (n, 3) origins and directions, film_x and film_y (the film position that keys the
    program's random(): scalars or (n,) arrays), into an (n, 8) float32 array of lt_hip_shade_ray records -- origin, film_x,
    direction, film_y."""
    o = np.asarray(origins, dtype=np.float32)
    d = np.asarray(directions, dtype=np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("origins and directions must both have shape (n, 3)")
    n = o.shape[0]
    fx = np.asarray(film_x, dtype=np.float32)
    fy = np.asarray(film_y, dtype=np.float32)
    if fx.shape not in ((), (n,)) or fy.shape not in ((), (n,)):
        raise ValueError("film_x and film_y must be scalars or have shape (n,)")
    out = np.empty((n, 8), dtype=np.float32)
    out[:, 0:3] = o
    out[:, 3] = fx
    out[:, 4:7] = d
    out[:, 7] = fy
    return out


def reference_camera_rays(camera28, W, H):
    """The reference camera's rays (accumulator.cl:304-312: a pinhole at cameraPosition + film aiming at the aperture (0, 0, 5),
    turned by yaw alone) in portable arithmetic, pixel-major (pixel y * W + x): (origins (n, 3), directions (n, 3), film_x (n,),
    film_y (n,)), all float32 -- the starting point for a caller's own camera.  In the portable flavour these are the render
    kernel's rays bit for bit; in the default and strict flavours only for yaw 0 and power-of-two W, H (they use a fused
    multiply-add in the rotation and the device's divide)."""
    cam = np.frombuffer(bytes(camera28), dtype=np.float32, count=7)
    f32 = np.float32
    x = np.tile(np.arange(W, dtype=np.float32), H)
    y = np.repeat(np.arange(H, dtype=np.float32), W)
    fx = (x / f32(W) - f32(0.5)).astype(np.float32)
    fy = (y / f32(H) - f32(0.5)).astype(np.float32)
    o = np.empty((W * H, 3), dtype=np.float32)
    o[:, 0] = cam[0] + fx
    o[:, 1] = cam[1] + fy
    o[:, 2] = cam[2] + f32(0.0)
    dx = f32(0.0) - fx
    dy = f32(0.0) - fy
    dz = np.full(W * H, f32(5.0) - f32(0.0), dtype=np.float32)
    cy, sy = f32(np.cos(np.float64(cam[3]))), f32(np.sin(np.float64(cam[3])))
    d = np.empty((W * H, 3), dtype=np.float32)
    d[:, 0] = (cy * dx).astype(np.float32) + (sy * dz).astype(np.float32)
    d[:, 1] = dy
    d[:, 2] = (-sy * dx).astype(np.float32) + (cy * dz).astype(np.float32)
    return o, d, fx, fy


def ray_records(rays, record_dtype, names):
    """A numpy batch of 32-byte ray records as a contiguous (n, 8) float32 array: an (n, 8) float32 array as it is, a 1-D array of
    `record_dtype` viewed as one.  names: (the function that packs such records, the dtype's name), for the error's text."""
    if rays.dtype == record_dtype and rays.ndim == 1:
        rays = rays.view(np.float32).reshape(-1, 8)
    if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError("rays must be an (n, 8) float32 array (%s) or a %s array" % names)
    return np.ascontiguousarray(rays)


POINT_DTYPE = C.POINT_DTYPE


def make_points(points, max_d2=np.inf):
    """Packs points for RendererHIP.nearest_points: (n, 3) positions and max_d2 (a candidate counts only if its squared distance
    is below it: a scalar or an (n,) array) into an (n, 4) float32 array of lt_hip_point records."""
    p = np.asarray(points, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must have shape (n, 3)")
    m = np.asarray(max_d2, dtype=np.float32)
    if m.shape not in ((), (p.shape[0],)):
        raise ValueError("max_d2 must be a scalar or have shape (n,)")
    out = np.empty((p.shape[0], 4), dtype=np.float32)
    out[:, 0:3] = p
    out[:, 3] = m
    return out


def point_records(points, max_d2=np.inf):
    """A numpy batch of points as a contiguous (n, 4) float32 array of lt_hip_point records: a 1-D POINT_DTYPE array or an (n, 4)
    float32 array as it is (max_d2 must then be left alone), an (n, 3) array packed with max_d2 (make_points)."""
    if points.dtype == POINT_DTYPE and points.ndim == 1:
        points = points.view(np.float32).reshape(-1, 4)
    elif points.ndim == 2 and points.shape[1] == 3:
        return make_points(points, max_d2)
    if points.dtype != np.float32 or points.ndim != 2 or points.shape[1] != 4:
        raise ValueError("points must be an (n, 3) array, an (n, 4) float32 array (make_points) or a POINT_DTYPE array")
    if not (np.ndim(max_d2) == 0 and np.isposinf(max_d2)):
        raise ValueError("ready lt_hip_point records carry their own max_d2")
    return np.ascontiguousarray(points)


def nearest_points_host(scene: Scene, points, max_d2=np.inf):
    """lt_hip_nearest_points_host: RendererHIP.nearest_points' answers computed on the host from the scene's own buffers, leaf by
    leaf -- no context, no GPU.  points as nearest_points takes numpy batches; returns a HIT_DTYPE array."""
    pts = point_records(np.asarray(points), max_d2)
    nodes, prims = np.ascontiguousarray(scene.nodes), np.ascontiguousarray(scene.prims)
    out = np.zeros(pts.shape[0], dtype=HIT_DTYPE)
    vp = ctypes.c_void_p
    rc = C.load().lt_hip_nearest_points_host(nodes.ctypes.data_as(vp), nodes.nbytes, prims.ctypes.data_as(vp), prims.nbytes,
                                             pts.ctypes.data_as(vp), pts.shape[0], out.ctypes.data_as(vp), out.nbytes)
    if rc:
        raise C.LensTraceError(rc, "lt_hip_nearest_points_host failed")
    return out


def _nearest_k_desc(k, count):
    if not count and not 1 <= k <= C.NEAREST_MAX_K:
        raise ValueError("k must be in 1..%d" % C.NEAREST_MAX_K)
    return C.NearestKDesc(ctypes.sizeof(C.NearestKDesc), 0, C.NEAREST_COUNT if count else C.NEAREST_FIRST_K, 0 if count else int(k))


def nearest_k_host(scene: Scene, points, k=4, count=False, max_d2=np.inf):
    """lt_hip_nearest_k_host: RendererHIP.nearest_k's answers computed on the host from the scene's own buffers, leaf by leaf -- no
    context, no GPU.  points as nearest_k takes numpy batches; returns an (n, k) HIT_DTYPE array or, count, (n,) uint32."""
    d = _nearest_k_desc(k, count)
    pts = point_records(np.asarray(points), max_d2)
    nodes, prims = np.ascontiguousarray(scene.nodes), np.ascontiguousarray(scene.prims)
    out = np.zeros(pts.shape[0], dtype=np.uint32) if count else np.zeros((pts.shape[0], int(k)), dtype=HIT_DTYPE)
    vp = ctypes.c_void_p
    rc = C.load().lt_hip_nearest_k_host(nodes.ctypes.data_as(vp), nodes.nbytes, prims.ctypes.data_as(vp), prims.nbytes, ctypes.byref(d),
                                        pts.ctypes.data_as(vp), pts.shape[0], out.ctypes.data_as(vp), out.nbytes)
    if rc:
        raise C.LensTraceError(rc, "lt_hip_nearest_k_host failed")
    return out


BOX_DTYPE = C.BOX_DTYPE


def make_boxes(lo, hi):
    """Packs boxes for RendererHIP.overlap_boxes: (n, 3) lower and upper corners into an (n, 8) float32 array of lt_hip_box
    records (lo, pad, hi, pad; the pads are zero and ignored)."""
    lo = np.asarray(lo, dtype=np.float32)
    hi = np.asarray(hi, dtype=np.float32)
    if lo.ndim != 2 or lo.shape[1] != 3 or hi.shape != lo.shape:
        raise ValueError("lo and hi must both have shape (n, 3)")
    out = np.zeros((lo.shape[0], 8), dtype=np.float32)
    out[:, 0:3] = lo
    out[:, 4:7] = hi
    return out


def box_records(boxes):
    """A numpy batch of boxes as a contiguous (n, 8) float32 array of lt_hip_box records: a 1-D BOX_DTYPE array or an (n, 8)
    float32 array (make_boxes)."""
    if boxes.dtype == BOX_DTYPE and boxes.ndim == 1:
        boxes = np.ascontiguousarray(boxes).view(np.float32).reshape(-1, 8)
    if boxes.dtype != np.float32 or boxes.ndim != 2 or boxes.shape[1] != 8:
        raise ValueError("boxes must be an (n, 8) float32 array (make_boxes) or a BOX_DTYPE array")
    return np.ascontiguousarray(boxes)


def _overlap_desc(k, count, any):
    if count and any:
        raise ValueError("count and any exclude each other")
    if (count or any) and k is not None:
        raise ValueError("k goes with neither count nor any")
    if not (count or any):
        k = 4 if k is None else k
        if not 1 <= k <= C.OVERLAP_MAX_K:
            raise ValueError("k must be in 1..%d" % C.OVERLAP_MAX_K)
    kind = C.OVERLAP_COUNT if count else C.OVERLAP_ANY if any else C.OVERLAP_FIRST_K
    return C.OverlapDesc(ctypes.sizeof(C.OverlapDesc), 0, kind, 0 if (count or any) else int(k))


def overlap_boxes_host(scene: Scene, boxes, k=None, count=False, any=False):
    """lt_hip_overlap_boxes_host: RendererHIP.overlap_boxes' answers computed on the host from the scene's own buffers, leaf by
    leaf -- no context, no GPU.  boxes as overlap_boxes takes numpy batches; returns an (n, k) int32 array or, count / any, (n,)
    uint32."""
    d = _overlap_desc(k, count, any)
    bx = box_records(np.asarray(boxes))
    nodes, prims = np.ascontiguousarray(scene.nodes), np.ascontiguousarray(scene.prims)
    out = np.zeros((bx.shape[0], d.max_k), dtype=np.int32) if d.max_k else np.zeros(bx.shape[0], dtype=np.uint32)
    vp = ctypes.c_void_p
    rc = C.load().lt_hip_overlap_boxes_host(nodes.ctypes.data_as(vp), nodes.nbytes, prims.ctypes.data_as(vp), prims.nbytes, ctypes.byref(d),
                                            bx.ctypes.data_as(vp), bx.shape[0], out.ctypes.data_as(vp), out.nbytes)
    if rc:
        raise C.LensTraceError(rc, "lt_hip_overlap_boxes_host failed")
    return out


TRI_DTYPE = C.TRI_DTYPE


def make_tris(a, b, c):
    """Packs query triangles for RendererHIP.overlap_tris: (n, 3) vertices a, b, c into an (n, 12) float32 array of lt_hip_tri
    records (a, pad, b, pad, c, pad; the pads are zero and ignored)."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3 or b.shape != a.shape or c.shape != a.shape:
        raise ValueError("a, b and c must all have shape (n, 3)")
    out = np.zeros((a.shape[0], 12), dtype=np.float32)
    out[:, 0:3] = a
    out[:, 4:7] = b
    out[:, 8:11] = c
    return out


def tri_records(tris):
    """A numpy batch of query triangles as a contiguous (n, 12) float32 array of lt_hip_tri records: a 1-D TRI_DTYPE array or an
    (n, 12) float32 array (make_tris)."""
    if tris.dtype == TRI_DTYPE and tris.ndim == 1:
        tris = np.ascontiguousarray(tris).view(np.float32).reshape(-1, 12)
    if tris.dtype != np.float32 or tris.ndim != 2 or tris.shape[1] != 12:
        raise ValueError("tris must be an (n, 12) float32 array (make_tris) or a TRI_DTYPE array")
    return np.ascontiguousarray(tris)


def overlap_tris_host(scene: Scene, tris, k=None, count=False, any=False):
    """lt_hip_overlap_tris_host: RendererHIP.overlap_tris' answers computed on the host from the scene's own buffers, leaf by
    leaf -- no context, no GPU.  tris as overlap_tris takes numpy batches; returns an (n, k) int32 array or, count / any, (n,)
    uint32."""
    d = _overlap_desc(k, count, any)
    tr = tri_records(np.asarray(tris))
    nodes, prims = np.ascontiguousarray(scene.nodes), np.ascontiguousarray(scene.prims)
    out = np.zeros((tr.shape[0], d.max_k), dtype=np.int32) if d.max_k else np.zeros(tr.shape[0], dtype=np.uint32)
    vp = ctypes.c_void_p
    rc = C.load().lt_hip_overlap_tris_host(nodes.ctypes.data_as(vp), nodes.nbytes, prims.ctypes.data_as(vp), prims.nbytes, ctypes.byref(d),
                                           tr.ctypes.data_as(vp), tr.shape[0], out.ctypes.data_as(vp), out.nbytes)
    if rc:
        raise C.LensTraceError(rc, "lt_hip_overlap_tris_host failed")
    return out


# The list families: (the descriptor, its FILL_ONLY flag, the numpy dtype of an item, the torch dtype and trailing shape of one).
_OVERLAP_LIST = (C.OverlapListDesc, C.OVERLAP_LIST_FLAG_FILL_ONLY, np.int32, ("int32", ()))
_NEAREST_LIST = (C.NearestListDesc, C.NEAREST_LIST_FLAG_FILL_ONLY, HIT_DTYPE, ("float32", (4,)))
# (the hit lists' descriptor also names a program and carries math flags: _list_call's `describe`)
_HITS_LIST = (C.HitsListDesc, C.TRACE_LIST_FLAG_FILL_ONLY, HIT_DTYPE, ("float32", (4,)))


def _list_host(name, scene, rec, family=_OVERLAP_LIST):
    """lt_hip_<name>_list_host over a contiguous numpy array of records: the sizing call, then the fill."""
    Desc, fill_only, item, _ = family
    nodes, prims = np.ascontiguousarray(scene.nodes), np.ascontiguousarray(scene.prims)
    vp = ctypes.c_void_p
    f = getattr(C.load(), "lt_hip_%s_list_host" % name)
    size = ctypes.sizeof(Desc)
    offsets = np.zeros(rec.shape[0] + 1, dtype=np.uint64)
    items = np.zeros(0, dtype=item)
    for flags in (0, fill_only):
        d = Desc(size, flags)
        rc = f(nodes.ctypes.data_as(vp), nodes.nbytes, prims.ctypes.data_as(vp), prims.nbytes, ctypes.byref(d), rec.ctypes.data_as(vp), rec.shape[0],
               offsets.ctypes.data_as(vp), offsets.nbytes, items.ctypes.data_as(vp) if flags else None, items.nbytes)
        if rc:
            raise C.LensTraceError(rc, "lt_hip_%s_list_host failed" % name)
        if not flags:
            items = np.zeros(int(offsets[-1]), dtype=item)
    return offsets, items


def nearest_list_host(scene: Scene, points, max_d2=np.inf):
    """lt_hip_nearest_list_host: RendererHIP.nearest_list's (offsets, items) computed on the host from the scene's own buffers, leaf
    by leaf -- no context, no GPU.  points as nearest_k takes numpy batches."""
    return _list_host("nearest", scene, point_records(np.asarray(points), max_d2), _NEAREST_LIST)


def overlap_boxes_list_host(scene: Scene, boxes):
    """lt_hip_overlap_boxes_list_host: RendererHIP.overlap_boxes_list's (offsets, items) computed on the host from the scene's own
    buffers, leaf by leaf -- no context, no GPU."""
    return _list_host("overlap_boxes", scene, box_records(np.asarray(boxes)))


def overlap_tris_list_host(scene: Scene, tris):
    """lt_hip_overlap_tris_list_host: RendererHIP.overlap_tris_list's (offsets, items) computed on the host, as
    overlap_boxes_list_host."""
    return _list_host("overlap_tris", scene, tri_records(np.asarray(tris)))


_QUERY_RAYS = (RAY_DTYPE, ("make_rays", "RAY_DTYPE"))
_SHADE_RAYS = (SHADE_RAY_DTYPE, ("make_shade_rays", "SHADE_RAY_DTYPE"))


def _program_id(program):
    return program if isinstance(program, int) else C.program_from_path(str(program))


def _ray_flags(coherent, portable_math, strict_math):
    return ((C.TRACE_FLAG_COHERENT if coherent else 0) | (C.RENDER_FLAG_PORTABLE_MATH if portable_math else 0) |
            (C.RENDER_FLAG_STRICT_MATH if strict_math else 0))


class RendererHIP:
    """One context per GPU.  `device` is the HIP ordinal."""

    def __init__(self, device=0):
        self._L = C.load()
        self.device = device
        self._ctx = ctypes.c_void_p()
        rc = self._L.lt_hip_create(device, ctypes.byref(self._ctx))
        if rc:
            raise C.LensTraceError(rc, self._L.lt_hip_last_error(None).decode())
        self._scene_key = None
        self._scene_refs = None
        self._scene_version = 0

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.lt_hip_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise C.LensTraceError(rc, self._L.lt_hip_last_error(self._ctx).decode())

    # -- scene -------------------------------------------------------------------------------------
    def set_scene(self, scene: Scene, materials: Optional[Scene] = None):
        m = (materials or scene).materials
        arrs = [np.ascontiguousarray(a) for a in (scene.nodes, scene.prims, m, scene.lights)]
        args = []
        for a in arrs:
            args += [a.ctypes.data_as(ctypes.c_void_p), a.nbytes]
        self._check(self._L.lt_hip_set_scene(self._ctx, *args))
        # keep the objects alive so that their ids cannot be recycled by a new scene
        self._scene_refs = (scene, materials or scene)
        self._scene_key = (id(scene), id(materials or scene))

    def invalidate_scene(self):
        """Forget the uploaded scene (call after modifying scene buffers in place)."""
        self._scene_key = None
        self._scene_refs = None

    def set_triangles(self, positions, normals, material_indices, materials, stream=None):
        """Makes a scene resident from bare triangles (lt_hip_set_triangles; include/lenstrace_hip.h defines the canonical median
        build): the tree, the ordered primitives and the light list are built on the GPU -- what
        scene.build_from_triangles_canonical builds on the host, byte for byte.  positions, normals: float32, 9 values per
        triangle ((n, 3, 3) or (n, 9)); material_indices: int32 (n,) or None (all 0); materials: MATERIAL_DTYPE records (or their
        bytes).  numpy arrays go to the host entry point; contiguous torch tensors on this context's GPU (materials then a uint8
        or float32 tensor of the records' bytes) go to the device one, which waits for the earlier work of `stream` (default: the
        current torch stream) and returns when the scene is resident."""
        vp = ctypes.c_void_p
        if isinstance(positions, np.ndarray):
            from .scene import _triangle_arrays
            pos, nrm, mi, mats = _triangle_arrays(positions, normals, material_indices, materials)
            d = C.TrianglesDesc(ctypes.sizeof(C.TrianglesDesc), 0, pos.shape[0], pos.ctypes.data_as(vp), nrm.ctypes.data_as(vp),
                                None if mi is None else mi.ctypes.data_as(vp), mats.ctypes.data_as(vp) if mats.size else None, mats.nbytes)
            rc = self._L.lt_hip_set_triangles(self._ctx, ctypes.byref(d))
        else:
            import torch
            dev = torch.device("cuda", self.device)
            wanted = (("positions", positions, torch.float32), ("normals", normals, torch.float32), ("material_indices", material_indices, torch.int32),
                      ("materials", materials, None))
            for what, t, dtype in wanted:
                if t is None and what == "material_indices":
                    continue
                if not isinstance(t, torch.Tensor) or t.device != dev or not t.is_contiguous() or (dtype is not None and t.dtype != dtype):
                    raise ValueError("%s must be a contiguous %s tensor on %s" % (what, dtype or "uint8 or float32", dev))
            if positions.numel() % 9 or normals.numel() != positions.numel() or \
                    (material_indices is not None and material_indices.numel() * 9 != positions.numel()):
                raise ValueError("triangle arrays disagree in length")
            if stream is None:
                stream = torch.cuda.current_stream(dev)
            handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
            d = C.TrianglesDesc(ctypes.sizeof(C.TrianglesDesc), 0, positions.numel() // 9, positions.data_ptr(), normals.data_ptr(),
                                None if material_indices is None else material_indices.data_ptr(),
                                materials.data_ptr() if materials.numel() else None, materials.numel() * materials.element_size())
            rc = self._L.lt_hip_set_triangles_device(self._ctx, ctypes.byref(d), vp(handle))
        self._check(rc)
        self.invalidate_scene()   # (render() hands its scene over again: the resident one is no Scene object's)

    def scene_buffers(self, camera=None):
        """lt_hip_read_scene_buffer: the four resident buffers -- nodes, primitives, materials, lights -- as a Scene, whichever
        call made them resident; `camera`: its 28-byte camera buffer (default: Scene's own)."""
        bufs = []
        for which in range(4):
            n = ctypes.c_uint64(0)
            self._check(self._L.lt_hip_read_scene_buffer(self._ctx, which, None, ctypes.c_uint64(0), ctypes.byref(n)))
            buf = np.zeros(n.value, dtype=np.uint8)
            self._check(self._L.lt_hip_read_scene_buffer(self._ctx, which, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(buf.nbytes),
                                                         ctypes.byref(n)))
            bufs.append(buf)
        return Scene(*bufs) if camera is None else Scene(*bufs, camera=bytes(camera))

    def resolve_program(self, kernel_file_path):
        """Built-in program by basename, or a user .hip file compiled with hipRTC at first use and cached by path."""
        out = ctypes.c_int(0)
        self._check(self._L.lt_hip_resolve_program(self._ctx, str(kernel_file_path).encode(), ctypes.byref(out)))
        return out.value

    # -- the plugin entry point ----------------------------------------------------------------------
    def render(self, props: RenderPropertiesHIP):
        W, H, D = props.imageDimensions
        out = props.pOutputBuffer
        if out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError("pOutputBuffer must be contiguous float32")
        a = props.pAccelerationStructureExplicit
        m = props.pModel or a
        program = self.resolve_program(props.kernelFilePath)
        d = make_desc(program, W, H, D, props.pCamera, props.kernelMode, props.frameFirst, props.frameCount,
                      props.accumulate, props.accumulateBase, None, props.giMaxDepth, props.collectStats, props.pixelCounters, props.portableMath, props.strictMath)
        # the reference uploads its scene on every call; a caller that versions its scene has it looked at only when the objects
        # or the number change, anyone else hands it over with the frame (lt_hip_render_scene: hashed in full while the frame
        # renders, uploaded -- and the frame rendered again -- only when a byte changed)
        key = (id(a), id(m))
        if props.sceneVersion and key == self._scene_key and props.sceneVersion == self._scene_version:
            self._check(self._L.lt_hip_render(self._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
            return
        arrs = [np.ascontiguousarray(x) for x in (a.nodes, a.prims, m.materials, a.lights)]
        args = []
        for x in arrs:
            args += [x.ctypes.data_as(ctypes.c_void_p), x.nbytes]
        self._check(self._L.lt_hip_render_scene(self._ctx, *args, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        self._scene_refs = (a, m)
        self._scene_key = key
        self._scene_version = props.sceneVersion

    # -- device-resident variants (bench / multi-GPU) -----------------------------------------------------
    def output_floats(self, desc):
        n = ctypes.c_uint64(0)
        self._check(self._L.lt_hip_output_floats(ctypes.byref(desc), ctypes.byref(n)))
        return n.value

    def render_device(self, desc, out_ptr, out_bytes, stream=0):
        self._check(self._L.lt_hip_render_device(self._ctx, ctypes.byref(desc), ctypes.c_void_p(out_ptr), out_bytes,
                                                 ctypes.c_void_p(stream)))

    def untile(self, gathered_ptr, floats_per_rank, n_ranks, W, H, D, tile_w, tile_h, image_ptr, stream=0):
        self._check(self._L.lt_hip_untile(self._ctx, ctypes.c_void_p(gathered_ptr), floats_per_rank, n_ranks, W, H, D,
                                          tile_w, tile_h, ctypes.c_void_p(image_ptr), ctypes.c_void_p(stream)))

    def synchronize(self, stream=0):
        self._check(self._L.lt_hip_synchronize(self._ctx, ctypes.c_void_p(stream)))

    def camera_hit_passes(self):
        """lt_hip_camera_hit_passes: camera-hit passes this context has launched.  accumulator keeps a call's camera hits, and a call
        with the same scene, camera, image, tiles and math flavour as the one before it (frame_first may move on) launches none."""
        return int(self._L.lt_hip_camera_hit_passes(self._ctx))

    def entry_cut_counts(self):
        """lt_hip_entry_cut_counts: (builds of entry cuts so far, squares whose list is not empty, entries of those lists) -- the
        last two of the cuts the context holds now.  The cuts are kept with the camera hits: the first call that reuses a set of
        hits builds them, later ones build none.  Waits for the context's last render.  LT_ENTRY_CUT=0: (0, 0, 0)."""
        out = (ctypes.c_uint64 * 3)()
        self._check(self._L.lt_hip_entry_cut_counts(self._ctx, out))
        return int(out[0]), int(out[1]), int(out[2])

    def entry_cut_leaf_counts(self):
        """lt_hip_entry_cut_leaf_counts: (squares the cuts' leaf pass marked clear -- their two-frame shadow walks are not run --,
        squares whose list is leaves, entries of those lists), of the cuts the context holds now.  entry_cut_counts keeps
        describing the node lists.  Waits for the context's last render.  LT_ENTRY_CUT_LEAVES=0: (0, 0, 0)."""
        out = (ctypes.c_uint64 * 3)()
        self._check(self._L.lt_hip_entry_cut_leaf_counts(self._ctx, out))
        return int(out[0]), int(out[1]), int(out[2])

    def entry_cut_chunk_counts(self):
        """lt_hip_entry_cut_chunk_counts, of the cuts the context holds now: a dict of `chunks` (the records a list may take,
        LT_ENTRY_CUT_CHUNKS), `leaf` and `plain` ((squares, entries) of the lists of leaves and of the node cuts that take more
        than one record), `pruned` ((squares, entries) of the cuts over the pruned tree) and `squares_by_chunks` (k -> the squares
        whose list takes k records, k = 1 .. 16).  Waits for the context's last render.  All zero while the context holds no
        cuts."""
        out = (ctypes.c_uint64 * 23)()
        self._check(self._L.lt_hip_entry_cut_chunk_counts(self._ctx, out))
        return {"chunks": int(out[0]), "leaf": (int(out[1]), int(out[2])), "pruned": (int(out[3]), int(out[4])),
                "plain": (int(out[5]), int(out[6])), "squares_by_chunks": {k: int(out[6 + k]) for k in range(1, 17)}}

    def entry_cuts(self):
        """lt_hip_read_entry_cuts: the entry cuts the context holds now as the two-frame shadow walks read them, a (planes x squares,
        16) uint32 array -- plane c holds record c of every square's list in hand-out order: a count (0xffffffff: marked clear), then
        that many references -- or None while it holds none.  Waits for the device."""
        n = ctypes.c_uint64(0)
        self._check(self._L.lt_hip_read_entry_cuts(self._ctx, None, ctypes.c_uint64(0), ctypes.byref(n)))
        if n.value == 0:
            return None
        buf = np.zeros(n.value // 4, dtype=np.uint32)
        self._check(self._L.lt_hip_read_entry_cuts(self._ctx, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(buf.nbytes), ctypes.byref(n)))
        return buf.reshape(-1, 16)

    def clear_item_counts(self):
        """lt_hip_clear_item_counts, of the item table the context holds now: a dict of `entries` (the table's work items),
        `whole` (the clear squares it hands out as one item each), `folded` (those of them whose samples the context's last
        render launch folded by their own wave: all or none) and `builds` (tables built so far).  Waits for the context's last
        render.  LT_CLEAR_ITEMS=0, or no cuts kept: all but `builds` zero."""
        out = (ctypes.c_uint64 * 5)()
        self._check(self._L.lt_hip_clear_item_counts(self._ctx, out))
        return {"entries": int(out[0]), "whole": int(out[1]), "folded": int(out[2]), "builds": int(out[3]), "used": bool(out[4])}

    def clear_square_counts(self):
        """lt_hip_clear_square_counts, of the context's last render launch: a dict of `entered` (clear squares whose frame groups
        one pass over the square began to render), `left` (those of them that went back to the per-group path before their last
        group) and `groups` (frame groups rendered in that pass).  Waits for the context's last render.  LT_CLEAR_SQUARE=0, or no
        item table: all zero."""
        out = (ctypes.c_uint64 * 3)()
        self._check(self._L.lt_hip_clear_square_counts(self._ctx, out))
        return {"entered": int(out[0]), "left": int(out[1]), "groups": int(out[2])}

    def scene_structure(self, what):
        """lt_hip_read_scene_structure: 0 own tree (NODE_DTYPE array), 1 leaf order table (n_prims x 8 uint32), 2 the per-lane walks'
        array (bytes), 3 (own height, group-tree height, groups, prepared on the device), 4 the packet walks' records (bytes, 64 per
        node of the own tree), 5 the traversal triangles (bytes, 48 per primitive).  None when the scene has no such structure
        (kinds 0, 1, 2 and 4 of a scene that walks the caller's tree)."""
        from . import scene as sc
        n = ctypes.c_uint64(0)
        self._check(self._L.lt_hip_read_scene_structure(self._ctx, what, None, ctypes.c_uint64(0), ctypes.byref(n)))
        if n.value == 0:
            return None
        buf = np.zeros(n.value, dtype=np.uint8)
        self._check(self._L.lt_hip_read_scene_structure(self._ctx, what, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(buf.nbytes), ctypes.byref(n)))
        if what == 0:
            return buf.view(sc.NODE_DTYPE)
        if what == 1:
            return buf.view(np.uint32).reshape(-1, 8)
        if what == 3:
            return tuple(int(x) for x in buf.view(np.int32))
        return buf

    # -- ray queries ------------------------------------------------------------------------------------
    def _host_call(self, name, d, records, out):
        """lt_hip_<name> over a contiguous numpy array of records; fills and returns `out`, one result per record."""
        self._check(getattr(self._L, "lt_hip_" + name)(self._ctx, ctypes.byref(d), records.ctypes.data_as(ctypes.c_void_p), records.shape[0],
                                                       out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    def _device_call(self, name, d, records, what, lead, width, result, stream):
        """lt_hip_<name>_device over a contiguous (`lead`, width) float32 tensor of records on this context's GPU (lead "n": two
        dimensions, "...": any number), enqueued on `stream`; returns a new tensor of dtype result[0] whose last dimension is
        replaced by the shape result[1]."""
        import torch
        if not isinstance(records, torch.Tensor):
            raise TypeError("%s must be a numpy array or a torch tensor" % what)
        dims_ok = records.dim() == 2 if lead == "n" else records.dim() >= 1
        if records.dtype != torch.float32 or not dims_ok or records.shape[-1] != width or not records.is_contiguous():
            raise ValueError("%s must be a contiguous (%s, %d) float32 tensor" % (what, lead, width))
        dev = torch.device("cuda", self.device)
        if records.device != dev:
            raise ValueError("%s must be on %s, the context's device" % (what, dev))
        out = torch.empty(tuple(records.shape[:-1]) + result[1], dtype=getattr(torch, result[0]), device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        self._check(getattr(self._L, "lt_hip_" + name + "_device")(self._ctx, ctypes.byref(d), ctypes.c_void_p(records.data_ptr()),
                                                                   records.numel() // width, ctypes.c_void_p(out.data_ptr()),
                                                                   out.numel() * out.element_size(), ctypes.c_void_p(handle)))
        return out

    def _ray_call(self, name, d, rays, kind, host_result, device_result, stream):
        """Rays through lt_hip_<name>: a numpy batch (kind: ray_records' arguments) gives numpy -- host_result: (dtype, shape per
        ray) --, a torch tensor gives torch -- device_result: the same with the dtype's name."""
        if isinstance(rays, np.ndarray):
            rays = ray_records(rays, *kind)
            return self._host_call(name, d, rays, np.zeros((rays.shape[0],) + host_result[1], dtype=host_result[0]))
        return self._device_call(name, d, rays, "rays", "n", 8, device_result, stream)

    def trace_rays(self, rays, any_hit=False, program="accumulator", coherent=False, portable_math=False, strict_math=False, stream=None):
        """Traces caller-supplied rays against the scene of the last set_scene / render (lt_hip_trace_rays): as the reference's
        intersect / intersectIgnorePrimitiveIndex would, with the triangle epsilon of `program` (an LT_PROGRAM_* id or a kernel path).
        rays: an (n, 8) float32 array of lt_hip_ray records (make_rays) or a RAY_DTYPE array -- then the host entry point runs and
        numpy comes back: a HIT_DTYPE array (t, prim -- -1 on a miss --, u, v) or, any_hit, uint32 occluded words; or a contiguous
        (n, 8) float32 torch tensor on this context's GPU -- then the query is enqueued on `stream` (default: the current torch
        stream) and torch comes back: an (n, 4) float32 tensor of lt_hip_hit records (column 1 holds int32 bits: .view(torch.int32))
        or an (n,) int32 tensor of occluded words.  coherent: runs of 64 consecutive rays are coherent (LT_TRACE_FLAG_COHERENT)."""
        d = C.TraceDesc(ctypes.sizeof(C.TraceDesc), _program_id(program), C.TRACE_ANY if any_hit else C.TRACE_CLOSEST,
                        _ray_flags(coherent, portable_math, strict_math))
        return self._ray_call("trace_rays", d, rays, _QUERY_RAYS, (np.uint32, ()) if any_hit else (HIT_DTYPE, ()),
                              ("int32", ()) if any_hit else ("float32", (4,)), stream)

    def trace_hits(self, rays, max_hits=4, count=False, program="accumulator", portable_math=False, strict_math=False, coherent=False,
                   stream=None):
        """The first `max_hits` (1..C.TRACE_MAX_HITS) hits of each ray, nearest first, or with count=True how many there are
        (lt_hip_trace_hits; include/lenstrace_hip.h defines the hit sequence: every primitive the reference's traversal accepts
        with t < tmax, by t, bit-equal t in the reference's traversal order).  Rays as trace_rays takes them.  A numpy array goes
        to the host entry point and numpy comes back: an (n, max_hits) HIT_DTYPE array whose unused slots are miss records
        (t = tmax, prim -1), or (n,) uint32 counts; a torch tensor on this context's GPU is enqueued on `stream` (default: the
        current torch stream) and torch comes back: (n, max_hits, 4) float32 (column 1: int32 bits) or (n,) int32 counts.
        coherent is accepted and changes nothing: these queries have no packet walk."""
        d = C.MultiHitDesc(ctypes.sizeof(C.MultiHitDesc), _program_id(program), C.TRACE_COUNT if count else C.TRACE_FIRST_K,
                           _ray_flags(coherent, portable_math, strict_math), 0 if count else max_hits)
        if not count and not 1 <= max_hits <= C.TRACE_MAX_HITS:
            raise ValueError("max_hits must be in 1..%d" % C.TRACE_MAX_HITS)
        k = 0 if count else int(max_hits)
        return self._ray_call("trace_hits", d, rays, _QUERY_RAYS, (np.uint32, ()) if count else (HIT_DTYPE, (k,)),
                              ("int32", ()) if count else ("float32", (k, 4)), stream)

    def trace_hits_list(self, rays, program="accumulator", portable_math=False, strict_math=False, coherent=False, stream=None):
        """Every hit of each ray, nearest first, as CSR (lt_hip_trace_hits_list): (offsets, items) with items[offsets[i] :
        offsets[i + 1]] the whole hit sequence of ray i -- trace_hits' records (t, prim, u, v) without the limit of eight and
        without miss records; surface_at takes them as they are.  Rays, program and the math flags as trace_hits takes them:
        numpy in gives numpy, offsets uint64 (n + 1,) and items HIT_DTYPE (total,); a torch tensor on this context's GPU gives
        tensors, offsets as int64 and items float32 (total, 4) (column 1: int32 bits), after the sizing call, one read of the
        total and the fill call on `stream` (default: the current torch stream).  coherent is accepted and changes nothing."""
        prog, flags = _program_id(program), _ray_flags(coherent, portable_math, strict_math)

        def describe(list_flags):
            return C.HitsListDesc(ctypes.sizeof(C.HitsListDesc), prog, flags | list_flags, 0)
        if isinstance(rays, np.ndarray):
            return self._list_call("trace_hits", rays, lambda r: ray_records(r, *_QUERY_RAYS), "rays", 8, stream, _HITS_LIST, describe)
        return self._list_call("trace_hits", rays, None, "rays", 8, stream, _HITS_LIST, describe)

    # -- surface queries -------------------------------------------------------------------------------
    def trace_surface(self, rays, program="accumulator", coherent=False, portable_math=False, strict_math=False, stream=None):
        """Closest hits with the surface behind them (lt_hip_trace_surface): for each ray trace_rays' record (t, prim, u, v), the
        position A*b.x + B*b.y + C*b.z the reference's shade starts its next ray from, the interpolated vertex normal (not
        normalised), the primitive's material index and flags (C.SURFACE_LIGHT: the primitive is in the light list); on a miss
        position = normal = 0, material = -1, flags = 0.  Rays, program and coherent as trace_rays takes them.  A numpy array goes
        to the host entry point and an (n,) SURFACE_DTYPE array comes back; a contiguous (n, 8) float32 torch tensor on this
        context's GPU is enqueued on `stream` (default: the current torch stream) and an (n, 12) float32 tensor comes back
        (columns 1, 7 and 11 hold integer bits: .view(torch.int32))."""
        d = C.TraceDesc(ctypes.sizeof(C.TraceDesc), _program_id(program), C.TRACE_CLOSEST, _ray_flags(coherent, portable_math, strict_math))
        return self._ray_call("trace_surface", d, rays, _QUERY_RAYS, (SURFACE_DTYPE, ()), ("float32", (12,)), stream)

    def surface_at(self, hits, portable_math=False, strict_math=False, stream=None):
        """The surface records of hit records the caller has (lt_hip_surface_at) -- above all trace_hits' K per ray: t, u and v
        copied, position, normal, material and flags as trace_surface gives them; a record whose prim is none of the scene's
        primitives gives the miss form (prim = -1, u = v = 0).  hits: a HIT_DTYPE array of any shape -- then the host entry point
        runs and a SURFACE_DTYPE array of the same shape comes back; or a contiguous (..., 4) float32 torch tensor on this
        context's GPU -- then the call is enqueued on `stream` (default: the current torch stream) and a (..., 12) float32 tensor
        comes back."""
        d = C.SurfaceDesc(ctypes.sizeof(C.SurfaceDesc), _ray_flags(False, portable_math, strict_math))
        if isinstance(hits, np.ndarray):
            if hits.dtype != HIT_DTYPE:
                raise ValueError("hits must be a HIT_DTYPE array")
            flat = np.ascontiguousarray(hits).reshape(-1)
            return self._host_call("surface_at", d, flat, np.zeros(flat.shape[0], dtype=SURFACE_DTYPE)).reshape(hits.shape)
        return self._device_call("surface_at", d, hits, "hits", "...", 4, ("float32", (12,)), stream)

    # -- nearest-point queries -------------------------------------------------------------------------
    def nearest_points(self, points, max_d2=np.inf, stream=None):
        """The closest primitive of each point (lt_hip_nearest_points; include/lenstrace_hip.h defines the distance and the
        selection): records (t = the squared distance, prim, u, v) that surface_at turns into the closest point, its normal and
        material; a miss -- nothing with a squared distance below max_d2 -- has prim = -1 and t = max_d2.
        points: an (n, 3) numpy array with max_d2 a scalar or an (n,) array, or ready lt_hip_point records (an (n, 4) float32 array
        from make_points, or a POINT_DTYPE array) -- then the host entry point runs and a HIT_DTYPE array comes back; or a
        contiguous float32 torch tensor on this context's GPU, (n, 3) with max_d2 a scalar or an (n,) tensor, or (n, 4) records --
        then the call is enqueued on `stream` (default: the current torch stream) and an (n, 4) float32 tensor of lt_hip_hit
        records comes back (column 1 holds int32 bits: .view(torch.int32))."""
        d = C.NearestDesc(ctypes.sizeof(C.NearestDesc), 0)
        if isinstance(points, np.ndarray):
            pts = point_records(points, max_d2)
            return self._host_call("nearest_points", d, pts, np.zeros(pts.shape[0], dtype=HIT_DTYPE))
        return self._device_call("nearest_points", d, self._point_tensor(points, max_d2, stream), "points", "n", 4, ("float32", (4,)), stream)

    @staticmethod
    def _point_tensor(points, max_d2, stream):
        """A torch batch of points as lt_hip_point records: (n, 3) positions are packed with max_d2, anything else is left to
        _device_call's checks."""
        import torch
        if isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[1] == 3:
            m = torch.as_tensor(max_d2, dtype=torch.float32, device=points.device)
            if m.shape not in ((), (points.shape[0],)):
                raise ValueError("max_d2 must be a scalar or have shape (n,)")
            # (the records are packed by torch, on the call's stream when it is a torch stream, else on the current one)
            with torch.cuda.stream(stream if isinstance(stream, torch.cuda.Stream) else None):
                points = torch.cat([points, m.expand(points.shape[0]).unsqueeze(1)], dim=1).contiguous()
        return points

    def nearest_k(self, points, k=4, count=False, max_d2=np.inf, stream=None):
        """The `k` (1..C.NEAREST_MAX_K) closest primitives of each point, nearest first, or with count=True how many lie within
        max_d2 (lt_hip_nearest_k; include/lenstrace_hip.h defines the candidate sequence: nearest_points' candidates by squared
        distance, the lower primitive offset first among equal ones).  Points and max_d2 as nearest_points takes them.  A numpy
        batch goes to the host entry point and numpy comes back: an (n, k) HIT_DTYPE array whose unused slots are miss records
        (t = max_d2, prim -1), or (n,) uint32 counts; a torch tensor on this context's GPU is enqueued on `stream` (default: the
        current torch stream) and torch comes back: (n, k, 4) float32 (column 1: int32 bits) or (n,) int32 counts.  A count with
        max_d2 = inf visits every leaf for every point."""
        d = _nearest_k_desc(k, count)
        k = 0 if count else int(k)
        if isinstance(points, np.ndarray):
            pts = point_records(points, max_d2)
            return self._host_call("nearest_k", d, pts, np.zeros(pts.shape[0], dtype=np.uint32) if count else np.zeros((pts.shape[0], k), dtype=HIT_DTYPE))
        return self._device_call("nearest_k", d, self._point_tensor(points, max_d2, stream), "points", "n", 4,
                                 ("int32", ()) if count else ("float32", (k, 4)), stream)

    def nearest_list(self, points, max_d2=np.inf, stream=None):
        """Every primitive within each point's radius, as CSR (lt_hip_nearest_list): (offsets, items) with items[offsets[i] :
        offsets[i + 1]] the whole candidate sequence of point i -- nearest_k's records (t = the squared distance, prim, u, v),
        nearest first, without the limit of eight; surface_at takes them as they are.  Points and max_d2 as nearest_k takes
        them: numpy in gives numpy, offsets uint64 (n + 1,) and items HIT_DTYPE (total,); a torch tensor on this context's GPU
        gives tensors, offsets as int64 and items float32 (total, 4) (column 1: int32 bits), after the sizing call, one read of
        the total and the fill call on `stream` (default: the current torch stream).  max_d2 = inf lists every leaf for every
        point: give a finite radius."""
        if isinstance(points, np.ndarray):
            return self._list_call("nearest", point_records(points, max_d2), lambda rec: rec, "points", 4, stream, _NEAREST_LIST)
        return self._list_call("nearest", self._point_tensor(points, max_d2, stream), None, "points", 4, stream, _NEAREST_LIST)

    # -- box-overlap queries ---------------------------------------------------------------------------
    def overlap_boxes(self, boxes, k=None, count=False, any=False, stream=None):
        """The primitives each axis-aligned box touches (lt_hip_overlap_boxes; include/lenstrace_hip.h defines "touches": the
        leaf's box meets the box and the triangle passes the 13-axis test): the `k` (1..C.OVERLAP_MAX_K, default 4) lowest
        primitive offsets in ascending order, -1 in unused slots; with count=True how many there are; with any=True 1 or 0.  A box
        with a bound that is not finite or with lo > hi on an axis touches nothing.
        boxes: an (n, 8) float32 array of lt_hip_box records (make_boxes) or a BOX_DTYPE array -- then the host entry point runs
        and numpy comes back: (n, k) int32 or (n,) uint32; or a contiguous (n, 8) float32 torch tensor on this context's GPU --
        then the call is enqueued on `stream` (default: the current torch stream) and torch comes back: (n, k) int32 or (n,)
        int32."""
        d = _overlap_desc(k, count, any)
        if isinstance(boxes, np.ndarray):
            bx = box_records(boxes)
            out = np.zeros((bx.shape[0], d.max_k), dtype=np.int32) if d.max_k else np.zeros(bx.shape[0], dtype=np.uint32)
            return self._host_call("overlap_boxes", d, bx, out)
        return self._device_call("overlap_boxes", d, boxes, "boxes", "n", 8, ("int32", (d.max_k,) if d.max_k else ()), stream)

    # -- triangle-overlap queries ----------------------------------------------------------------------
    def overlap_tris(self, tris, k=None, count=False, any=False, stream=None):
        """The primitives each query triangle meets (lt_hip_overlap_tris; include/lenstrace_hip.h defines "touches": the leaf's
        box meets the triangle's box and none of 17 axes separates the two triangles): the `k` (1..C.OVERLAP_MAX_K, default 4)
        lowest primitive offsets in ascending order, -1 in unused slots; with count=True how many there are; with any=True 1 or 0.
        A triangle with a coordinate that is not finite meets nothing; a needle or a point is a valid query.
        tris: an (n, 12) float32 array of lt_hip_tri records (make_tris) or a TRI_DTYPE array -- then the host entry point runs
        and numpy comes back: (n, k) int32 or (n,) uint32; or a contiguous (n, 12) float32 torch tensor on this context's GPU --
        then the call is enqueued on `stream` (default: the current torch stream) and torch comes back: (n, k) int32 or (n,)
        int32."""
        d = _overlap_desc(k, count, any)
        if isinstance(tris, np.ndarray):
            tr = tri_records(tris)
            out = np.zeros((tr.shape[0], d.max_k), dtype=np.int32) if d.max_k else np.zeros(tr.shape[0], dtype=np.uint32)
            return self._host_call("overlap_tris", d, tr, out)
        return self._device_call("overlap_tris", d, tris, "tris", "n", 12, ("int32", (d.max_k,) if d.max_k else ()), stream)

    # -- overlap lists ----------------------------------------------------------------------------------
    def _list_call(self, name, records, numpy_records, what, width, stream, family=_OVERLAP_LIST, describe=None):
        """lt_hip_<name>_list: numpy in, the host entry point sized and then filled; a torch tensor in, the device entry point --
        the sizing call, one .item() for the total, the items allocated, the family's FILL_ONLY call.  describe(flags): the
        family's descriptor with these list flags, where it holds more than its size and flags (a program, math flags)."""
        vp = ctypes.c_void_p
        Desc, fill_only, item, (tdtype, tshape) = family
        size = ctypes.sizeof(Desc)
        if describe is None:
            describe = lambda flags: Desc(size, flags)  # noqa: E731
        sizing, fill = describe(0), describe(fill_only)
        if isinstance(records, np.ndarray):
            rec = numpy_records(records)
            f = getattr(self._L, "lt_hip_%s_list" % name)
            offsets = np.zeros(rec.shape[0] + 1, dtype=np.uint64)
            self._check(f(self._ctx, ctypes.byref(sizing), rec.ctypes.data_as(vp), rec.shape[0], offsets.ctypes.data_as(vp), offsets.nbytes, None, 0))
            items = np.zeros(int(offsets[-1]), dtype=item)
            if len(items):
                self._check(f(self._ctx, ctypes.byref(fill), rec.ctypes.data_as(vp), rec.shape[0], offsets.ctypes.data_as(vp), offsets.nbytes,
                              items.ctypes.data_as(vp), items.nbytes))
            return offsets, items
        import torch
        if not isinstance(records, torch.Tensor):
            raise TypeError("%s must be a numpy array or a torch tensor" % what)
        if records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != width or not records.is_contiguous():
            raise ValueError("%s must be a contiguous (n, %d) float32 tensor" % (what, width))
        dev = torch.device("cuda", self.device)
        if records.device != dev:
            raise ValueError("%s must be on %s, the context's device" % (what, dev))
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        if not hasattr(stream, "cuda_stream"):
            stream = torch.cuda.ExternalStream(int(stream), device=dev)
        handle = stream.cuda_stream
        f = getattr(self._L, "lt_hip_%s_list_device" % name)
        n = records.shape[0]
        with torch.cuda.stream(stream):     # (the total is read on the stream the sizing call runs on)
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)     # (uint64 words: torch has no arithmetic on them)
            self._check(f(self._ctx, ctypes.byref(sizing), vp(records.data_ptr()), n, vp(offsets.data_ptr()), 8 * (n + 1), None, 0, vp(handle)))
            total = int(offsets[-1].item())
            items = torch.empty((total,) + tshape, dtype=getattr(torch, tdtype), device=dev)
            if total:
                self._check(f(self._ctx, ctypes.byref(fill), vp(records.data_ptr()), n, vp(offsets.data_ptr()), 8 * (n + 1),
                              vp(items.data_ptr()), items.numel() * items.element_size(), vp(handle)))
        return offsets, items

    def overlap_boxes_list(self, boxes, stream=None):
        """Every primitive each box touches, as CSR (lt_hip_overlap_boxes_list): (offsets, items) with items[offsets[i] :
        offsets[i + 1]] the whole sequence of box i -- overlap_boxes' offsets, ascending, without the limit of eight.  boxes as
        overlap_boxes takes them: numpy in gives numpy, offsets uint64 (n + 1,) and items int32 (total,); a torch tensor on this
        context's GPU gives tensors, offsets as int64, after the sizing call, one read of the total and the fill call on `stream`
        (default: the current torch stream)."""
        return self._list_call("overlap_boxes", boxes, box_records, "boxes", 8, stream)

    def overlap_tris_list(self, tris, stream=None):
        """Every primitive each query triangle meets, as CSR (lt_hip_overlap_tris_list): overlap_boxes_list's (offsets, items)
        for tris as overlap_tris takes them."""
        return self._list_call("overlap_tris", tris, tri_records, "tris", 12, stream)

    # -- shaded rays ------------------------------------------------------------------------------------
    def shade_rays(self, rays, program="accumulator", frame_first=0, frame_count=1, kernel_mode=KERNEL_MODE_LINEAR, portable_math=False,
                   strict_math=False, coherent=False, stream=None):
        """Shades caller-supplied rays (lt_hip_shade_rays): for each ray the colour `program`'s shade returns for it -- what the
        render kernels would have stored had it been a pixel's camera ray at that film position -- for frames frame_first ..
        frame_first + frame_count - 1, folded by the running mean, and the primitive the ray itself hit (-1: none).  Programs:
        basic, basic_lighting, accumulator, custom_opencl (an LT_PROGRAM_* id or a kernel path).
        rays: an (n, 8) float32 array of lt_hip_shade_ray records (make_shade_rays) or a SHADE_RAY_DTYPE array -- then the host
        entry point runs and a SHADE_DTYPE array (rgb, prim) comes back; or a contiguous (n, 8) float32 torch tensor on this
        context's GPU -- then the call is enqueued on `stream` (default: the current torch stream) and an (n, 4) float32 tensor
        comes back (column 3 holds int32 bits: .view(torch.int32)).  coherent is accepted and changes nothing: there is no
        packet path."""
        d = C.ShadeDesc(ctypes.sizeof(C.ShadeDesc), _program_id(program), kernel_mode, _ray_flags(coherent, portable_math, strict_math),
                        frame_first, frame_count)
        return self._ray_call("shade_rays", d, rays, _SHADE_RAYS, (SHADE_DTYPE, ()), ("float32", (4,)), stream)

    # -- shaded paths -----------------------------------------------------------------------------------
    def shade_paths(self, rays, program="global_illumination", gi_max_depth=0, frame_first=0, frame_count=1, kernel_mode=KERNEL_MODE_LINEAR,
                    portable_math=False, strict_math=False, coherent=False, stream=None):
        """Shades caller-supplied rays with a global-illumination program (lt_hip_shade_paths): for each ray what a render of
        `program` (global_illumination, global_illumination25: an LT_PROGRAM_* id or a kernel path) leaves in a pixel whose
        camera ray it is, for frames frame_first .. frame_first + frame_count - 1 folded by the running mean, with paths of at most
        gi_max_depth bounces (0: the reference's 16), and the primitive the ray itself hit (-1: none).
        rays and the result: shade_rays' contract -- an (n, 8) float32 array (make_shade_rays) or a SHADE_RAY_DTYPE array in, a
        SHADE_DTYPE array out; or a contiguous (n, 8) float32 torch tensor on this context's GPU in, enqueued on `stream` (default:
        the current torch stream), an (n, 4) float32 tensor out (column 3 holds int32 bits).  coherent is accepted and changes
        nothing."""
        d = C.PathsDesc(ctypes.sizeof(C.PathsDesc), _program_id(program), kernel_mode, _ray_flags(coherent, portable_math, strict_math),
                        frame_first, frame_count, gi_max_depth)
        return self._ray_call("shade_paths", d, rays, _SHADE_RAYS, (SHADE_DTYPE, ()), ("float32", (4,)), stream)

    def stats(self):
        s = C.Stats()
        self._check(self._L.lt_hip_get_stats(self._ctx, ctypes.byref(s)))
        return s.as_dict()
