"""Fixtures and checkers of the tests whose buffers pass 2^31 and 2^32 bytes (tests/test_gpu_large_offsets.py; what this module
claims: tests/test_large_offsets_cpu.py).

At these sizes the CPU oracle cannot say what every record holds, so a ray case is PERIODIC: a base batch of B rays whose result
the oracle settles bit for bit, repeated on the device until it has n records.  Record i of the large result must then hold the
bits of record i % B of the base result.  A store whose 32-bit offset wrapped lands inside the buffer: it leaves the sentinel in
a record beyond 2^32 bytes and the wrong repetition's bits in a record near the start, and check_periodic reports both.

* CASES: the ray cases -- entry point, n, bytes of a record in and out, the base batch, what crosses which power of two;
* query_base / coherent_base / shade_base: the base batches on the Cornell box (tests/golden/cornell_box_O0.ltsb), drawn with
  the building blocks of tests/query_edges.py, and the oracle's word on each of them;
* check_periodic(out, base): the comparison, in pieces, on whichever device the tensors live; Report says how many records
  differ, where the first and the last are, and whether they pair up as a wrap modulo 2^32 would pair them;
* R1, R2, R4: the render cases' shapes, cameras and oracle rows (oracle_rows: rows of an image too large to allocate)."""
import ctypes
import functools
import math
from dataclasses import dataclass

import numpy as np

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import FLT_MAX, HIT_DTYPE, make_rays
from oracle import pyoracle as po
from tests import multihit as mh
from tests import octant_scenes as oc
from tests import query_edges as qe
from tests import shade_paths as P
from tests import shade_rays as F
from tests import surface as S

F32 = np.float32
SENTINEL = 0x7fa5a5a5            # a NaN no result holds: not a tmax of the batches, not the oracle's centre-column NaN (0x7fc00000)
SCENE = "cornell_box_O0"
B_PRIME = 4099                   # prime: every repetition meets the 64-lane chunks (and the 512-ray claims) at another alignment
B_COHERENT = 64 * 65             # whole chunks, and an odd number of them: 2^32 / record bytes is no multiple of B
LANES = qe.LANES
N_RAYS = 2 ** 27 + 2 ** 20 + 37
N_HITS = 2 ** 25 + 2 ** 12 + 5
N_SURFACE = 90_000_037
K_HITS = 8

# bytes of the records, from the binding's structures (include/lenstrace_hip.h)
RAY, HIT, SURFACE = ctypes.sizeof(C.TraceRay), ctypes.sizeof(C.TraceHit), ctypes.sizeof(C.Surface)
SHADE_RAY, SHADE, WORD = ctypes.sizeof(C.ShadeRay), ctypes.sizeof(C.ShadeResult), 4


@dataclass(frozen=True)
class Case:
    call: str            # RendererHIP's method
    n: int
    in_record: int       # bytes
    out_record: int
    base: str            # "prime" (B_PRIME rays), "coherent" (B_COHERENT), "shade" (B_PRIME shade rays), "hits" (the prime batch's hits)
    in_crosses: int      # the power of two the input passes (0: none claimed)
    out_crosses: int
    kw: tuple = ()       # the method's keyword arguments, but the math flavour

    @property
    def in_bytes(self):
        return self.n * self.in_record

    @property
    def out_bytes(self):
        return self.n * self.out_record

    @property
    def period(self):
        return B_COHERENT if self.base == "coherent" else B_PRIME


CASES = {
    "closest": Case("trace_rays", N_RAYS, RAY, HIT, "prime", 2 ** 32, 2 ** 31),
    "closest_coherent": Case("trace_rays", N_RAYS, RAY, HIT, "coherent", 2 ** 32, 2 ** 31, (("coherent", True),)),
    "any_coherent": Case("trace_rays", N_RAYS, RAY, WORD, "coherent", 2 ** 32, 0, (("coherent", True), ("any_hit", True))),
    "hits8": Case("trace_hits", N_HITS, RAY, K_HITS * HIT, "prime", 0, 2 ** 32, (("max_hits", K_HITS),)),
    "surface": Case("trace_surface", N_SURFACE, RAY, SURFACE, "prime", 2 ** 31, 2 ** 32),
    "surface_at": Case("surface_at", N_SURFACE, HIT, SURFACE, "hits", 0, 2 ** 32),
    "shade_rays": Case("shade_rays", N_RAYS, SHADE_RAY, SHADE, "shade", 2 ** 32, 2 ** 31, (("program", "accumulator"), ("frame_count", 2))),
    "shade_paths": Case("shade_paths", N_RAYS, SHADE_RAY, SHADE, "shade", 2 ** 32, 2 ** 31,
                        (("program", "global_illumination"), ("gi_max_depth", 2), ("frame_count", 1))),
}


# Device memory of a case: its records in and out, what the library allocates for the call, and the comparison.
PATHS_SLOTS = 2 ** 24            # LT_PATHS_SLOTS of the shade_paths case: at the default (63 M slots) its path queues alone take 12.3 GB
GI_SLOT_BYTES = 17 * 16          # ensure_gi_buffers: seventeen arrays of 16 bytes per path slot
COMPARE_BYTES = 2 ** 30          # check_periodic: two masks of n bytes, the temporaries of one piece of 2^29 bytes; the base batch
DEVICE_LIMIT = 16 * 2 ** 30      # no test holds more


def paths_sets(n, frames=1, slots=PATHS_SLOTS):
    """(sets, rays per set) of lt_hip_shade_paths for n rays of `frames` frames (enqueue_paths, one sample per frame)"""
    at_most = min(n, max(1, slots // frames))
    ranges = -(-n // at_most)
    return ranges, -(-n // ranges)


def scratch_bytes(case):
    """what the library allocates on the device for the call"""
    if case.call == "trace_surface":
        return case.n * HIT                                      # lt_hip_trace_rays' hits, for lt_hip_surface_at's launch over them
    if case.call == "shade_paths":
        return paths_sets(case.n)[1] * (GI_SLOT_BYTES + 16)      # the path queues and the camera hits of one set
    return 0


def device_bytes(case):
    """the device memory the case states as its need"""
    return case.in_bytes + case.out_bytes + scratch_bytes(case) + COMPARE_BYTES


HOST_FORM_BYTES = N_RAYS * (RAY + HIT)       # the host-form case: the context's two staging buffers
R1_BYTES = 2 * 16384 * 16400 * 16 + 9 * 16384 * 2048 * 16 + 2 ** 29   # the image twice, nine bands of 512 MiB, a piece's comparison
R3_BYTES = 2 * 16384 * 16400 * 16 + 2 ** 30  # the image in the caller's buffer and in the context's, a piece of the host's on the device
R2_BYTES = 44 * 3840 * 2160 * 12 + 8 * 3840 * 2160 * 12 + 2 ** 29   # the sample scratch; images, camera hits and shadow queue beside it


def scene():
    return F.scene(SCENE)


# ------------------------------------------------------------------------------------------------- base batches of the queries
CENTRE = np.array(F.CENTRE)     # of the box; its half extent is 2.5
STANDOFF = 8.0                  # origins of the coherent chunks: this far from the centre on every axis, jitter below 1


def all_prims(s):
    P3 = qe.corners(s)
    area = np.linalg.norm(np.cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0]), axis=1)
    return np.flatnonzero(area > 1e-3)


def octant_chunk(s, k, rng, jitter=False, away=False):
    """query_edges.coherent_chunk for the box: 64 rays of octant k from one origin (or 64 nearby ones) outside the box onto points
    of its triangles: every component of target - origin has the octant's sign (|target - centre| <= 2.5 < 8 - 1).  away: the
    same rays turned round -- octant 7 - k, and nothing in front of them."""
    sg = oc.octant_signs(k)
    o = CENTRE - STANDOFF * sg + (rng.uniform(-1, 1, (LANES, 3)) if jitter else rng.uniform(-1, 1, 3))
    o = np.broadcast_to(o, (LANES, 3)).astype(F32).astype(np.float64)
    target = qe.points_on(s, rng.choice(all_prims(s), LANES), rng, "mixed")
    d = target - o
    return make_rays(o, -d if away else d)


def tmax_chunk(s, k, rng):
    r = octant_chunk(s, k, rng)
    r[:, 3] = qe.TMAX_KINDS[rng.integers(0, len(qe.TMAX_KINDS), LANES)]
    rnd = rng.integers(0, 3, LANES) == 0
    r[rnd, 3] = rng.uniform(0.0, 2.0, rnd.sum())
    return r


def ignore_chunk(s, k, rng):
    """query_edges.fam_ignore's chunk: half the lanes start on a triangle and ignore it; k < 0: every lane, in mixed octants."""
    pool = all_prims(s)
    if k < 0:
        p = rng.choice(pool, LANES)
        d = rng.normal(0, 1, (LANES, 3))
        d[:8], d[8:16] = np.abs(d[:8]), -np.abs(d[8:16])
        return make_rays(qe.points_on(s, p, rng, "interior"), d, FLT_MAX, np.where(rng.integers(0, 2, LANES) == 0, p, -1))
    r = octant_chunk(s, k, rng)
    lanes = rng.permutation(LANES)[: LANES // 2]
    p = rng.choice(pool, len(lanes))
    d = oc.octant_signs(k) * rng.uniform(0.2, 1.0, (len(lanes), 3))
    r[lanes] = make_rays(qe.points_on(s, p, rng, "interior"), d, FLT_MAX, p)
    return r


def random_chunks(s, rng, chunks):
    """query_edges.random_rays: rays of every kind the contract names -- axis-parallel, signed zeros, non-finite,
    beyond the packet limits, mixed tmax, ignoring lanes -- in whole chunks"""
    return qe.random_rays(s, rng, LANES * chunks)[:LANES * chunks]


@functools.lru_cache(maxsize=None)
def coherent_base(seed=0):
    """(rays (B_COHERENT, 8), names): 65 chunks of 64 -- named by what they are built to be.  The coherent octant chunks come
    last: the large batch's partial last chunk copies one of them."""
    s = scene()
    rng = np.random.default_rng(seed)
    chunks, names = [], []

    def add(name, r):
        assert r.shape == (LANES, 8)
        chunks.append(r.astype(F32))
        names.append(name)

    rnd = random_chunks(s, rng, 8)
    for i in range(8):
        add("random", rnd[i * LANES:(i + 1) * LANES])
    for i, kind in enumerate(qe.INTRUDERS):
        r = octant_chunk(s, i % 8, rng)
        qe.spoil(r, qe.PACKET_SLOTS[i % len(qe.PACKET_SLOTS)], kind, i % 8, rng, s.n_prims)
        add("intruder_" + kind, r)
    for i in range(4):
        r = octant_chunk(s, 2 * i, rng)       # mixed octants, nothing ignored: any hit takes the sign-generic walk
        r[::2, 4:7] *= -1.0
        add("mixed", r)
    for k in (0, 1, 2, 3, 4, 5, 6, 7, -1, -1, -1, -1):
        add("ignore", ignore_chunk(s, k, rng))
    for k in range(8):
        add("tmax", tmax_chunk(s, k, rng))
    for k in range(8):
        add("miss", octant_chunk(s, k, rng, away=True))
    for k in range(8):
        for jitter in (False, True):
            add("coherent", octant_chunk(s, k, rng, jitter))
    rays = np.concatenate(chunks)
    assert rays.shape == (B_COHERENT, 8)
    return F.frozen(rays), tuple(names)


@functools.lru_cache(maxsize=None)
def query_base(seed=1):
    """(B_PRIME, 8): the coherent base's families in another draw and more random rays, cut to the prime"""
    s = scene()
    rng = np.random.default_rng(seed)
    rays = np.concatenate([coherent_base(seed + 100)[0][8 * LANES:], random_chunks(s, rng, 8)])
    assert len(rays) >= B_PRIME
    return F.frozen(np.ascontiguousarray(rays[:B_PRIME]))


def chunk_of_large(base, n, chunk):
    """the rays of chunk `chunk` (64 rays, fewer for the last) of the batch base.repeat(...)[:n]"""
    i = np.arange(chunk * LANES, min(n, (chunk + 1) * LANES))
    return base[i % len(base)]


@functools.lru_cache(maxsize=None)
def oracle_closest(base):
    """(HIT_DTYPE records, occluded words) of the oracle for a base batch ("prime" or "coherent"), accumulator's epsilon"""
    rays = query_base() if base == "prime" else coherent_base()[0]
    hits, occ = qe.Oracle(scene()).trace(rays, C.PROGRAM_ACCUMULATOR)
    return F.frozen(hits), F.frozen(occ)


same_hits = qe.same_hits     # the records that differ in any bit, but for NaN t (the oracle's tmax passes through a C float)


@functools.lru_cache(maxsize=None)
def oracle_hits8():
    """(B_PRIME, K_HITS) HIT_DTYPE: the peeling oracle's first eight hits of query_base's rays"""
    rays = query_base()
    peeler = mh.Peeler(scene())
    seqs = [peeler.peel(r, C.PROGRAM_ACCUMULATOR, K_HITS) for r in rays]
    return F.frozen(mh.expected_records(seqs, rays, K_HITS))


@functools.lru_cache(maxsize=None)
def oracle_surface():
    """(B_PRIME,) SURFACE_DTYPE: tests/surface.expected over the oracle's closest hits, portable flavour"""
    return F.frozen(S.expected(scene(), oracle_closest("prime")[0], "portable"))


# ------------------------------------------------------------------------------------------------- base batch of the shade families
EXTRA_CAMERA = (0.3, 50.0, 37, 29)    # tests/shade_rays.CAMERAS[1] at SIZES[1]: 1073 rays behind the ring's 3072


@functools.lru_cache(maxsize=None)
def shade_base():
    """(B_PRIME, 8) lt_hip_shade_ray records: shade_rays.ring_batch (twelve cameras round and inside the box, shuffled) and one
    more camera's pixels, cut to the prime"""
    rays = np.concatenate([F.ring_batch()[0], F.camera_batch(*EXTRA_CAMERA)])
    assert len(rays) >= B_PRIME
    return F.frozen(np.ascontiguousarray(rays[:B_PRIME]))


@functools.lru_cache(maxsize=None)
def shade_oracle(call):
    """(B_PRIME, 4) uint32: what po.render leaves in the pixels whose camera rays shade_base holds -- rgb bits of frames 0, 1
    folded (shade_rays: accumulator) or of frame 0 with two bounces (shade_paths: global_illumination) --, and the primitive"""
    yaw, dist, W, H = EXTRA_CAMERA
    if call == "shade_rays":
        rgb = np.concatenate([F.ring_oracle("accumulator", po.MODE_LINEAR, 0, 2),
                              F.oracle_fold(SCENE, yaw, dist, W, H, "accumulator", po.MODE_LINEAR, 0, 2)])
    else:
        rgb = np.concatenate([P.ring_oracle("global_illumination", po.MODE_LINEAR, 0, 1, 2),
                              P.oracle_fold(yaw, dist, W, H, "global_illumination", po.MODE_LINEAR, 0, 1, 2)])
    prim, _ = F.oracle_hits(SCENE, shade_base())
    out = np.empty((B_PRIME, 4), dtype=np.uint32)
    out[:, :3] = np.ascontiguousarray(rgb[:B_PRIME]).view(np.uint32)
    out[:, 3] = prim.view(np.uint32)
    return F.frozen(out)


# ------------------------------------------------------------------------------------------------- the periodic comparison
@dataclass
class Report:
    n: int
    record: int                 # bytes
    modulus: int
    differing: int = 0          # records that are not the base's
    first: int = -1
    last: int = -1
    stale: int = 0              # records with a word that still holds the sentinel
    first_stale: int = -1
    beyond: int = 0             # differing records that start at or beyond `modulus` bytes
    aliased: int = 0            # ... whose offset modulo `modulus` lies in a record that differs too
    head: int = 0               # differing records below `modulus` that such an offset lies in

    @property
    def ok(self):
        return self.differing == 0 and self.stale == 0

    def offset(self, i):
        return i * self.record

    def __str__(self):
        if self.ok:
            return "all %d records of %d bytes are the base batch's" % (self.n, self.record)
        wrap = ("%d of the %d differing records at or beyond byte %d land, modulo %d, on a record that differs too (%d such records below it): "
                "%s" % (self.aliased, self.beyond, self.modulus, self.modulus, self.head,
                        "a wrapped offset" if self.beyond and self.aliased * 2 >= self.beyond else "not the pattern of a wrapped offset"))
        return ("%d of %d records differ from the base batch's: first %d (byte %d), last %d (byte %d); %d still hold the sentinel (first %d, byte %d); %s"
                % (self.differing, self.n, self.first, self.offset(self.first), self.last, self.offset(self.last), self.stale, self.first_stale,
                   self.offset(max(self.first_stale, 0)), wrap))


def check_periodic(out, base, modulus=2 ** 32, sentinel=SENTINEL, piece_bytes=2 ** 29):
    """out: (n, w) int32 tensor (torch, any device; numpy is wrapped), base: (B, w) int32 on the same device.  Record i of `out`
    against record i % B of `base`, bit for bit, in pieces of at most piece_bytes (whole repetitions), so that no temporary
    exceeds a quarter of that.  Returns a Report."""
    import torch
    if isinstance(out, np.ndarray):
        out = torch.from_numpy(np.ascontiguousarray(out).view(np.int32))
    if isinstance(base, np.ndarray):
        base = torch.from_numpy(np.ascontiguousarray(base).view(np.int32))
    assert out.dtype == torch.int32 and base.dtype == torch.int32 and out.device == base.device
    B = base.shape[0]
    base = base.reshape(B, -1)
    w = base.shape[1]
    out = out.reshape(-1, w)
    n = out.shape[0]
    rep = Report(n, 4 * w, modulus)
    reps = max(1, piece_bytes // (4 * w * B))
    bad = torch.zeros(n, dtype=torch.bool, device=out.device)
    stale = torch.zeros(n, dtype=torch.bool, device=out.device)
    for lo in range(0, n, reps * B):
        hi = min(n, lo + reps * B)
        whole = (hi - lo) // B
        if whole:
            piece = out[lo:lo + whole * B].view(whole, B, w)
            bad[lo:lo + whole * B] = (piece != base).any(dim=2).view(-1)
            stale[lo:lo + whole * B] = (piece == sentinel).any(dim=2).view(-1)
        rest = hi - lo - whole * B
        if rest:
            piece = out[hi - rest:hi]
            bad[hi - rest:hi] = (piece != base[:rest]).any(dim=1)
            stale[hi - rest:hi] = (piece == sentinel).any(dim=1)
    rep.differing, rep.stale = int(bad.sum()), int(stale.sum())
    if rep.ok:
        return rep
    if rep.stale:
        rep.first_stale = int(torch.nonzero(stale)[0])
    if rep.differing:
        idx = torch.nonzero(bad).view(-1)
        rep.first, rep.last = int(idx[0]), int(idx[-1])
        far = idx[idx * rep.record >= modulus]
        rep.beyond = int(far.numel())
        if rep.beyond:
            alias = ((far * rep.record) % modulus) // rep.record      # the record a store at the wrapped offset starts in
            hit = bad[alias]
            rep.aliased = int(hit.sum())
            rep.head = int(torch.unique(alias[hit]).numel())
    return rep


def wrapped_store(base, n, record, modulus, sentinel=SENTINEL):
    """What a kernel whose byte offset i * record is taken modulo `modulus` leaves in a sentinel-filled buffer of n records, written
    in the order of i: (n, record / 4) int32.  base: (B, record / 4) int32."""
    buf = np.full(n * record // 4, sentinel, dtype=np.int32)
    raw = buf.view(np.uint8)
    src = np.ascontiguousarray(base).view(np.uint8).reshape(len(base), record)
    for i in range(n):
        at = (i * record) % modulus
        raw[at:at + record] = src[i % len(base)]
    return buf.reshape(n, record // 4)


# ------------------------------------------------------------------------------------------------- renders
def oracle_rows(camera28, W, H, program, y0, y1, depth=3, frame=None, threads=8):
    """Rows [y0, y1) of po.render(scene, camera28, W, H, program, depth=depth): (y1 - y0, W, depth) float32, zeros in the channels
    past 2.  lt_oracle_render writes ((y * W + x) * depth) floats from the pointer it is given and touches rows [y0, y1) alone, so
    it is handed a band's buffer with the pointer moved back by y0 rows: po.render itself would allocate all H rows (25 GB at
    46340 x 46340)."""
    from concurrent.futures import ThreadPoolExecutor
    L = po.lib()
    s = scene()
    arrs = po._scene_arrays(s)
    cam = np.frombuffer(bytes(camera28 if frame is None else sc.camera_with_frame(camera28, frame)), dtype=np.uint8).copy()
    band = np.zeros((y1 - y0, W, depth), dtype=np.float32)
    origin = band.ctypes.data - y0 * W * depth * 4

    def run(y):
        if L.lt_oracle_render(program, po.MODE_LINEAR, *[po._p(a) for a in arrs], po._p(cam), ctypes.c_void_p(origin), W, H, depth, y, y + 1, 16, None):
            raise RuntimeError("oracle: traversal stack overflow")

    with ThreadPoolExecutor(max(1, min(threads, y1 - y0))) as ex:
        list(ex.map(run, range(y0, y1)))
    return band


def row_camera_rays(camera28, W, H, y):
    """(origins, directions) of the pixels of row y: lens_trace_amd.renderer.reference_camera_rays' arithmetic for one row of an
    image too large to hold every pixel's ray (tests/test_large_offsets_cpu.py compares the two on a small image)"""
    cam = np.frombuffer(bytes(camera28), dtype=np.float32, count=7)
    fx = (np.arange(W, dtype=F32) / F32(W) - F32(0.5)).astype(F32)
    fy = np.full(W, F32(y) / F32(H) - F32(0.5), dtype=F32)
    o = np.stack([cam[0] + fx, cam[1] + fy, np.full(W, cam[2] + F32(0.0), dtype=F32)], axis=1).astype(F32)
    dx, dy, dz = F32(0.0) - fx, F32(0.0) - fy, np.full(W, F32(5.0) - F32(0.0), dtype=F32)
    cy, sy = F32(np.cos(np.float64(cam[3]))), F32(np.sin(np.float64(cam[3])))
    d = np.stack([(cy * dx).astype(F32) + (sy * dz).astype(F32), dy, (-sy * dx).astype(F32) + (cy * dz).astype(F32)], axis=1).astype(F32)
    return o, d


def row_hits(camera28, W, H, y):
    """per pixel of row y: does the oracle's closest-hit query of its camera ray hit?"""
    o, d = row_camera_rays(camera28, W, H, y)
    return qe.Oracle(scene()).trace(make_rays(o, d), C.PROGRAM_ACCUMULATOR)[1] != 0


INSIDE = F.camera(0.0, 2.0, 1)    # two units in front of the box's centre, inside it: every pixel's ray ends on a wall


class R1:
    W, H, DEPTH = 16384, 16400, 4
    BYTES = W * H * DEPTH * 4
    PITCH = W * DEPTH * 4
    BAND = 2048                                  # tile_h of the banded render: tile_w = W
    ROWS = (0, 8191, 8192, 8193, 16383, 16384, 16399)
    PROGRAMS = {"basic": po.BASIC, "accumulator": po.ACCUMULATOR}
    CAMERA = INSIDE

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def oracle_row(program, y):
        return F.frozen(oracle_rows(R1.CAMERA, R1.W, R1.H, R1.PROGRAMS[program], y, y + 1, R1.DEPTH)[0])


class R2:
    W, H, DEPTH, FRAMES = 3840, 2160, 3, 44
    FRAME_BYTES = W * H * DEPTH * 4
    SCRATCH = FRAMES * FRAME_BYTES
    ROWS = (0, 1079, 2159)
    CAMERA = F.camera(0.0, 2.0, 0)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def oracle_row(y):
        """row y of the 44 frames folded by po.accumulate from n = 0"""
        acc = np.zeros((1, R2.W, 3), dtype=np.float32)
        for f in range(R2.FRAMES):
            po.accumulate(acc, oracle_rows(R2.CAMERA, R2.W, R2.H, po.ACCUMULATOR, y, y + 1, 3, frame=f, threads=1), f)
        return F.frozen(acc[0])

    @staticmethod
    def oracle_all():
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(3) as ex:
            return dict(zip(R2.ROWS, ex.map(R2.oracle_row, R2.ROWS)))


class R4:
    SIDE = 46340                                 # floor(sqrt(2^31 - 1)): the largest square image plan_tiles takes
    TILE = 8
    TILES_X = -(-SIDE // TILE)
    STRIDE = 2 ** 32 - 1                         # tile_stride of a call for one tile: the largest there is
    PROGRAMS = {"basic": po.BASIC, "accumulator": po.ACCUMULATOR}
    CAMERA = INSIDE

    @staticmethod
    def tiles():
        """(tile index, x0, y0, w, h) of tile 0, the tile that holds pixel (23170, 23170) and the last tile"""
        out = []
        for tx, ty in ((0, 0), (23170 // R4.TILE, 23170 // R4.TILE), (R4.TILES_X - 1, R4.TILES_X - 1)):
            x0, y0 = tx * R4.TILE, ty * R4.TILE
            out.append((ty * R4.TILES_X + tx, x0, y0, min(R4.TILE, R4.SIDE - x0), min(R4.TILE, R4.SIDE - y0)))
        return out

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def oracle_tile(program, tile):
        """(h, w, 3): the tile's block of the oracle's rows [y0, y0 + h)"""
        _, x0, y0, w, h = [t for t in R4.tiles() if t[0] == tile][0]
        rows = oracle_rows(R4.CAMERA, R4.SIDE, R4.SIDE, R4.PROGRAMS[program], y0, y0 + h, 3)
        return F.frozen(np.ascontiguousarray(rows[:, x0:x0 + w]))
