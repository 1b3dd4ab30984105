"""CPU: what tests/large_offsets.py claims (the fixtures of tests/test_gpu_large_offsets.py).

* every ray case crosses the power of two its table entry names, computed from n and the record sizes of lens_trace_amd/_capi.py;
  no period of a base batch divides 2^32 bytes, so a wrapped store never meets its own repetition;
* the base batches hold hits, misses, ignoring lanes, mixed tmax and coherent chunks of every octant; a coherent chunk keeps its
  verdict wherever the large batch repeats it, and the large batch's last chunk is partial;
* the oracle rows and tiles of the renders lie on both sides of bytes 2^31 and 2^32, and at least half of each row's pixels hit;
* check_periodic finds a store whose offset wrapped (the unwritten tail, the overwritten head, the first record) and a last chunk
  that was written in part."""
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import reference_camera_rays
from tests import large_offsets as LO
from tests import query_edges as qe
from tests import shade_rays as F

# name: (n, bytes in, bytes out): the issue's table, in figures
TABLE = {
    "closest": (2 ** 27 + 2 ** 20 + 37, 4_328_522_912, 2_164_261_456),
    "closest_coherent": (2 ** 27 + 2 ** 20 + 37, 4_328_522_912, 2_164_261_456),
    "any_coherent": (2 ** 27 + 2 ** 20 + 37, 4_328_522_912, 541_065_364),
    "hits8": (2 ** 25 + 2 ** 12 + 5, 1_073_873_056, 4_295_492_224),
    "surface": (90_000_037, 2_880_001_184, 4_320_001_776),
    "surface_at": (90_000_037, 1_440_000_592, 4_320_001_776),
    "shade_rays": (2 ** 27 + 2 ** 20 + 37, 4_328_522_912, 2_164_261_456),
    "shade_paths": (2 ** 27 + 2 ** 20 + 37, 4_328_522_912, 2_164_261_456),
}


# --------------------------------------------------------------------------------------------------------------- 1: the table
def test_record_sizes_are_the_bindings():
    assert (LO.RAY, LO.HIT, LO.SURFACE, LO.SHADE_RAY, LO.SHADE) == (32, 16, 48, 32, 16)
    assert LO.RAY == C.RAY_DTYPE.itemsize and LO.HIT == C.HIT_DTYPE.itemsize and LO.SURFACE == C.SURFACE_DTYPE.itemsize
    assert LO.SHADE_RAY == C.SHADE_RAY_DTYPE.itemsize and LO.SHADE == C.SHADE_DTYPE.itemsize


@pytest.mark.parametrize("name", sorted(LO.CASES))
def test_every_case_crosses_what_it_says(name):
    case = LO.CASES[name]
    assert set(LO.CASES) == set(TABLE)
    assert (case.n, case.in_bytes, case.out_bytes) == TABLE[name]
    for nbytes, record, crosses in ((case.in_bytes, case.in_record, case.in_crosses), (case.out_bytes, case.out_record, case.out_crosses)):
        if crosses:
            assert nbytes > crosses and -(-crosses // record) < case.n       # a whole record starts at or beyond the crossing
            assert nbytes - crosses >= 64 * record                        # ... and more than a chunk of them
        # a store whose offset wrapped modulo 2^32 lands on another phase of the period: it cannot write the bits that belong there
        assert 2 ** 32 % (case.period * record) != 0
    assert case.in_crosses or case.out_crosses
    assert max(case.in_bytes, case.out_bytes) > 2 ** 32
    assert LO.device_bytes(case) < LO.DEVICE_LIMIT
    if case.base == "coherent":
        assert case.period % 64 == 0 and case.n % 64 != 0                # whole chunks repeated; the last chunk partial
    else:
        assert case.period == 4099 and all(4099 % p for p in range(2, 65))   # prime: every alignment to the 64-lane chunks occurs


def test_every_case_states_the_device_memory_it_holds():
    """records in and out, the library's own allocations for the call and the comparison: below 16 GiB for every case"""
    GB = 10 ** 9
    slots_default = min(64 * 2 ** 20, 16 * 2 ** 30 // LO.GI_SLOT_BYTES)                  # enqueue_paths: kPathsSlots, LT_FUSED_BYTES / 272
    paths = LO.CASES["shade_paths"]
    sets, per_set = LO.paths_sets(paths.n, slots=slots_default)
    assert (sets, per_set) == (3, 45_088_781)
    assert paths.in_bytes + paths.out_bytes + per_set * (LO.GI_SLOT_BYTES + 16) > LO.DEVICE_LIMIT   # the default: 19.5 GB, too much
    sets, per_set = LO.paths_sets(paths.n)
    assert (sets, per_set) == (9, 15_029_594) and per_set <= LO.PATHS_SLOTS and sets * per_set >= paths.n
    assert LO.scratch_bytes(paths) == per_set * 288 and 4.3 * GB < LO.scratch_bytes(paths) < 4.4 * GB
    assert (sets - 1) * per_set < 2 ** 27 < paths.n and 2 ** 27 * LO.SHADE_RAY == 2 ** 32   # the last set's p.ray0 + r passes byte 2^32 of the rays
    assert LO.scratch_bytes(LO.CASES["surface"]) == 1_440_000_592                         # lt_hip_trace_surface's hits
    assert all(LO.scratch_bytes(c) == 0 for n, c in LO.CASES.items() if n not in ("surface", "shade_paths"))
    want = {"closest": 7.6, "closest_coherent": 7.6, "any_coherent": 5.9, "hits8": 6.4, "surface": 9.7, "surface_at": 6.8, "shade_rays": 7.6, "shade_paths": 11.9}
    for name, case in LO.CASES.items():
        assert abs(LO.device_bytes(case) / GB - want[name]) < 0.06, (name, LO.device_bytes(case))
    assert LO.COMPARE_BYTES >= 2 * LO.N_RAYS + 3 * 2 ** 29 // 4 + 2 ** 20
    assert LO.HOST_FORM_BYTES == LO.CASES["closest"].in_bytes + LO.CASES["closest"].out_bytes
    R = LO.R1
    assert LO.R1_BYTES == 2 * R.BYTES + 9 * R.W * R.BAND * 16 + 2 ** 29 and LO.R3_BYTES == 2 * R.BYTES + 2 ** 30
    assert LO.R2_BYTES > LO.R2.SCRATCH + 4 * LO.R2.FRAME_BYTES + (LO.R2.W // 8) * (LO.R2.H // 8) * 64 * 16
    for nbytes in (LO.HOST_FORM_BYTES, LO.R1_BYTES, LO.R2_BYTES, LO.R3_BYTES):
        assert nbytes < LO.DEVICE_LIMIT


def test_the_ray_that_crosses_is_the_one_the_table_names():
    c = LO.CASES["closest"]
    assert 2 ** 27 * c.in_record == 2 ** 32 and 2 ** 27 * c.out_record == 2 ** 31 and 2 ** 27 < c.n
    assert 2 ** 25 * LO.CASES["hits8"].out_record == 2 ** 32 and 2 ** 25 < LO.CASES["hits8"].n
    assert 2 ** 26 * LO.RAY == 2 ** 31 and 2 ** 26 < LO.N_SURFACE and 2 ** 32 // LO.SURFACE < LO.N_SURFACE


# --------------------------------------------------------------------------------------------------------------- 2: the base batches
def test_the_coherent_base_holds_every_family_and_verdict():
    rays, names = LO.coherent_base()
    assert rays.shape == (LO.B_COHERENT, 8) and len(names) == 65
    closest, any_hit = qe.chunk_verdicts(rays, False), qe.chunk_verdicts(rays, True)
    assert set(closest) == {None, 0, 1, 2, 3, 4, 5, 6, 7} and set(any_hit) == {None, -1, 0, 1, 2, 3, 4, 5, 6, 7}
    for i, name in enumerate(names):
        chunk = rays[i * 64:(i + 1) * 64]
        if name in ("coherent", "tmax", "miss"):
            assert closest[i] is not None and closest[i] == any_hit[i], (i, name)
        if name == "ignore":
            assert closest[i] is None and any_hit[i] is not None and qe.ignores(chunk).any(), i
        if name == "mixed":
            assert closest[i] is None and any_hit[i] == -1, i
        if name == "tmax":
            assert len(np.unique(chunk[:, 3].view(np.uint32))) >= 6, i
    hits, occ = LO.oracle_closest("coherent")
    hit = (hits["prim"] >= 0).reshape(65, 64)
    # (coherent: a ray aimed at a vertex or an edge may slip past it)
    for name, lo, hi in (("coherent", 0.9, 1.0), ("miss", 0.0, 0.0), ("tmax", 0.1, 0.9), ("ignore", 0.5, 1.0)):
        share = hit[[i for i, n in enumerate(names) if n == name]].mean()
        assert lo <= share <= hi, (name, share)
    assert np.array_equal(occ, (hits["prim"] >= 0).astype(np.uint32))
    assert len({n for n in names if n.startswith("intruder_")}) == len(qe.INTRUDERS)


def test_the_prime_base_holds_every_family():
    rays = LO.query_base()
    assert rays.shape == (LO.B_PRIME, 8)
    hits, _ = LO.oracle_closest("prime")
    assert 0.3 < (hits["prim"] >= 0).mean() < 0.9
    assert qe.ignores(rays).sum() > 300 and (~np.isfinite(rays[:, :7])).any(axis=1).sum() > 20
    assert len(np.unique(rays[:, 3].view(np.uint32))) > 100 and {0x7f7fffff, 0x7f800000, 0, 0x80000000, 0x7fc00000} <= set(rays[:, 3].view(np.uint32).tolist())
    assert set(qe.chunk_verdicts(rays[:57 * 64], False)) >= set(range(8))
    # the multi-hit case has rays with no, one and several hits, and lists that are full
    per_ray = (LO.oracle_hits8()["prim"] >= 0).sum(axis=1)
    assert (per_ray == 0).sum() > 500 and (per_ray == 1).sum() > 200 and (per_ray >= 3).sum() > 200
    surf = LO.oracle_surface()
    assert (surf["flags"] == C.SURFACE_LIGHT).any() and (surf["material"] >= 0).sum() == (hits["prim"] >= 0).sum()


def test_coherent_chunks_keep_their_verdicts_in_the_large_batch():
    rays, names = LO.coherent_base()
    n = LO.CASES["closest_coherent"].n
    chunks = -(-n // 64)
    assert chunks == 2 ** 21 + 2 ** 14 + 1 and n - 64 * (chunks - 1) == 37
    for any_hit in (False, True):
        base = qe.chunk_verdicts(rays, any_hit)
        picks = [0, 1, 64, 65, 66, chunks // 2, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, chunks - 2, chunks - 1]
        picks += list(range(chunks // 2 - 65, chunks // 2))                  # every base chunk once, mid-batch
        for c in picks:
            got = qe.verdict(LO.chunk_of_large(rays, n, c), any_hit)
            assert got == base[c % 65], (c, got, base[c % 65])
    # the partial last chunk copies a coherent octant chunk: its 37 rays walk as a packet, as the whole chunk does
    assert names[(chunks - 1) % 65] == "coherent" and len(LO.chunk_of_large(rays, n, chunks - 1)) == 37


def test_the_shade_base_is_cameras_round_and_inside_the_box():
    rays = LO.shade_base()
    assert rays.shape == (LO.B_PRIME, 8)
    for call in ("shade_rays", "shade_paths"):
        want = LO.shade_oracle(call)
        prim = want[:, 3].view(np.int32)
        assert 0.3 < (prim >= 0).mean() < 0.95
        rgb = want[:, :3].view(np.float32)
        assert np.isfinite(rgb).all() and len(np.unique(want[:, :3], axis=0)) > 500 and (want != LO.SENTINEL).all()
    d = rays[:, 4:7]
    assert len(set(((d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4).tolist())) == 8


# --------------------------------------------------------------------------------------------------------------- 3: the renders
def test_row_camera_rays_are_reference_camera_rays():
    for cam in (F.camera(0.3, 50.0), F.camera(-2.4, 2.0), LO.INSIDE):
        o, d, _, _ = reference_camera_rays(cam, 37, 29)
        for y in (0, 11, 28):
            ro, rd = LO.row_camera_rays(cam, 37, 29, y)
            assert np.array_equal(o[y * 37:(y + 1) * 37].view(np.uint32), ro.view(np.uint32))
            assert np.array_equal(d[y * 37:(y + 1) * 37].view(np.uint32), rd.view(np.uint32))


def test_oracle_rows_are_po_renders():
    from oracle import pyoracle as po
    cam = F.camera(0.3, 50.0, 2)
    want = po.render(LO.scene(), cam, 37, 29, po.ACCUMULATOR, depth=4)
    got = LO.oracle_rows(cam, 37, 29, po.ACCUMULATOR, 11, 14, depth=4)
    assert np.array_equal(got.view(np.uint32), want[11:14].view(np.uint32))
    assert np.array_equal(LO.oracle_rows(F.camera(0.3, 50.0, 0), 37, 29, po.ACCUMULATOR, 11, 14, depth=4, frame=2), got)


def test_r1_rows_lie_on_both_sides_of_the_crossings():
    R = LO.R1
    assert R.BYTES == 4_299_161_600 > 2 ** 32 and R.PITCH == 2 ** 18
    assert 8192 * R.PITCH == 2 ** 31 and 16384 * R.PITCH == 2 ** 32
    assert {8191, 8192, 8193, 16383, 16384, 0, R.H - 1} == set(R.ROWS)
    assert R.W * R.H <= 2 ** 31 - 1 and R.W * R.BAND * R.DEPTH * 4 == 512 * 2 ** 20 and R.H % R.BAND != 0    # the last band is clipped
    for y in R.ROWS:
        hit = LO.row_hits(R.CAMERA, R.W, R.H, y)
        assert 2 * hit.sum() >= R.W, y
        for program in R.PROGRAMS:
            row = R.oracle_row(program, y)
            # (basic stores the hit material's colour: a few flat runs per row; accumulator's noise makes every row its own)
            assert row.shape == (R.W, 4) and (row[:, 3] == 0).all() and len(np.unique(row[:, :3], axis=0)) > (100 if program == "accumulator" else 1), (program, y)
    rows = np.stack([R.oracle_row("accumulator", y)[:, :3] for y in R.ROWS])
    assert all((rows[i] != rows[j]).any(axis=1).mean() > 0.5 for i in range(len(rows)) for j in range(i))   # no two checked rows alike


def test_r2_frames_lie_on_both_sides_of_the_crossings():
    R = LO.R2
    assert R.FRAME_BYTES == 99_532_800 and R.SCRATCH == 4_379_443_200
    assert 21 * R.FRAME_BYTES < 2 ** 31 < 22 * R.FRAME_BYTES and 43 * R.FRAME_BYTES < 2 ** 32 < 44 * R.FRAME_BYTES
    assert R.SCRATCH < 16 * 2 ** 30                       # under plan_fusion's default cap: one fused launch
    assert 7 * R.W * R.H * 16 < 2 ** 30 <= 16 * 2 ** 30 // (R.W * R.H * 284) * R.W * R.H * 284 // 7   # (the docstring's word on the GI arrays)
    for y in R.ROWS:
        assert 2 * LO.row_hits(R.CAMERA, R.W, R.H, y).sum() >= R.W, y
        row = R.oracle_row(y)
        assert row.shape == (R.W, 3) and len(np.unique(row, axis=0)) > 100, y


def test_r4_is_the_top_of_the_accepted_range():
    R = LO.R4
    assert R.SIDE ** 2 == 2_147_395_600 <= 2 ** 31 - 1 < (R.SIDE + 1) ** 2
    tiles = R.tiles()
    assert R.TILES_X == 5793 and R.TILES_X ** 2 < 2 ** 26
    assert tiles[0][:3] == (0, 0, 0)
    _, x0, y0, w, h = tiles[1]
    assert x0 <= 23170 < x0 + w and y0 <= 23170 < y0 + h
    last, x0, y0, w, h = tiles[2]
    assert last == R.TILES_X ** 2 - 1 and (x0 + w, y0 + h) == (R.SIDE, R.SIDE) and (w, h) == (4, 4)
    assert (y0 * R.SIDE + x0) * 3 * 4 > 2 ** 32                  # (its first float in a whole image: far beyond 4 GiB)
    t = R.oracle_tile("basic", tiles[1][0])
    assert t.shape == (8, 8, 3) and np.isfinite(t).all()


# --------------------------------------------------------------------------------------------------------------- 4: the checker
def some_base(B, words, seed=0):
    return np.random.default_rng(seed).integers(0, 2 ** 30, (B, words)).astype(np.int32)


def test_the_checker_passes_a_periodic_buffer():
    base = some_base(13, 4)
    out = np.resize(base, (100, 4))
    rep = LO.check_periodic(out, base, piece_bytes=512)        # (pieces of two repetitions, and a rest)
    assert rep.ok and rep.differing == 0 and rep.stale == 0 and "all 100 records" in str(rep)


@pytest.mark.parametrize("words,n,modulus", [(4, 100, 1024), (1, 300, 1024), (12, 60, 1024), (32, 23, 2048)])
def test_the_checker_catches_a_wrapped_offset(words, n, modulus):
    """A store at (i * record) mod M: the records from byte M on keep the sentinel, and the first records hold a later repetition's
    bits."""
    record = 4 * words
    base = some_base(13, words)
    out = LO.wrapped_store(base, n, record, modulus)
    first_beyond = -(-modulus // record)
    assert first_beyond < n
    for piece in (2 ** 29, 4 * record * 13):
        rep = LO.check_periodic(out, base, modulus=modulus, piece_bytes=piece)
        assert not rep.ok
        assert rep.stale == n - first_beyond and rep.first_stale == first_beyond          # the unwritten tail
        assert rep.first == 0 and rep.last == n - 1                                        # the overwritten head, from the first record
        assert rep.beyond == n - first_beyond and rep.aliased == rep.beyond                # every tail record pairs up with a wrong head record
        assert rep.head >= (n - first_beyond) * record // (record + 4 * words) and rep.head <= rep.differing - rep.beyond
        assert rep.differing == rep.beyond + int((out[:first_beyond] != np.resize(base, (n, words))[:first_beyond]).any(axis=1).sum())
        text = str(rep)
        assert "first 0 (byte 0)" in text and "last %d (byte %d)" % (n - 1, (n - 1) * record) in text and "a wrapped offset" in text
        assert "not the pattern" not in text


def test_the_checker_catches_a_last_chunk_written_in_part():
    base = some_base(13, 4)
    n = 64 * 5 + 37
    out = np.resize(base, (n, 4)).copy()
    out[n - 20:] = LO.SENTINEL                     # 17 of the last chunk's 37 records written
    rep = LO.check_periodic(out, base)
    assert not rep.ok and rep.differing == 20 and rep.stale == 20 and rep.first == rep.first_stale == n - 20 and rep.last == n - 1
    assert rep.beyond == 0 and rep.aliased == 0 and "not the pattern of a wrapped offset" in str(rep)
    assert "first %d (byte %d)" % (n - 20, (n - 20) * 16) in str(rep)


def test_the_checker_catches_one_wrong_word_and_one_stale_word():
    base = some_base(4099 % 97, 12)
    out = np.resize(base, (500, 12)).copy()
    out[123, 7] ^= 1
    out[321, 11] = LO.SENTINEL
    rep = LO.check_periodic(out, base, piece_bytes=4096)
    assert (rep.differing, rep.first, rep.last, rep.stale, rep.first_stale) == (2, 123, 321, 1, 321)


def test_the_sentinel_is_no_result():
    assert np.isnan(np.uint32(LO.SENTINEL).view(np.float32)) and LO.SENTINEL != 0x7fc00000
    for a in (LO.query_base(), LO.coherent_base()[0], LO.shade_base(), LO.oracle_closest("prime")[0], LO.oracle_closest("coherent")[0],
              LO.oracle_hits8(), LO.oracle_surface()):
        assert not (np.ascontiguousarray(a).view(np.uint32) == LO.SENTINEL).any()
    assert ctypes.sizeof(ctypes.c_int32) == 4
