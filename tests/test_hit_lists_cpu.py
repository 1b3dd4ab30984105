"""CPU: what the fixtures of the hit-list tests (tests/hit_lists.py) claim, checked with the peeling oracle alone, and the Python
wrapper's argument checks that need no context.

1. the three batches hold empty segments, segments longer than eight and -- the tie rays -- runs of bit-equal t wider than eight
   in every octant;
2. the stack: its lines cross every sheet once, one primitive per hit, and the rays' tmax give the lengths they are meant to;
3. a ray's sequence under a smaller tmax is the prefix with t < tmax of its sequence under a larger one (the long stack's expected
   sequences rest on it);
4. csr / gather / differ on a hand-made batch;
5. RendererHIP.trace_hits_list refuses what it cannot pass on, before any call into the library."""
import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd.renderer import HIT_DTYPE, RendererHIP, make_rays
from oracle import pyoracle as po
from tests import hit_lists as hl
from tests import multihit as mh
from tests import multihit_edges as me


def test_the_batches_hold_what_the_gpu_tests_need():
    for name in ("sheets", "cornell"):
        n = mh.expected_counts(hl.sequences(name))          # (no ray through the Cornell box has more than eight hits)
        assert (n == 0).sum() >= 64 and (n > 8).sum() >= (64 if name == "sheets" else 0), (name, (n == 0).sum(), (n > 8).sum())
    s, rays = hl.batch("ties")
    seqs = hl.sequences("ties")
    widest = np.array([me.widest_tie(q) for q in seqs])
    octant = hl.octants(rays)
    for o in range(8):
        assert (widest[octant == o] > 8).sum() >= 2, (o, widest[octant == o].max())
    assert (mh.expected_counts(seqs) > 8).sum() >= 256
    # a tie wider than eight lies wholly behind the first eight hits for some rays: only the list shows its order
    assert sum(any(a >= 8 and b - a > 1 for a, b in me.tie_groups(q)) for q in seqs) >= 128


def test_the_stack_has_the_lengths_it_says():
    tile, span = hl.tuning()
    n = hl.stack_sheets()
    assert n == 2 * span + 64 and {0, 1, 2, 63, 64, 65, span - 1, span, span + 1, n} <= set(hl.stack_lengths())
    s = hl.stack_scene()
    assert s.n_prims == n
    rays, seqs, lengths = hl.stack_rays()
    assert len(rays) > 64 and len(rays) == len(seqs) == len(lengths)
    assert [len(q) for q in seqs] == lengths.tolist()
    assert len(set(hl.octants(rays).tolist())) == hl.STACK_LINES
    for q in seqs:
        prims = [h[1] for h in q]
        assert len(set(prims)) == len(prims)                                  # one primitive per hit
    # the peeler itself on the short ones, and on one ray of span + 1 hits
    p = mh.Peeler(s)
    for i in list(np.flatnonzero(lengths <= 129)) + [int(np.flatnonzero(lengths == span + 1)[0])]:
        assert p.peel(rays[i], po.ACCUMULATOR) == seqs[i], i
    # the builder lays the primitives out along z, and half the lines run up the stack and half down it: whichever way a walk meets
    # the sheets, it meets them nearest first for half the rays at most
    z = s.prim_view["positionA"][:, 2]
    assert (np.diff(z) > 0).all() and (rays[:, 6] > 0).sum() == (rays[:, 6] < 0).sum() == len(rays) // 2


@pytest.mark.parametrize("prog", (po.BASIC, po.ACCUMULATOR))
def test_a_smaller_tmax_gives_a_prefix(prog):
    n = 40
    s = hl.scene_of_triangles(hl.stack_triangles(n), 3)
    lengths = (0, 1, 2, 7, 8, 9, 20, n - 1, n)
    rays, whole = hl.rays_of_lengths(s, n, lengths, prog)
    p = mh.Peeler(s)
    for r, want in zip(rays, hl.prefix_sequences(rays, whole)):
        assert p.peel(r, prog) == want
    # ... and on the sheets, ties included: the rays whose tmax lies between two of their own hits
    sheets, (all_rays, cats) = mh.sheets_scene(), mh.sheet_rays()
    p = mh.Peeler(sheets)
    for r in all_rays[cats == "tmax_between"][:24]:
        far = r.copy()
        far[3] = np.inf
        assert p.peel(r, prog) == [h for h in p.peel(far, prog) if h[0] < r[3]]


def test_csr_gather_and_differ():
    seqs = [[(0.5, 3, 0.25, 0.5)], [], [(-0.0, 1, 0.0, 1.0), (0.0, 2, 1.0, 0.0)]]
    offsets, items = hl.csr(seqs)
    assert offsets.dtype == np.uint64 and offsets.tolist() == [0, 1, 1, 3] and items.dtype == HIT_DTYPE and items["prim"].tolist() == [3, 1, 2]
    assert hl.differ((offsets, items), (offsets, items)) is None
    assert [len(g) for g in hl.segments((offsets, items))] == [1, 0, 2]
    go, gi = hl.gather((offsets, items), [2, 0])
    assert go.tolist() == [0, 2, 3] and gi["prim"].tolist() == [1, 2, 3]
    other = items.copy()
    other["t"][1] = 0.0                                                        # +0 for -0: equal as floats, other bits
    assert "record 1 (ray 2, hit 0)" in hl.differ((offsets, other), (offsets, items))
    assert "offsets[3]" in hl.differ((offsets + np.uint64([0, 0, 0, 1]), items), (offsets, items))
    assert hl.octants(make_rays([[0, 0, 0]] * 2, [[1, -1, 0.0], [-0.0, 2, -3]])).tolist() == [2, 5]


def test_the_wrapper_checks_its_arguments_without_a_context():
    assert C.TRACE_LIST_FLAG_FILL_ONLY & (C.RENDER_FLAG_STRICT_MATH | C.RENDER_FLAG_PORTABLE_MATH | C.TRACE_FLAG_COHERENT) == 0
    import ctypes
    assert ctypes.sizeof(C.HitsListDesc) == 16
    r = object.__new__(RendererHIP)                                            # no context: nothing may reach the library

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the wrapper called %s" % name)

    r._L, r._ctx, r.device = NoLibrary(), None, 0
    with pytest.raises(ValueError):
        r.trace_hits_list(np.zeros((4, 6), dtype=np.float32))
    with pytest.raises(ValueError):
        r.trace_hits_list(np.zeros((4, 8), dtype=np.float64))
    with pytest.raises(ValueError):
        r.trace_hits_list(np.zeros(4, dtype=HIT_DTYPE))
    with pytest.raises(TypeError):
        r.trace_hits_list([[0.0] * 8])
