"""The records lt_hip_set_scene derives from the own tree and the primitives, once more in plain numpy (no GPU, no library call):
what lt_own16.hpp, lt_retile_kernel, lt_own_pair_kernel, lt_wide_kernel and lt_wide_leaf_kernel compute, float32 where they use
float and float64 where they use double, every sum and product rounded on its own (the library is built without contraction).
tests/test_structures_cpu.py holds it against the host-only lt_hip_own_wide, tests/test_gpu_scene_history.py holds what
lt_hip_read_scene_structure reads back against it, byte for byte.

own_nodes: the own tree as a NODE_DTYPE array (kind 0); prims: a PRIM_DTYPE array."""
import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32
NONE = 0xffffffff
LEAF = 0x80000000


def _bits(f):
    return np.ascontiguousarray(f, dtype=F32).view(U32)


def _floats(u):
    return np.ascontiguousarray(u, dtype=U32).view(F32)


def outwards(b, up):
    """lt_own16::outwards: the bound moved by 2^-21 of its magnitude and one float more, away from the box (up: towards +inf).
    +-0 (also what a denormal's 2^-21 rounds to) becomes the smallest denormal of that side."""
    b = np.asarray(b, dtype=F32)
    up = np.broadcast_to(np.asarray(up, dtype=bool), b.shape)
    with np.errstate(all="ignore"):
        d = np.abs(b) * F32(2.0 ** -21)
        t = np.where(up, b + d, b - d).astype(F32)
    u = _bits(t).astype(np.int64)
    zero = (u & 0x7fffffff) == 0
    away = (t > 0) == up                      # away from zero: the next larger magnitude, one more in the bit pattern
    stepped = np.where(away, u + 1, u - 1)
    tiny = np.where(up, 0x00000001, 0x80000001)
    return _floats(np.where(zero, tiny, stepped).astype(U32)).reshape(b.shape)


def frame(lo, hi):
    """lt_own16::frame for the three axes of the root box: (origin, step), float32 each."""
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    l = outwards(outwards(lo, False), False)
    h = outwards(outwards(hi, True), True)
    step = (h.astype(F64) - l.astype(F64)) / F64(65528.0)
    floor_step = np.maximum(np.abs(l.astype(F64)), np.abs(h.astype(F64))) * F64(2.0 ** -28) + F64(2.0 ** -120)
    step = np.where(step > floor_step, step, floor_step)
    s = step.astype(F32)
    s = np.where(s.astype(F64) < step, _floats(_bits(s) + U32(1)), s)   # the step rounded up
    return l, s.astype(F32)


def quantise(lo, hi, O, S):
    """lt_own16::quantise along one or more axes (arrays broadcast): (ql, qh, ok)."""
    O, S = np.asarray(O, dtype=F32).astype(F64), np.asarray(S, dtype=F32).astype(F64)
    tl, th = outwards(lo, False).astype(F64), outwards(hi, True).astype(F64)
    O, S, tl, th = np.broadcast_arrays(O, S, tl, th)
    q = np.clip(np.floor((tl - O) / S), -2.0, 65537.0)
    while True:
        more = (O + q * S > tl) & (q >= 0.0)
        if not more.any():
            break
        q = np.where(more, q - 1.0, q)
    ok = (q >= 0.0) & (q <= 65535.0)
    ql = np.clip(q, 0.0, 65535.0).astype(U32)
    q = np.clip(np.ceil((th - O) / S), -2.0, 65537.0)
    while True:
        more = (O + q * S < th) & (q <= 65535.0)
        if not more.any():
            break
        q = np.where(more, q + 1.0, q)
    ok &= (q >= 0.0) & (q <= 65535.0)
    qh = np.clip(q, 0.0, 65535.0).astype(U32)
    return ql, qh, ok


def slot_record(lo, hi, link, O, S):
    """lt_own16::slot_record for m nodes (lo, hi: (m, 3)): ((m, 4) uint32 words, ok per node)."""
    ql, qh, ok = quantise(np.asarray(lo, dtype=F32).reshape(-1, 3), np.asarray(hi, dtype=F32).reshape(-1, 3), O, S)
    r = np.empty((len(ql), 4), dtype=U32)
    r[:, 0] = ql[:, 0] | (ql[:, 1] << U32(16))
    r[:, 1] = ql[:, 2] | (qh[:, 0] << U32(16))
    r[:, 2] = qh[:, 1] | (qh[:, 2] << U32(16))
    r[:, 3] = np.asarray(link, dtype=U32)
    return r, ok.all(axis=1)


def empty_slot(groups, n_prims):
    return np.array([0xffffffff, 0x0000ffff, 0, LEAF | (groups + n_prims)], dtype=U32)


def _tri9(prims):
    """A, B - A, C - A: the nine floats lt_retile_kernel, lt_own_pair_kernel and lt_wide_leaf_kernel put in front."""
    a, b, c = (np.asarray(prims[k], dtype=F32) for k in ("positionA", "positionB", "positionC"))
    with np.errstate(all="ignore"):
        return np.concatenate([a, b - a, c - a], axis=1).astype(F32)


def retile(prims):
    """Kind 5: the 48-byte traversal triangles, (n, 12) float32."""
    out = np.zeros((len(prims), 12), dtype=F32)
    out[:, :9] = _tri9(prims)
    return out


def _leaf_records(own_nodes, prims):
    """The 16 words both walks keep per leaf: the triangle, the leaf's box bit for bit, the primitive offset."""
    off = own_nodes["offset"].astype(np.int64)
    r = np.empty((len(own_nodes), 16), dtype=U32)
    r[:, :9] = _tri9(prims[off]).view(U32)
    r[:, 9:12] = own_nodes["boundsMin"].view(U32)
    r[:, 12:15] = own_nodes["boundsMax"].view(U32)
    r[:, 15] = own_nodes["offset"].view(U32)
    return r


def pair_records(own_nodes, prims):
    """Kind 4: the packet walks' 64-byte records, one per node of the own tree, (n, 16) uint32."""
    n = len(own_nodes)
    leaf = own_nodes["primitiveCount"] != 0
    out = np.zeros((n, 16), dtype=U32)
    if leaf.any():
        out[leaf] = _leaf_records(own_nodes[leaf], prims)
    inner = np.flatnonzero(~leaf)
    for k, child in enumerate((inner + 1, own_nodes["offset"][inner].astype(np.int64))):
        c = own_nodes[child]
        w = out[inner, 8 * k: 8 * k + 8]
        w[:, 0:3] = outwards(c["boundsMin"], False).view(U32)
        w[:, 3:6] = outwards(c["boundsMax"], True).view(U32)
        w[:, 6] = child.astype(U32) | np.where(c["primitiveCount"] != 0, U32(LEAF), U32(0))
        w[:, 7] = 0                                                       # 0.0f
        out[inner, 8 * k: 8 * k + 8] = w
    return out


def _half_area(own_nodes):
    d = (own_nodes["boundsMax"] - own_nodes["boundsMin"]).astype(F32)
    with np.errstate(all="ignore"):
        return ((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]).astype(F32) + d[:, 2] * d[:, 0]).astype(F32)


def collapse(own_nodes):
    """lt_retree::collapse_wide: (children (groups, 4), groupOf (n,)) -- a group stands for an interior node and holds its two
    children, the one with the largest box replaced by its own two, and once more; interior children first, leaves last; groups
    numbered in the order of their nodes."""
    n = len(own_nodes)
    off = own_nodes["offset"].astype(np.int64)
    is_leaf = own_nodes["primitiveCount"] != 0
    area = _half_area(own_nodes)

    def kids_of(b):
        kids = [b + 1, int(off[b])]
        while len(kids) < 4:
            best, best_area = -1, F32(-1.0)
            for k, c in enumerate(kids):
                if not is_leaf[c] and area[c] > best_area:
                    best, best_area = k, area[c]
            if best < 0:
                break
            d = kids[best]
            kids[best] = d + 1
            kids.append(int(off[d]))
        return [c for c in kids if not is_leaf[c]] + [c for c in kids if is_leaf[c]]

    heads, todo, kids = [], [0], {}
    while todo:
        b = todo.pop()
        heads.append(b)
        kids[b] = kids_of(b)
        todo.extend(c for c in kids[b] if not is_leaf[c])
    heads.sort()
    groupOf = np.full(n, NONE, dtype=U32)
    groupOf[heads] = np.arange(len(heads), dtype=U32)
    children = np.full((len(heads), 4), NONE, dtype=U32)
    for g, b in enumerate(heads):
        children[g, :len(kids[b])] = kids[b]
    return children, groupOf


def unlinked(own_nodes, n_prims):
    """The primitive offsets no leaf of the own tree names: nobody writes their leaf records in kind 2."""
    named = np.zeros(n_prims, dtype=bool)
    named[own_nodes["offset"][own_nodes["primitiveCount"] != 0]] = True
    return np.flatnonzero(~named)


def wide_records(own_nodes, children, groupOf, prims, n_prims):
    """Kind 2: the 64-byte head (the grid), the groups' slots, the leaf records by primitive offset, the sentinel behind the last
    primitive's: (1 + groups + n_prims + 1, 16) uint32.  The leaf records of `unlinked` offsets are left zero here.
    Also returns whether every bound stayed on the grid."""
    children = np.asarray(children, dtype=U32).reshape(-1, 4)
    groups = len(children)
    O, S = frame(own_nodes["boundsMin"][0], own_nodes["boundsMax"][0])
    out = np.zeros((1 + groups + n_prims + 1, 16), dtype=U32)
    out[0, 8:11], out[0, 12:15] = O.view(U32), S.view(U32)
    slots = np.tile(empty_slot(groups, n_prims), (4 * groups, 1))
    flat = children.reshape(-1)
    used = np.flatnonzero(flat != NONE)
    c = own_nodes[flat[used]]
    link = np.where(c["primitiveCount"] != 0, U32(LEAF) | (U32(groups) + c["offset"].view(U32)), np.asarray(groupOf, dtype=U32)[flat[used]])
    slots[used], ok = slot_record(c["boundsMin"], c["boundsMax"], link, O, S)
    out[1: 1 + groups] = slots.reshape(groups, 16)
    leaves = own_nodes[own_nodes["primitiveCount"] != 0]
    out[1 + groups + leaves["offset"].astype(np.int64)] = _leaf_records(leaves, prims)
    nan = 0x7fc00000
    out[1 + groups + n_prims] = [0] * 9 + [nan] * 6 + [n_prims]
    return out, bool(ok.all())


def wide_mask(own_nodes, groups, n_prims):
    """Rows of kind 2 (64-byte records, the head included) that a comparison covers: all but the leaf records of `unlinked`."""
    keep = np.ones(1 + groups + n_prims + 1, dtype=bool)
    keep[1 + groups + unlinked(own_nodes, n_prims)] = False
    return keep
