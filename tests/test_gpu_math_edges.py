"""GPU tests (-m gpu) that pin lt_device.hpp's leaf layer -- Math<0/1/2>::{mad, rcp, fdiv, div25, sqrt_user, rsqrt,
sqrt_in_distance, sin, cos, clamp01}, normalize4, distance4, dot4, dot2, cross4, bary3's contraction shape -- at the edges of its
domain (tests/math_edges.py: every exponent, denormals, FLT_MIN's neighbours, zeros, infinities, NaN, squared lengths below
FLT_MIN and overflowing, cancelling differences, operands that separate fused from unfused), where rendered images never go.

Ground truth per flavour:
* as shipped (default)  -- oracle/math_probe.cl compiled as the reference's kernels are built (math_probe.default.co): the real
  OpenCL compiler and device library, run on the same GPU (oracle/ref_gpu.py:probe);
* strict (LT_RENDER_FLAG_STRICT_MATH) -- the same file built with -ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt;
* portable (LT_RENDER_FLAG_PORTABLE_MATH) -- the CPU oracle's leaf functions (lt_oracle_leaf), themselves held against a
  high-precision reference by tests/test_math_edges_cpu.py.
The probe user program tests/user_kernels/math_probe.hip evaluates the lt:: function of one record per pixel and compares bit
patterns on the device (NaN equals NaN); inputs and expectations ride in the primitives' normals of an ordinary scene.

Left out, by name:
* clamp01 / "NaN through clamp" (every flavour): OpenCL leaves clamp of NaN undefined, the compiler lowers it differently from
  context to context (v_med3_f32 in the render kernels, v_max_f32 with the clamp modifier in the probe), and C's fmin / fmax differ
  between quiet and signalling NaNs from library to library.  0.5 % of clamp01's inputs.
* portable sin / cos may disagree with the oracle on the share DESIGN section 4 states for two <= 1-ulp double implementations
  after the float rounding (1e-10), times 4, plus one value -- never on 0, +-inf or NaN."""
import os

import numpy as np
import pytest

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import KERNEL_MODE_TILE, RendererHIP, RenderPropertiesHIP
from oracle import pyoracle as po
from oracle import ref_gpu
from tests import math_edges as me

pytestmark = pytest.mark.gpu
PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "user_kernels", "math_probe.hip")
W = H = 256
VALUES = {op: (1 if op == "mad1d" else m) for op, (_, _, m) in me.OPS.items()}   # values compared per record (a double is one)
DOUBLE_SINE_SHARE = 1e-10


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def probe_scene():
    """An ordinary scene of 1 + 2 W H small triangles on a grid: one header primitive and two per record."""
    n = 1 + 2 * W * H
    i = np.arange(n)
    corner = np.stack([(i % 512) * 0.02 - 5.0, (i // 512) * 0.02, np.full(n, 5.0)], axis=-1)
    pos = (corner[:, None, :] + np.array([[0.0, 0.0, 0.0], [0.015, 0.0, 0.0], [0.0, 0.015, 0.0]])[None]).astype(np.float32)
    nrm = np.tile(np.array([0.0, 0.0, -1.0], dtype=np.float32), (n, 3, 1))
    m = np.zeros(1, dtype=sc.MATERIAL_DTYPE)
    m["diffuse"], m["ior"], m["dissolve"] = (0.5, 0.5, 0.5), 1.0, 1.0
    return sc.build_from_triangles(pos, nrm, np.zeros(n, dtype=np.int32), m).validate()


def expected(flavour, op, words):
    if flavour == "portable":
        return po.leaf(op, words)
    return ref_gpu.probe("probe_" + op, flavour, words, me.OPS[op][2])


def left_out(op, words):
    """Rows of an operation's inputs that no flavour compares: NaN through clamp (module docstring)."""
    if op == "clamp01":
        return np.isnan(me.floats(words[:, 0]))
    return np.zeros(words.shape[0], dtype=bool)


def render_probe(renderer, scene, records, flavour, frame=0):
    """One render per W * H records; returns the (records, 3) colours."""
    out = []
    for first in range(0, records.shape[0], W * H):
        chunk = records[first:first + W * H]
        payload = me.probe_payload(chunk, W, H)
        words = scene.prims.view(np.uint32).reshape(-1, 19)
        words[:payload.shape[0], 9:18] = payload
        scene.validate()
        img = np.full((H, W, 3), -1.0, dtype=np.float32)
        renderer.render(RenderPropertiesHIP(PROBE, (W, H, 3), img, scene, pCamera=sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, frame),
                                            kernelMode=KERNEL_MODE_TILE, portableMath=flavour == "portable", strictMath=flavour == "strict"))
        out.append(img.reshape(-1, 3)[:chunk.shape[0]])
        assert (img.reshape(-1, 3)[chunk.shape[0]:] == 0).all(), "pixels past the last record must check nothing"
    return np.concatenate(out)


def run_flavour(renderer, scene, flavour):
    """Every operation and family through the probe; returns (per-record mismatch counts, row table, report lines)."""
    batches, rows = [], []
    for op in me.OPS:
        words, family, names = me.all_inputs(op)
        skip = left_out(op, words)
        assert skip.sum() <= 0.01 * words.shape[0], "more than 1 %% of %s left out" % op
        words, family = words[~skip], family[~skip]
        want = expected(flavour, op, words)
        batches.append((op, words, want))
        rows += [(op, names[f]) for f in family]
    records = me.pack_records(batches)
    colour = render_probe(renderer, scene, records, flavour)
    checked = np.array([VALUES[op] for op, _ in rows], dtype=np.float32)
    assert (colour[:, 1] == checked).all(), "values checked per record: %d records differ from what the test packed (first %s)" % (
        int((colour[:, 1] != checked).sum()), rows[int(np.argmax(colour[:, 1] != checked))])
    assert colour[:, 1].sum() == checked.sum() and checked.sum() >= 100000
    bad = colour[:, 0] != 0
    report = []
    if bad.any():
        assert (colour[bad, 2] == records[bad, 0]).all(), "the mismatching operation's id must be the record's"
        got = np.concatenate([render_probe(renderer, scene, records, flavour, frame=1), render_probe(renderer, scene, records, flavour, frame=4)[:, :1]],
                             axis=1).view(np.uint32)
        seen = {}
        for i in np.flatnonzero(bad):
            seen.setdefault(rows[i], []).append(i)
        for (op, name), idx in sorted(seen.items()):
            k, m = me.OPS[op][1], me.OPS[op][2]
            i = idx[0]
            report.append("%s / %s: %d records; first: in %s want %s got %s" % (
                op, name, len(idx), " ".join("%08x" % v for v in records[i, 1:1 + k]), " ".join("%08x" % v for v in records[i, 9:9 + m]),
                " ".join("%08x" % v for v in got[i, :m])))
    return colour[:, 0], rows, records, report


@pytest.mark.parametrize("flavour", ["default", "strict"])
def test_leaf_layer_equals_the_opencl_builtins_bit_for_bit(renderer, probe_scene, flavour):
    """Every operation and family: the HIP flavour's lt:: function returns the bits the OpenCL compiler and device library give
    for the same source expression / builtin on this GPU.  Zero mismatches; the one exclusion is NaN through clamp."""
    if not ref_gpu.available("math_probe", flavour):
        pytest.skip("oracle/_ref/math_probe.*.co not built (oracle/build_ref.sh)")
    bad, rows, records, report = run_flavour(renderer, probe_scene, flavour)
    print("%s flavour: %d records, %d values, %d mismatching values" % (flavour, len(rows), sum(VALUES[op] for op, _ in rows), int(bad.sum())))
    assert not report, "%s flavour differs from math_probe.%s.co:\n%s" % (flavour, flavour, "\n".join(report))


def test_portable_flavour_equals_the_cpu_oracle(renderer, probe_scene):
    """Bit for bit on everything but sin / cos, where the GPU's and the C library's double functions (both <= 1 ulp) may round to
    different floats on a share of 1e-10 of the arguments: at most 4 * 1e-10 * n + 1 values per function, none of
    them an exact case (0, +-inf, NaN).  Measured on the MI355X: sin 0 of 6205, cos 0 of 6205."""
    bad, rows, records, report = run_flavour(renderer, probe_scene, "portable")
    ops = np.array([op for op, _ in rows])
    for op in ("sin", "cos"):
        sel = ops == op
        n_bad = int((bad[sel] != 0).sum())
        print("portable %s: %d of %d values differ from the oracle" % (op, n_bad, int(sel.sum())))
        assert n_bad <= int(4 * DOUBLE_SINE_SHARE * sel.sum()) + 1, "\n".join(report)
        x = me.floats(records[sel, 1])
        assert not (bad[sel][(x == 0) | ~np.isfinite(x)]).any(), "an exact case of %s differs:\n%s" % (op, "\n".join(report))
    rest = [line for line in report if not line.startswith(("sin /", "cos /"))]
    assert not rest, "portable flavour differs from the CPU oracle:\n%s" % "\n".join(rest)
