"""GPU test (-m gpu) of random()'s short sine (lt_device.hpp: random_fast_r): a probe program, compiled at run time,
compares random_ / randoms_ / random_x_ with random_library_ -- today's expression with the library's sine -- bit for bit on
every pixel of a 480 x 270 film over 5 frames: 96 seeds per frame and their negated arguments, the same seeds four at a time,
arguments built to sit on float ties, and edge values (zeros, multiples and neighbours of pi and pi / 2, denormals, 2^40 where
the library's fmod takes over, infinities, NaN).  In the default (as shipped) and the portable flavour."""
import os

import numpy as np
import pytest

from lens_trace_amd import scene as sc
from lens_trace_amd.renderer import RendererHIP, RenderPropertiesHIP
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "user_kernels")
W, H, FRAMES = 480, 270, 5
SEEDED = 2 * 96              # per pixel and frame: the seeds' own arguments and their negatives
CHECKED = SEEDED + 96 + 14 + 25
RATE = 2.0 ** -21            # 2 delta 2^24 with delta = 2^-46: the derived bound of the fallback rate per value


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    yield r
    r.close()


@pytest.mark.parametrize("portable", [False, True], ids=["default", "portable"])
def test_random_is_the_library_expression_bit_for_bit(renderer, portable):
    s = sc.load_ltsb(os.path.join(GOLDEN, "cornell_box_O0.ltsb")).validate()
    seeded = rest = 0
    for frame in range(FRAMES):
        out = np.empty((H, W, 3), dtype=np.float32)
        cam = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, frame)
        renderer.render(RenderPropertiesHIP(os.path.join(HERE, "random_check.hip"), (W, H, 3), out, s, pCamera=cam, portableMath=portable))
        assert out[..., 1].min() == out[..., 1].max() == CHECKED
        assert out[..., 0].max() == 0.0, "frame %d: %d pixels saw a difference" % (frame, int((out[..., 0] != 0).sum()))
        fell = out[..., 2].astype(np.int64)
        seeded += int((fell % 1024).sum())
        rest += int((fell // 1024).sum())
    n = W * H * FRAMES * SEEDED
    print("fallbacks: %d of %d seeded values (derived bound %.1f), %d of the tie-built and edge values" % (seeded, n, n * RATE, rest))
    assert seeded <= 4 * RATE * n
    assert seeded + rest > 0
    # every pixel's edge list holds 2^40, -2^40, 1e300, two infinities and a NaN, which never take the fast path, and its 14
    # tie-built values lie within a few 2^-52 of a tie (the library's asin and three neighbours), inside the bracket of 2^-46
    assert rest >= (6 + 14) * W * H * FRAMES
