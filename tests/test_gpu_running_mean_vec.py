"""GPU tests (-m gpu) of the fold's four-floats-per-thread form (lt_capi.hip: lt_running_mean4_kernel), which a fused launch's fold
takes when every float of its range is folded (depth 3, no padded tiles) and the output takes 16-byte stores; everything else keeps
lt_running_mean_kernel.  Not a bit may change: every call is compared with LT_FUSED_FRAMES=0 (one launch per frame, the running mean
in the render kernel's own store).

The images are rows of 1, 2, 3, 12, 13 and 4099 pixels -- 3, 6, 9, 36, 39 and 12297 floats: every remainder modulo four, so the last
thread's four floats straddle the end by one, two and three floats, images shorter than one thread's four floats, more than one
block (4099 pixels: 13 blocks of 1024 floats), and sample images that lie a number of floats apart that is no multiple of four (the
frames' loads are then not 16-byte aligned).  7 frames in one launch are one round of four frames in flight and three behind it; cut
into launches of three they end in a fold of a single frame."""
import ctypes

import numpy as np
import pytest

from lens_trace_amd import _capi as C
from lens_trace_amd import scene as sc
from lens_trace_amd import synth
from lens_trace_amd.renderer import RendererHIP, make_desc

pytestmark = pytest.mark.gpu

CAM = sc.camera_bytes(0.0, 2.5, -50.0, 0.0, 0.0, 0.0, 1)
ROWS = (1, 2, 3, 12, 13, 4099)


@pytest.fixture(scope="module")
def renderer():
    r = RendererHIP(0)
    r.set_scene(synth.heightfield_wall(24).validate())
    yield r
    r.close()


@pytest.fixture(autouse=True)
def fixed_shadow_walk(monkeypatch):
    monkeypatch.setenv("LT_SHADOW_PACKETS", "1")   # no timing launches between the two calls compared


def render(r, W, H, count, base, depth=3, tile=None, first=2):
    d = make_desc(C.PROGRAM_ACCUMULATOR, W, H, depth, CAM, frame_first=first, frame_count=count, accumulate=True, accumulate_base=base, tile=tile)
    n = r.output_floats(d)
    out = (np.arange(n, dtype=np.float32) % 7.0) / 7.0   # (a running mean with accumulate_base > 0 reads it)
    r._check(r._L.lt_hip_render(r._ctx, ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out, r.stats()["kernel_launches"]


def fused_and_not(monkeypatch, fn, launches):
    """fn() as fused launches (`launches` of them) and with LT_FUSED_FRAMES=0: equal bits."""
    got, n = fn()
    assert n == launches, (n, launches)
    monkeypatch.setenv("LT_FUSED_FRAMES", "0")
    want, _ = fn()
    monkeypatch.delenv("LT_FUSED_FRAMES")
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), "%d of %d floats differ" % (int((~same).sum()), got.size)
    return got


@pytest.mark.parametrize("base", [0, 5])
@pytest.mark.parametrize("W", ROWS)
def test_rows_of_every_length(renderer, monkeypatch, W, base):
    fused_and_not(monkeypatch, lambda: render(renderer, W, 1, 7, base), 1)
    fused_and_not(monkeypatch, lambda: render(renderer, W, 1, 1, base), 1)   # (one frame: nothing to fold)
    monkeypatch.setenv("LT_FUSED_BYTES", str(3 * W * 3 * 4 + 8))            # three sample images per launch: 3 + 3 + 1
    fused_and_not(monkeypatch, lambda: render(renderer, W, 1, 7, base), 3)


@pytest.mark.parametrize("base", [0, 5])
def test_padded_tiles_keep_the_old_form(renderer, monkeypatch, base):
    # (131 x 77 in tiles of 24 x 20: the edge tiles' pixels outside the image are in the buffer and are not to be touched)
    got = fused_and_not(monkeypatch, lambda: render(renderer, 131, 77, 7, base, tile=(24, 20, 0, 1)), 1)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("base", [0, 5])
def test_depth_4_keeps_the_old_form(renderer, monkeypatch, base):
    # (the fourth channel is not the fold's: a thread's four floats would hold it)
    fused_and_not(monkeypatch, lambda: render(renderer, 13, 5, 7, base, depth=4), 1)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_output_at_every_alignment(renderer, monkeypatch, offset):
    """lt_hip_render_device into a caller's buffer that starts `offset` floats behind a 16-byte boundary: only offset 0 takes 16-byte
    stores."""
    import torch
    W, H, count, base = 13, 3, 7, 5
    d = make_desc(C.PROGRAM_ACCUMULATOR, W, H, 3, CAM, frame_first=2, frame_count=count, accumulate=True, accumulate_base=base)
    n = renderer.output_floats(d)
    start = (np.arange(n, dtype=np.float32) % 7.0) / 7.0
    images = []
    for fused in ("1", "0"):
        monkeypatch.setenv("LT_FUSED_FRAMES", fused)
        buf = torch.full((n + 8,), -1.0, dtype=torch.float32, device="cuda:0")
        buf[offset:offset + n] = torch.from_numpy(start).to(buf.device)
        torch.cuda.synchronize()
        renderer.render_device(d, buf.data_ptr() + 4 * offset, 4 * n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:offset] == -1.0).all() and (host[offset + n:] == -1.0).all()   # nothing outside the image was written
        images.append(host[offset:offset + n])
    assert np.array_equal(images[0].view(np.uint32), images[1].view(np.uint32))


@pytest.mark.parametrize("W,H", [(512, 192), (349, 251)], ids=["512x192", "349x251"])
def test_pieced_read_back(renderer, monkeypatch, W, H):
    """Images of 1 MiB and more come back in eight pieces and their last fold is cut into the same pieces (launch_running_mean):
    512 x 192 in whole pieces, 349 x 251 (262 797 floats) with a last piece whose last thread straddles the end."""
    assert W * H * 3 * 4 >= 1 << 20
    fused_and_not(monkeypatch, lambda: render(renderer, W, H, 3, 5), 1)
