"""k_bilateral_filter, and the k_depth_pyramid pass that runs behind it (store0 = 0: level 0 is already in place), against the oracle bit for
bit: scaled_depth(0) against so_bilateral_filter, scaled_depth(1) and (2) against halfSampleRobustImageKernel of the oracle's filtered image.
The exponential is DEFINED (so_exp_f32 / se_exp_f32, tests/test_exp_host.py), so nothing here holds a tolerance; where the oracle's value is a
NaN the device's must be one (tests/icp_edge_util.py same_bits).

The image is read the way the library offers it: filter_depth(True), set_depth, one tracking call, scaled_depth.  The handle is fresh -- no map,
the reference images zero -- and what the tracker makes of that is not the subject.  A level exists while it keeps a pixel a side
(se_hip_track refuses a deeper pyramid), so 2x1 is filtered with one level and 2x2, 3x5, 5x3, 255x2, 256x2 and 257x3 with two."""
import numpy as np
import pytest

from oracle.binding import SDF, oracle_bilateral_filter, oracle_half_sample
from tests import bilateral_util as B
from tests import depth_domain_frames as D
from tests.icp_edge_util import same_bits

pytestmark = pytest.mark.gpu


def _k_of(W, H):
    return np.asarray([W, W, 0.5 * W, 0.5 * H], np.float32)


@pytest.fixture(params=B.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def handle(request):
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H = request.param
    gpu = DenseSLAMPipeline((W, H), 64, 2.4, field_type=SDF, max_blocks=1 << 10)
    gpu.filter_depth(True)
    yield W, H, gpu
    gpu.close()


def _filtered_on_device(gpu, image, k, levels):
    gpu.set_depth(image)
    gpu.setPose(np.eye(4, dtype=np.float32))
    gpu.tracking(k, 1e-5, 1, 0, (1,) * levels)
    return [gpu.scaled_depth(level) for level in range(levels)]


def _filtered_on_oracle(image, levels):
    out = [oracle_bilateral_filter(image)]
    for _ in range(1, levels):
        out.append(oracle_half_sample(out[-1], B.E_DELTA * 3, 1))
    return out


def _assert_same_pyramid(got, want, what):
    for level, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, level, g.shape, w.shape)
        same = same_bits(g, w)
        bad = np.argwhere(~same)
        assert same.all(), (what, level, len(bad), [(int(y), int(x), float(g[y, x]), float(w[y, x])) for y, x in bad[:4]])


def test_filter_and_pyramid_at_every_shape(handle):
    """The seeded millimetre image, the constant image, all zeros, one pixel among zeros, a vertical and a horizontal step (two different
    images: an exchanged clamp or loop order shows on one of them), and the left-right and top-bottom mirror images of the seeded one, each
    against the oracle's output of that same image."""
    W, H, gpu = handle
    levels, k = B.levels_of(W, H), _k_of(W, H)
    images = B.images(W, H)
    want = {name: _filtered_on_oracle(img, levels) for name, img in images.items()}
    # what the images are there for, on the oracle alone
    two = np.float32(2.0)
    assert (want["constant"][0] == two).all() and (want["zeros"][0].view(np.uint32) == 0).all()          # c * sum / sum: exact for a power of two
    if W >= 5 and H >= 5:                                       # beyond the reach of both clamps the window holds the pixel once: (1 * c) / 1
        assert (want["single"][0].view(np.uint32) == images["single"].view(np.uint32)).all()
    assert ((want["single"][0] != 0) == (images["single"] != 0)).all()
    assert not same_bits(want["random"][0], images["random"]).all()                                         # the filter does something
    assert not same_bits(want["step_vertical"][0], want["step_horizontal"][0]).all()
    for name, img in images.items():
        got = _filtered_on_device(gpu, img, k, levels)
        _assert_same_pyramid(got, want[name], (W, H, name))
        assert ((got[0] == 0) == (img == 0)).all()


def _domain_image(case, W, H):
    from supereight_amd.synthetic import SyntheticStream
    from tests.edge_frames import CONSUMER, RoomStream
    if (W, H) == (160, 120):
        base, dim = SyntheticStream(W, H, D.DIM), D.DIM
    else:
        assert (W, H) == (CONSUMER["W"], CONSUMER["H"])
        base, dim = RoomStream(W, H, CONSUMER["dim"], CONSUMER["k"]), CONSUMER["dim"]
    s = D.DomainStream(case, W, H, dim, frames=1, first=0, base=base)
    return s.depths[0], s.masks[0], s.k


def _window_has_positive(depth):
    """Per pixel: does its clamped 5x5 window hold a pixel > 0 (clamping repeats border pixels and adds none)."""
    H, W = depth.shape
    pos = np.pad(depth > 0, 2, mode="edge")
    out = np.zeros((H, W), bool)
    for dy in range(5):
        for dx in range(5):
            out |= pos[dy:dy + H, dx:dx + W]
    return out


@pytest.mark.parametrize("shape", [(160, 120), (163, 101)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_of_depth_no_millimetre_image_holds(shape):
    """The classes of tests/depth_domain_frames.py, each alone and all in one image (`mixed`), put into a tenth of a room frame and one 16x16
    patch: NaN of both signs, +-inf, negative values, -0.0, denormals, 1000 m, the render planes to the ulp, off-grid room depth.  On the
    oracle: a NaN centre stays NaN, a negative centre (-inf too) with no positive pixel in its window is 0 / 0, zero (of either sign) stays
    +0, and no pixel comes out infinite -- an infinite neighbour gives a weight of exp(-inf) = 0 and 0 * inf = NaN.  The device: bit for bit."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H = shape
    levels = B.levels_of(W, H)
    gpu = DenseSLAMPipeline((W, H), 64, 2.4, field_type=SDF, max_blocks=1 << 10)
    gpu.filter_depth(True)
    seen = {}
    try:
        for case in D.CASES:
            depth, mask, k = _domain_image(case, W, H)
            want = _filtered_on_oracle(depth, levels)
            f0 = want[0]
            nan_centre = np.isnan(depth)
            alone = (depth < 0) & ~_window_has_positive(depth)
            assert np.isnan(f0[nan_centre]).all() and np.isnan(f0[alone]).all() and (f0[depth == 0].view(np.uint32) == 0).all()
            assert not np.isinf(f0).any()
            seen[case] = dict(nan=int(nan_centre.sum()), alone=int(alone.sum()), zero=int((depth == 0).sum()), nan_out=int(np.isnan(f0).sum()))
            got = _filtered_on_device(gpu, depth, k, levels)
            _assert_same_pyramid(got, want, (W, H, case))
    finally:
        gpu.close()
    print(W, H, seen)
    assert seen["nan"]["nan"] > 500 and seen["mixed"]["nan"] > 50
    assert seen["negative"]["alone"] > 50 and seen["ninf"]["alone"] > 50
    assert seen["negzero"]["zero"] > seen["offgrid"]["zero"] and seen["offgrid"]["nan_out"] == 0
    assert seen["pinf"]["nan_out"] > 500 and seen["far"]["nan_out"] == 0
