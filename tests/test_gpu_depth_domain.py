"""Every kernel that reads float_depth_ on depth no uint16 millimetre image holds -- NaN, +-inf, negative, -0.0, denormal, beyond the volume,
between the millimetres, the render planes to the ulp (tests/depth_domain_frames.py) -- through the C ABI against the oracle, bit for bit:
the allocation scans and the sweep of both fields with the raycast behind them, the four routes a depth image takes into a frame, the fast and
the IEEE sweep, and the consumers (depth pyramid, bilateral filter, tracker, renderDepth).  tests/test_depth_domain_oracle.py shows on the
oracle alone that every class does what its row of RELATION says, and with a sanitized stand-alone replay that the oracle is defined on every
class these tests send through a stage."""
import numpy as np
import pytest

from oracle.binding import SDF, OraclePipeline, load, oracle_bilateral_filter, oracle_half_sample, oracle_tracking
from supereight_amd.synthetic import to_colmajor
from tests import depth_domain_frames as D
from tests.icp_edge_util import same_bits

pytestmark = pytest.mark.gpu

SMALL, LARGE = list(D.SHAPES)
POOLS = {"dense": {SMALL: 0, LARGE: 0}, "pooled": {SMALL: 1 << 13, LARGE: 1 << 14}}
ROUTE_FRAMES = 6          # raycasts at frames 3, 4, 5: on a streaming handle those of 3 and 4 ride in the scan launches of frames 4 and 5


def _assert_same_map(gpu, blocks, nodes, what):
    for name, got, want in (("blocks", gpu.blocks(), blocks), ("nodes", gpu.nodes(), nodes)):
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape, (what, name, i, g.shape, w.shape)
            if g.dtype == np.float32:
                bad = int((~same_bits(g, w)).sum())
                assert bad == 0, (what, name, i, bad)
                assert not np.isnan(g).any(), (what, name, i)
            else:
                assert (g == w).all(), (what, name, i)
    return len(blocks[0])


def _assert_same_images(v_g, n_g, v_c, n_c, what):
    assert same_bits(v_g, v_c).all() and same_bits(n_g, n_c).all(), (what, int((~same_bits(v_g, v_c)).sum()), int((~same_bits(n_g, n_c)).sum()))
    return int((n_g[..., 0] != -2).sum())


# ------------------------------------------------------------------ 1. scan, sweep, raycast
@pytest.mark.parametrize("shape", [SMALL, LARGE])
@pytest.mark.parametrize("field_name", list(D.FIELDS))
@pytest.mark.parametrize("case", D.CASES)
def test_scan_sweep_and_raycast(case, field_name, shape):
    """A dense and a pooled handle beside one run of the oracle, frame by frame: block and node sets, every voxel, flag and node value after
    every frame, and the raycast that runs."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = D.SHAPES[shape]
    field, mu = D.FIELDS[field_name]
    s = D.domain_frames(case, shape)
    gpus = {pool: DenseSLAMPipeline((W, H), N, D.DIM, field_type=field, max_blocks=POOLS[pool][shape]) for pool in POOLS}
    hits = []

    def on_frame(f, cpu, ran, v_c, n_c):
        blocks, nodes = cpu.blocks(), cpu.nodes()
        for pool, gpu in gpus.items():
            gpu.set_depth(s.depth(f))
            gpu.setPose(s.pose(f))
            assert gpu.integration(s.k, 1, mu, f) and gpu.raycasting(s.k, mu, f) == ran
            _assert_same_map(gpu, blocks, nodes, (pool, f))
            if ran:
                hits.append(_assert_same_images(*gpu.vertex_normal(), v_c, n_c, (pool, f)))

    try:
        run = D.oracle_replay(s, field_name, N, on_frame=on_frame)
        print(case, field_name, shape, "blocks", len(run["blocks"][0]), "hits", hits)
        assert len(hits) == 2 and min(hits) >= 50 and len(run["blocks"][0]) >= 300
    finally:
        for gpu in gpus.values():
            gpu.close()


@pytest.mark.parametrize("field_name", list(D.FIELDS))
@pytest.mark.parametrize("case", D.CASES)
def test_probes_and_swept_blocks(case, field_name):
    """Band steps inside the volume and blocks the sweep takes, per frame: the observables of a pixel that allocates nothing new and of a
    block that is swept without a visible change -- what tells `!(depth == 0)` from `depth > 0` on a negative pixel.  A handle that counts takes
    other kernel instantiations, hence a test of its own (as tests/test_gpu_attitudes.py::test_tumble_swept_counts)."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = D.SHAPES[SMALL]
    field, mu = D.FIELDS[field_name]
    s = D.domain_frames(case, SMALL)
    gpu = DenseSLAMPipeline((W, H), N, D.DIM, field_type=field)
    gpu.enable_stats(True)
    counted = []

    def on_frame(f, cpu, ran, v_c, n_c):
        gpu.set_depth(s.depth(f))
        gpu.setPose(s.pose(f))
        assert gpu.integration(s.k, 1, mu, f)
        g = gpu.stats(reset=True)
        counted.append((g["probes"], g["swept"]))
        _assert_same_map(gpu, cpu.blocks(), cpu.nodes(), f)

    try:
        run = D.oracle_replay(s, field_name, N, on_frame=on_frame)
        want = list(zip(run["probes"], run["swept"]))
        print(case, field_name, "probes, swept per frame (device)", counted, "(oracle)", want)
        assert counted == want and min(p for p, _ in want) > 0
    finally:
        gpu.close()


# ------------------------------------------------------------------ 2. the routes in
@pytest.fixture(scope="module")
def route_frames():
    W, H, N = D.SHAPES[LARGE]
    s = D.DomainStream("mixed", W, H, frames=ROUTE_FRAMES)
    out = {}

    def reference(field_name):
        if field_name not in out:
            casts = {}
            run = D.oracle_replay(s, field_name, N, on_frame=lambda f, cpu, ran, v, n: casts.update({f: (v, n)}) if ran else None)
            out[field_name] = (run, casts)
        return out[field_name]

    return s, reference


@pytest.mark.parametrize("route", ["pageable", "device", "pinned", "one-queue"])
@pytest.mark.parametrize("field_name", list(D.FIELDS))
def test_routes_in(route_frames, field_name, route):
    """The mixed frames as pageable host floats (copied; the scan reads the pinned copy), behind a device pointer, as pinned floats read in
    place, and on the one-queue streaming schedule, whose scans run inside k_raycast_scan: the same map, and every raycast kept in an image
    ring, against the oracle's."""
    import torch
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = D.SHAPES[LARGE]
    field, mu = D.FIELDS[field_name]
    s, reference = route_frames
    run, casts = reference(field_name)
    frames = len(s)
    gpu = DenseSLAMPipeline((W, H), N, D.DIM, field_type=field, streaming=route == "one-queue")
    ring = torch.zeros((frames, 2, H, W, 3), dtype=torch.float32, device="cuda")
    gpu.set_image_ring(ring.data_ptr(), frames, keepalive=ring)
    try:
        if route in ("device", "one-queue"):
            dev = torch.from_numpy(np.stack(s.depths)).cuda()
            assert gpu.frame_is_fused() == (route == "one-queue")
            for f in range(frames):
                assert gpu.frame(dev[f].data_ptr(), to_colmajor(s.pose(f)), s.k, mu, f) == (3 if f > 2 else 1)
            assert gpu.launch_counts()["fused"] == (frames - 4 if route == "one-queue" else 0)
        else:
            pinned = []
            if route == "pinned":
                gpu.set_pinned_input(True)
                pinned = [gpu.pinned_image(np.float32) for _ in range(4)]          # unmodified until three further uploads
            scratch = np.empty((H, W), np.float32)
            for f in range(frames):
                if route == "pinned":
                    pinned[f % 4][:] = s.depth(f)
                    gpu.set_depth(pinned[f % 4])
                else:
                    scratch[:] = s.depth(f)
                    gpu.set_depth(scratch)
                    scratch[:] = 0                                                   # copied: the caller's buffer is free at once
                gpu.setPose(s.pose(f))
                assert gpu.integration(s.k, 1, mu, f) and gpu.raycasting(s.k, mu, f) == (f > 2)
        gpu.sync()
        blocks = _assert_same_map(gpu, run["blocks"], run["nodes"], route)
        images = ring.cpu().numpy()
        hits = [_assert_same_images(images[f, 0], images[f, 1], *casts[f], (route, f)) for f in sorted(casts)]
        print(field_name, route, "blocks", blocks, "hits", hits)
        assert sorted(casts) == [3, 4, 5] and min(hits) >= 1000 and blocks >= 1000
    finally:
        gpu.close()


# ------------------------------------------------------------------ 3. fast and IEEE sweeps
@pytest.mark.parametrize("field_name", list(D.FIELDS))
@pytest.mark.parametrize("case", ["mixed", "pinf", "far", "tiny"])
def test_fast_and_ieee_sweeps_give_the_same_map(case, field_name, monkeypatch):
    """tests/test_gpu_sweep_arith.py's end-to-end case on quotients that overflow or are NaN: k_integrate<FAST> (shared refined reciprocal) and
    the compiler's own divisions (SE_HIP_IEEE_SWEEP=1) give byte-identical blocks and nodes."""
    import torch
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = D.SHAPES[LARGE]
    field, mu = D.FIELDS[field_name]
    s = D.domain_frames(case, LARGE)
    dev = torch.from_numpy(np.stack(s.depths)).cuda()

    def run(ieee):
        if ieee:
            monkeypatch.setenv("SE_HIP_IEEE_SWEEP", "1")
        else:
            monkeypatch.delenv("SE_HIP_IEEE_SWEEP", raising=False)
        p = DenseSLAMPipeline((W, H), N, D.DIM, field_type=field)      # (the knob is read once, here)
        for f in range(len(s)):
            p.frame(dev[f].data_ptr(), to_colmajor(s.pose(f)), s.k, mu, f)
        out = p.blocks() + p.nodes()
        p.close()
        return out

    a, b = run(False), run(True)
    assert len(a[0]) >= 1000
    for u, v in zip(a, b):
        assert u.shape == v.shape and (u.view(np.uint8) == v.view(np.uint8)).all()


# ------------------------------------------------------------------ 4. the consumers
def _consumer_frames(shape, classes):
    from supereight_amd.synthetic import SyntheticStream
    from tests.edge_frames import CONSUMER, RoomStream
    if shape == "160x120":
        return D.ConsumerFrames(classes, 160, 120, D.DIM, base=SyntheticStream(160, 120, D.DIM)), 256
    c = CONSUMER
    return D.ConsumerFrames(classes, c["W"], c["H"], c["dim"], base=RoomStream(c["W"], c["H"], c["dim"], c["k"])), c["N"]


@pytest.fixture(scope="module", params=["160x120", "163x101"])
def tracked(request):
    """Four clean frames fused and raycast on both sides (SDF, mu 0.1), and the fifth frame, which holds TRACKED."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    c, N = _consumer_frames(request.param, D.TRACKED)
    mu = 0.1
    cpu = OraclePipeline(SDF, N, c.dim, c.W, c.H)
    gpu = DenseSLAMPipeline((c.W, c.H), N, c.dim, field_type=SDF)
    for f in range(4):
        gpu.set_depth(c.depths[f]); gpu.setPose(c.poses[f])
        cpu.integrate(c.depths[f], c.poses[f], c.k, mu, f); gpu.integration(c.k, 1, mu, f)
        ran, v, n = cpu.raycast(c.poses[f], c.k, mu, f); gpu.raycasting(c.k, mu, f)
    cpu.close()
    assert ran and _assert_same_images(*gpu.vertex_normal(), v, n, "reference images") > 1000
    depth = c.depths[4]
    held = depth[c.masks[4]]
    assert np.isnan(held).sum() > 100 and (held < 0).sum() > 100 and (np.signbit(held) & (held == 0)).sum() > 20
    yield c, gpu, v, n, depth
    gpu.close()


def test_tracking_a_frame_with_nan_negative_and_offgrid_depth(tracked):
    """k_depth_pyramid (the float4 path at 160x120, the scalar path at 163x101), k_vertex_normal_levels and the ICP on a (4, 3, 2) pyramid:
    scaled_depth(0..2) with their NaN pixels, the decision, the iteration count, the 32 sums, tracking_result_ and the pose."""
    c, gpu, v, n, depth = tracked
    pyramid = (4, 3, 2)
    ok_c, pose_c, track_c, red_c, it_c = oracle_tracking(depth, c.k, c.poses[3], c.poses[3], v, n, 1e-5, pyramid)
    gpu.filter_depth(False)
    gpu.set_depth(depth)
    gpu.setPose(c.poses[3])
    ok_g = gpu.tracking(c.k, 1e-5, 1, 4, pyramid)
    l1 = oracle_half_sample(depth, 0.1 * 3, 1)
    l2 = oracle_half_sample(l1, 0.1 * 3, 1)
    for level, want in enumerate((depth, l1, l2)):
        got = gpu.scaled_depth(level)
        assert got.shape == want.shape and same_bits(got, want).all(), level
    assert np.isnan(l1).sum() > 20 and np.isnan(l2).sum() > 5 and (l1 < 0).sum() > 20       # a NaN centre is 0 / 0, a negative one survives
    track_g, red_g, it_g = gpu.track_data()
    print(c.W, c.H, "tracked", ok_c, "iterations", it_c, "inliers", red_c[28])
    assert (ok_g, it_g) == (ok_c, it_c) and ok_c and it_c >= 3 and red_c[28] > 1000
    assert same_bits(red_g, red_c).all(), (red_g, red_c)
    assert same_bits(gpu.getPose(), pose_c).all()
    assert (track_g["result"] == track_c["result"]).all()
    good = track_c["result"] == 1
    assert same_bits(track_g["error"][good], track_c["error"][good]).all() and same_bits(track_g["J"][good], track_c["J"][good]).all()
    bad = c.masks[4] & ~(depth > 0)                              # NaN, negative and -0.0 pixels have no vertex (`d > 0`), hence no normal
    assert (track_c["result"][bad] == -1).all()


def test_bilateral_filter_of_such_a_frame(tracked):
    """filter_depth(True): scaled_depth(0) is the oracle's bit for bit on every finite pixel (the filter's exponential is defined:
    so_exp_f32 / se_exp_f32), its NaN pattern the oracle's exactly, zeros preserved."""
    c, gpu, v, n, depth = tracked
    gpu.filter_depth(True)
    try:
        gpu.set_depth(depth)
        gpu.setPose(c.poses[3])
        ok_g = gpu.tracking(c.k, 1e-5, 1, 4, (4, 3, 2))
        filt_g, filt_c = gpu.scaled_depth(0), oracle_bilateral_filter(depth)
    finally:
        gpu.filter_depth(False)
    assert (np.isnan(filt_g) == np.isnan(filt_c)).all()
    assert np.isnan(filt_c).sum() >= np.isnan(depth).sum() > 100                  # a NaN centre stays NaN, a negative one has no neighbour near it
    assert ((filt_g == 0) == (filt_c == 0)).all() and ((filt_c == 0) == (depth == 0)).all()
    fin = np.isfinite(filt_c) & (filt_c != 0)
    differ = int((filt_g[fin].view(np.uint32) != filt_c[fin].view(np.uint32)).sum())
    print(c.W, c.H, "filtered: NaN", int(np.isnan(filt_c).sum()), "finite pixels that differ", differ, "tracked", ok_g)
    assert fin.sum() > 0.5 * c.W * c.H and differ == 0
    ok_c, *_ = oracle_tracking(filt_c, c.k, c.poses[3], c.poses[3], v, n, 1e-5, (4, 3, 2))
    assert ok_g == ok_c


@pytest.mark.parametrize("shape", ["160x120", "163x101"])
def test_render_depth_of_every_class_it_is_defined_on(shape):
    """renderDepth of an image that holds the planes to the ulp, negative, denormal, infinite, far and off-grid depth, byte for byte."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    c, N = _consumer_frames(shape, D.RENDERED)
    depth = c.depths[4]
    ref = np.zeros((c.H, c.W, 4), np.uint8)
    load().so_render_depth(ref.reshape(-1), depth.reshape(-1), c.W, c.H)
    gpu = DenseSLAMPipeline((c.W, c.H), N, c.dim, field_type=SDF, max_blocks=1 << 10)
    try:
        gpu.set_depth(depth)
        got = gpu.renderDepth()
    finally:
        gpu.close()
    assert (got == ref).all()
    held = ref[c.masks[4]].reshape(-1, 4)
    white, black = (held[:, :3] == 255).all(axis=1).sum(), (held[:, :3] == 0).all(axis=1).sum()
    # below the near plane, beyond the far plane, and in between: the planes themselves, their inner neighbours and the off-grid share
    assert white > 100 and black > 100 and len(np.unique(held, axis=0)) >= 10 and len(np.unique(ref.reshape(-1, 4), axis=0)) > 50
