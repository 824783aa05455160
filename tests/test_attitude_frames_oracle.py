"""CPU side of tests/test_gpu_attitudes.py: the scene renderer is the stress stream's where their cameras agree, and every attitude the GPU tests
compare with the oracle exercises, on the oracle alone, what its table entry says -- enough blocks and fused voxels, band steps that leave the
volume, a camera that fuses nothing, a camera on an existing block's corner, and in the tumble blocks that are swept from behind the camera -- so
that no case can turn into a comparison of two empty or untouched maps unnoticed."""
import numpy as np
import pytest

from oracle.binding import SDF, OraclePipeline
from supereight_amd.synthetic import intrinsics, render_stress_depth, stress_pose
from tests.attitude_frames import (ATTITUDES, CORNER_ATTITUDES, DIM, FIELDS, SHAPES, TUMBLE, AttitudeStream, aniso_k, attitude_pose,
                                   behind_and_in_image, block_key, camera_frame, corner_block, metres, node_corners_m, ofusion_steps,
                                   render_scene_mm, sdf_steps)

SHAPE_IDS = list(SHAPES)
FIELD_IDS = list(FIELDS)


@pytest.mark.parametrize("W,H", [(80, 60), (160, 120), (83, 61)])
def test_scene_renderer_is_the_stress_stream_at_its_poses(W, H):
    k = intrinsics(W, True)
    for f in (0, 7, 30, 45, 90, 135, 179):       # yaw 0, +-90 deg and in between, pitch of either sign
        want = np.clip(np.floor(render_stress_depth(f, W, H, DIM) * 1000.0), 0, 65535).astype(np.uint16)
        got = render_scene_mm(stress_pose(f, DIM), W, H, DIM, k)
        assert got.dtype == np.uint16 and got.shape == (H, W) and (got == want).all(), f


def test_scene_renderer_outside_the_room_and_past_everything():
    W, H = 80, 60
    k = intrinsics(W)
    # outside the room: no wall, only the spheres and the pillar; what meets nothing is 0
    mm = render_scene_mm(attitude_pose("outside_low", DIM, 128), W, H, DIM, k)
    assert 100 < (mm != 0).sum() < W * H // 2 and (mm == 0).sum() > W * H // 2
    assert mm[mm != 0].min() > 1000 * 0.5 * DIM * 0.9          # nothing nearer than the pillar, 0.86 dim away
    # inside: every ray ends on a wall
    assert (render_scene_mm(attitude_pose("-z", DIM, 128), W, H, DIM, k) != 0).all()
    # far outside, looking away: nothing at all
    away = attitude_pose("outside_low", DIM, 128).copy()
    away[:3, :3] = attitude_pose("-z", DIM, 128)[:3, :3]
    assert (render_scene_mm(away, W, H, DIM, k) == 0).all()
    # 65.535 m is the most the format holds: a wall 100 m away through a scaled scene is clipped, not wrapped
    far = render_scene_mm(attitude_pose("-z", 100.0, 128), W, H, 100.0, k)
    assert far.max() == 65535 and np.isfinite(metres(far)).all()


def test_tables_hold_what_the_gpu_tests_need():
    for name, (make, purpose) in ATTITUDES.items():
        T = make(DIM, 128)
        assert T.dtype == np.float32 and T.shape == (4, 4) and purpose, name
        R = T[:3, :3].astype(np.float64)
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-6) and np.linalg.det(R) > 0.999, name
    exact = ("+z", "-z", "+x", "-x", "+y", "-y", "roll90", "roll180", "roll270", "on_block_corner_axis")
    axes = set()
    for name in exact:
        R = attitude_pose(name, DIM, 128)[:3, :3]
        assert np.isin(R, (-1.0, 0.0, 1.0)).all() and (np.abs(R).sum(axis=0) == 1).all(), name     # a signed permutation: exact zeros
        axes.add(tuple(R[:, 2]))
    assert len(axes) == 6                                                                           # the optical axis along +-x, +-y, +-z
    for name in ("generic", "generic_pitched", "on_block_corner"):
        assert (attitude_pose(name, DIM, 128)[:3, :3] != 0).all(), name
    assert abs(attitude_pose("generic_pitched", DIM, 128)[1, 2]) > np.sin(np.pi / 4)                # optical axis more than 45 deg off the horizon
    for name, axis, side in (("outside_low", 2, -1), ("outside_high", 0, 1)):
        t = attitude_pose(name, DIM, 128)[:3, 3] / DIM
        beyond = -t[axis] if side < 0 else t[axis] - 1.0
        assert 0.3 <= beyond <= 0.8, name
    for N in (128, 256):
        for name in CORNER_ATTITUDES:
            t = attitude_pose(name, DIM, N)[:3, 3]
            want = corner_block(N).astype(np.float32) * (np.float32(DIM) / np.float32(N))
            assert (corner_block(N) % 8 == 0).all() and (t.view(np.uint32) == want.view(np.uint32)).all(), (name, N)
    assert 12 <= len(TUMBLE) <= 14 and len(set(TUMBLE)) == len(TUMBLE) and set(TUMBLE) <= set(ATTITUDES)
    assert TUMBLE.index("on_block_corner") >= 8
    for a, b in zip(TUMBLE, TUMBLE[1:]):            # consecutive frames look in opposite or orthogonal directions, give or take 60 deg
        za, zb = attitude_pose(a, DIM, 128)[:3, 2], attitude_pose(b, DIM, 128)[:3, 2]
        assert float(za @ zb) < 0.5, (a, b)


def _fused(o, field):
    c, x, _, _ = o.blocks()
    return len(c), int((x != (1.0 if field == SDF else 0.0)).sum())        # initValue().x


@pytest.mark.parametrize("shape", SHAPE_IDS)
@pytest.mark.parametrize("field_name", FIELD_IDS)
@pytest.mark.parametrize("name", list(ATTITUDES))
def test_single_attitude_is_not_vacuous_on_the_oracle(name, field_name, shape):
    """Two frames of one attitude on an empty map.  `probes` counts the band steps INSIDE the volume, one per step, for both fields
    (se_oracle.cpp buildAllocationList / buildOctantList: ++probes behind the six range tests) -- as the device's counter does
    (se_scan_sdf_wg / se_scan_ofusion_wg) --, so probes < valid pixels x steps per ray means that band steps left the volume."""
    W, H, N = SHAPES[shape]
    field, mu = FIELDS[field_name]
    k = intrinsics(W)
    T = attitude_pose(name, DIM, N)
    mm = render_scene_mm(T, W, H, DIM, k)
    depth = metres(mm)
    valid = int((mm != 0).sum())
    o = OraclePipeline(field, N, DIM, W, H)
    o.count_stats(True)
    try:
        if name in CORNER_ATTITUDES:
            o.insert_octants(block_key(o.lib, corner_block(N), N))
            coords = o.blocks()[0]
            assert len(coords) == 1 and (coords[0] == corner_block(N)).all()            # the block on whose min corner the camera stands exists
            assert (coords[0].astype(np.float32) * (np.float32(DIM) / np.float32(N)) == T[:3, 3]).all()
        for f in range(2):
            assert o.integrate(depth, T, k, mu, f)
        st = o.stats()
        blocks, voxels = _fused(o, field)
    finally:
        o.close()
    steps = 2 * (valid * sdf_steps(mu, DIM, N) if field == SDF else ofusion_steps(depth, T, k, mu, DIM, N))
    print(name, field_name, shape, "blocks", blocks, "voxels", voxels, "valid", valid, "probes", st["probes"], "of", steps, "swept", st["swept"])
    assert st["truncated"] == 0 and st["oob_ub"] == 0, st
    if name == "looking_out":
        assert valid > 1000 and st["probes"] == 0 and blocks == 0, (valid, st, blocks)
        return
    assert blocks >= 50 and voxels >= 2000, (blocks, voxels)
    assert 0 < st["probes"] <= steps, (st, steps)
    if name in ("outside_low", "outside_high", "surface_outside"):
        assert st["probes"] < steps, (st, steps)


@pytest.mark.parametrize("field_name", FIELD_IDS)
def test_looking_out_leaves_a_filled_map_alone_on_the_oracle(field_name):
    """What the GPU test runs: a +z frame fills the map, then two frames look out.  The block set does not change and no band step is counted."""
    W, H, N = SHAPES[SHAPE_IDS[0]]
    field, mu = FIELDS[field_name]
    k = intrinsics(W)
    o = OraclePipeline(field, N, DIM, W, H)
    o.count_stats(True)
    try:
        T = attitude_pose("+z", DIM, N)
        o.integrate(metres(render_scene_mm(T, W, H, DIM, k)), T, k, mu, 0)
        before, probes = o.blocks()[0].copy(), o.stats()["probes"]
        T = attitude_pose("looking_out", DIM, N)
        depth = metres(render_scene_mm(T, W, H, DIM, k))
        for f in (1, 2):
            o.integrate(depth, T, k, mu, f)
        after = o.blocks()[0]
        assert len(before) >= 50 and before.shape == after.shape and (before == after).all()
        assert (depth != 0).sum() > 1000 and o.stats()["probes"] == probes
    finally:
        o.close()


TUMBLE_RUNS = [(s, f, False) for s in SHAPE_IDS for f in FIELD_IDS] + [(SHAPE_IDS[1], "sdf", True), (SHAPE_IDS[0], "ofusion", True)]


@pytest.mark.parametrize("shape,field_name,aniso", TUMBLE_RUNS, ids=[f"{s}-{f}{'-aniso' if a else ''}" for s, f, a in TUMBLE_RUNS])
def test_tumble_is_not_vacuous_on_the_oracle(shape, field_name, aniso):
    """One frame of each kind the GPU test is about: (i) the block count grows, (ii) swept < blocks, (iii) blocks go from active to inactive,
    (iv) a block inactive before the frame lies behind the camera and projects into the image, (v) a node corner lies behind the camera; and
    the raycasts see something.  No key list is truncated.  (In this 2.4 m volume blocks exist in the outermost layers, and some raycast samples -- from the
    cameras outside most of all -- fall past a face at a place where the position modulo size holds a block: the reference indexes out of bounds
    there, oracle and device both read "not allocated" (se_oracle.cpp, count_oob).  stats()["oob_ub"] counts those reads, some 2 000 to 6 000
    per run, all of them in raycasts; it is printed, not bounded -- integration, which this is about, counts none, and that is asserted.)"""
    W, H, N = SHAPES[shape]
    field, mu = FIELDS[field_name]
    s = AttitudeStream(W, H, N, k=aniso_k(W) if aniso else None)
    voxel = DIM / N
    o = OraclePipeline(field, N, DIM, W, H)
    o.count_stats(True)
    grows, partial, deactivated, behind, nodes_behind, hits = [], [], [], [], [], []
    try:
        for f, name in enumerate(s.names):
            T = s.pose(f)
            c0, _, _, a0 = o.blocks()
            code, side, _, _ = o.nodes()
            if name in CORNER_ATTITUDES:          # the corner camera's block exists by now, through fusion
                assert (c0 == corner_block(N)).all(axis=1).any(), (f, name)
            oob = o.stats()["oob"]
            assert o.integrate(s.depth(f), T, s.k, mu, f)
            assert o.stats()["oob"] == oob, f
            ran, _, n = o.raycast(T, s.k, mu, f)
            assert ran == (f > 2)
            if ran:
                hits.append(int((n[..., 0] != -2).sum()))
            c1, _, _, a1 = o.blocks()
            st = o.stats()
            assert st["truncated"] == 0, (f, st)
            # (blocks are sorted by key and never leave: those of before are a subset of those of after)
            index = {tuple(c): i for i, c in enumerate(c1.tolist())}
            was = np.array([index[tuple(c)] for c in c0.tolist()], np.int64)
            grows.append(len(c1) > len(c0))
            partial.append(st["swept"] < len(c1))
            deactivated.append(int(((a0 == 1) & (a1[was] == 0)).sum()) if len(c0) else 0)
            # blocks inactive before the frame whose min corner lies behind the camera and projects into the image: only se_in_frustum's
            # missing z > 0 test can put them on the sweep's list
            behind.append(int(behind_and_in_image(c0[a0 == 0] * voxel, T, s.k, W, H, margin=2.0).sum()) if len(c0) else 0)
            nodes_behind.append(int((camera_frame(node_corners_m(o.lib, code, side, DIM, N), T)[:, 2] < 0).sum()))
        oob_ub = st["oob_ub"]
    finally:
        o.close()
    print(shape, field_name, "oob_ub", oob_ub, "grows", grows, "swept<blocks", partial, "deactivated", deactivated, "behind", behind, "node corners behind", nodes_behind, "hits", hits)
    assert any(grows) and any(partial) and max(deactivated) > 0
    assert max(behind) > 0 and max(nodes_behind) > 0
    assert len(hits) == len(TUMBLE) - 3 and sum(h >= 50 for h in hits) * 2 >= len(hits), hits
