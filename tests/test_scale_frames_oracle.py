"""CPU side of tests/test_gpu_scales.py: every case of tests/scale_frames.py is well posed on the oracle alone (no key-list truncation, no
undefined out-of-volume read) and non-trivial (its floors on blocks, on the hits of every raycast that runs and, where no ray can hit, on
written voxels), the table holds the voxel-size mantissas it claims, and the switch between the fast and the IEEE sweep at mu = 2^-30 is
invisible in the reference's arithmetic."""
import numpy as np
import pytest

from oracle.binding import OraclePipeline
from tests.scale_frames import ALL_CASES, MU_BELOW_FAST, MU_FAST_MIN, NAMED, SEEDED, SWITCH_PAIRS, by_name, scale_stream, voxel_mantissa


def _run(case):
    """The case on the oracle: (blocks() + nodes(), hits of every raycast that ran, stats, the vertex and normal images of those raycasts)."""
    s = scale_stream(case)
    o = OraclePipeline(case["field"], case["N"], case["dim"], case["W"], case["H"])
    o.count_stats(True)
    hits, images = [], []
    try:
        for f in range(case["frames"]):
            pose = s.pose(f)
            assert o.integrate(s.depth(f), pose, s.k, case["mu"], f)
            ran, v, n = o.raycast(pose, s.k, case["mu"], f)
            assert ran == (f > 2)
            if ran:
                hits.append(int((n[..., 0] != -2).sum()))
                images += [v, n]
        return o.blocks() + o.nodes(), hits, o.stats(), images
    finally:
        o.close()


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_scale_case_is_well_posed_on_the_oracle(case):
    m, hits, st, _ = _run(case)
    blocks, written = len(m[0]), int((m[2] != 0).sum())
    print(case["name"], case["purpose"], "| blocks", blocks, "hits", hits, "written", written, st)
    assert st["truncated"] == 0 and st["oob_ub"] == 0, st
    assert blocks >= case["min_blocks"], blocks
    assert len(hits) == case["frames"] - 3 and min(hits) >= case["min_hits"], hits
    if case["min_hits"] == 0:
        assert case["min_written"] > 0 and written >= case["min_written"], written


def test_table_is_the_one_the_issue_of_scale_asks_for():
    """23 named cases and 16 seeded ones per field; floors everywhere; no hit floor of zero without a written-voxel floor."""
    assert len(NAMED) == 23 and len(SEEDED) == 32 and len({c["name"] for c in ALL_CASES}) == 55
    for c in ALL_CASES:
        assert c["min_blocks"] >= 20 and (c["min_hits"] >= 100 or c["min_written"] > 100000), c
        assert c["dim"] >= 0.4 and 0 < c["mu"] / (c["dim"] / c["N"]) < c["N"] / 16, c     # dim above the near plane; mu / voxel under the key reserve
    assert np.float32(MU_FAST_MIN) == np.float32(2.0 ** -30) and np.float32(MU_BELOW_FAST) < np.float32(MU_FAST_MIN)
    assert np.nextafter(np.float32(MU_BELOW_FAST), np.float32(1)) == np.float32(MU_FAST_MIN)


def test_voxel_sizes_have_many_mantissas_and_none_is_that_of_1_2():
    mantissas = {voxel_mantissa(c) for c in ALL_CASES}
    usual = int(np.float32(1.2).view(np.uint32)) & 0x7FFFFF
    assert voxel_mantissa(dict(dim=4.8, N=512)) == usual and voxel_mantissa(dict(dim=2.4, N=256)) == usual      # what every other stream has
    assert len(mantissas) >= 30, len(mantissas)
    assert usual not in mantissas
    assert 0 in mantissas                                 # the exact cases: voxel a power of two


@pytest.mark.parametrize("pair", SWITCH_PAIRS, ids=["sdf", "ofusion"])
def test_fast_sweep_switch_is_invisible_on_the_oracle(pair):
    """mu = 2^-30 and the float32 below it give bit-identical maps and raycasts on the oracle: whatever differs between them on the device is
    the switch of sweeps, not the arithmetic of the reference."""
    a, hits_a, _, img_a = _run(by_name(pair[0]))
    b, hits_b, _, img_b = _run(by_name(pair[1]))
    assert hits_a == hits_b and len(img_a) == len(img_b) == 6
    for u, v in zip(a + tuple(img_a), b + tuple(img_b)):
        assert u.shape == v.shape and (u.view(np.uint8) == v.view(np.uint8)).all()
