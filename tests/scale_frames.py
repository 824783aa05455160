"""The table of scales -- volume dimension, resolution and mu -- that tests/test_gpu_scales.py runs against the oracle, held to be well posed and
non-trivial by tests/test_scale_frames_oracle.py.

Every other stream of the suite fuses into a volume of 1.2, 2.4 or 4.8 m, so that with a power-of-two resolution the voxel size is always
1.2 * 2^j: voxel, inv_voxel, step, largestep, grad_scale, near / dim, far / dim, origin / dim + 1, the beam cell sizes, the leap spacing and
the sweep's R * (voxel, 0, 0) have had one float32 mantissa each, and mu / voxel has stayed between about 0.4 and 20.  Here the room stream of
supereight_amd/synthetic.py (``SyntheticStream(W, H, dim)``: the scene scales with dim, the near and far planes, 0.4 m and 4 m, do not) runs at
other volume dimensions and other mu.

``NAMED``: 80x60 images, 6 frames (raycasts at frames 3, 4 and 5), one case per regime.  ``SEEDED``: 16 (dim, N, mu) triples per field at
40x30 over 5 frames, drawn log-uniformly once and rounded to three significant digits, for mantissa diversity; literals, not a generator.

Each case lists the least number of blocks the oracle allocates and the least number of hits of every raycast that runs (about 90 % of what the
oracle gives: it is deterministic, the margin only absorbs a later change of the stream).  Cases with ``min_hits == 0`` compare "no hit
anywhere" on both sides; what keeps them non-vacuous is the block floor and ``min_written``, a floor on the voxels with y != 0.

Why no case goes higher in mu / voxel: the reference's allocation list holds (N / 8) * W * H keys, a first frame emits one key per band step,
and on overflow the reference drops keys in thread order.  On the oracle SDF truncates from mu / voxel of about N / 16, OFusion earlier (for
example at dim 1.0, 128^3, mu 0.02).  That regime is the reference's undefined behaviour, not a gap of this table.  Neither does the table hold
a dim below the near plane, or a mu near 2^30, where num_steps overflows int in the reference."""
from __future__ import annotations

import numpy as np

from oracle.binding import OFUSION, SDF
from supereight_amd.synthetic import SyntheticStream

W, H, FRAMES = 80, 60, 6
SEEDED_W, SEEDED_H, SEEDED_FRAMES = 40, 30, 5
SEEDED_MIN_BLOCKS, SEEDED_MIN_HITS = 20, 100

# se_hip_integrate takes the fast sweep for 2^-30 <= mu <= 2^30 and the IEEE sweep outside
MU_FAST_MIN = float(np.float32(2.0) ** -30)
MU_BELOW_FAST = float(np.nextafter(np.float32(MU_FAST_MIN), np.float32(0)))


def _case(name, field, dim, N, mu, purpose, blocks, hits, written=0):
    """blocks, hits, written: what the oracle gives (blocks after the last frame, the smallest raycast, voxels with y != 0; written only where
    hits == 0).  The floors are nine tenths of them; the pool of the pooled run is the next power of two above twice the block count."""
    return dict(name=name, W=W, H=H, frames=FRAMES, dim=dim, N=N, field=field, mu=mu, purpose=purpose, min_blocks=blocks * 9 // 10,
                min_hits=hits * 9 // 10, min_written=written * 9 // 10, pooled=1 << (2 * blocks).bit_length())


NAMED = [
    _case("sdf_d1.0_n128", SDF, 1.0, 128, 0.05, "voxel = 2^-7: every scale constant exact", 414, 4030),
    _case("sdf_d3.0_n256", SDF, 3.0, 256, 0.1, "another mantissa, everyday mu", 2006, 4552),
    _case("sdf_d5.0_n256", SDF, 5.0, 256, 0.1, "another mantissa", 1551, 3777),
    _case("sdf_d1.7_n256_band30", SDF, 1.7, 256, 0.1, "band 30 voxels, just under the key reserve", 2780, 4545),
    _case("sdf_d6.0_n512_band51", SDF, 6.0, 512, 0.3,
          "band 51 voxels: several SE_SCAN_SLOTS flushes per ray; back wall beyond far", 16688, 1043),
    _case("sdf_d2.0_n64_two_steps", SDF, 2.0, 64, 0.0333, "voxel = 2^-5, band * inv_voxel just above 2", 60, 499),
    _case("sdf_d0.77_n64_thin", SDF, 0.77, 64, 0.003,
          "band thinner than a voxel (num_steps = 1), march pinned at step; surfaces just past the near plane", 56, 826),
    _case("sdf_d3.0_n256_thin", SDF, 3.0, 256, 0.003, "band thinner than a voxel at 256^3", 778, 183),
    _case("sdf_d7.3_n128_far", SDF, 7.3, 128, 0.1, "most rays end at the far plane, side walls and sphere hit", 230, 443),
    _case("sdf_d40_n256_beyond_far", SDF, 40.0, 256, 0.5, "voxel 0.156 m; every surface beyond the far plane", 797, 0, written=283652),
    _case("sdf_d3.0_n256_mu_fast_min", SDF, 3.0, 256, MU_FAST_MIN, "last mu the fast sweep admits", 772, 0, written=176770),
    _case("sdf_d3.0_n256_mu_below_fast", SDF, 3.0, 256, MU_BELOW_FAST, "first mu that falls back to the IEEE sweep", 772, 0, written=176770),
    _case("of_d1.0_n128", OFUSION, 1.0, 128, 0.01, "exact constants", 419, 4065),
    _case("of_d3.0_n256", OFUSION, 3.0, 256, 0.02, "another mantissa, everyday mu", 1570, 4599),
    _case("of_d5.0_n256", OFUSION, 5.0, 256, 0.02, "fine step about band / 6", 1287, 3796),
    _case("of_d1.7_n256", OFUSION, 1.7, 256, 0.02, "another mantissa, band 9 voxels", 2106, 4607),
    _case("of_d6.0_n512_leap", OFUSION, 6.0, 512, 0.05, "leap over long empty stretches at 512^3", 10114, 1041),
    _case("of_d2.0_n64", OFUSION, 2.0, 64, 0.02, "N = 64: no fine beam grid, octants at levels 1-2", 61, 4585),
    _case("of_d0.77_n64", OFUSION, 0.77, 64, 0.01, "N = 64, surfaces just past the near plane", 63, 4114),
    _case("of_d7.3_n128_stages", OFUSION, 7.3, 128, 0.002, "6 * mu far below a voxel: stage switches inside the first step", 225, 562),
    _case("of_d40_n256_beyond_far", OFUSION, 40.0, 256, 0.15, "everything beyond far", 801, 0, written=344972),
    _case("of_d3.0_n256_mu_fast_min", OFUSION, 3.0, 256, MU_FAST_MIN, "last mu the fast sweep admits", 778, 4600),
    _case("of_d3.0_n256_mu_below_fast", OFUSION, 3.0, 256, MU_BELOW_FAST, "first mu that falls back to the IEEE sweep", 778, 4600),
]

# the two pairs on either side of the fast-sweep switch: (2^-30, the float32 below)
SWITCH_PAIRS = [("sdf_d3.0_n256_mu_fast_min", "sdf_d3.0_n256_mu_below_fast"), ("of_d3.0_n256_mu_fast_min", "of_d3.0_n256_mu_below_fast")]

SEEDED_TRIPLES = {
    SDF: [(1.26, 64, 0.0063), (1.13, 128, 0.00398), (0.892, 64, 0.00846), (4.42, 128, 0.184), (1.27, 64, 0.0338), (1.44, 128, 0.0303),
          (1.22, 64, 0.0367), (2.65, 128, 0.038), (4.99, 64, 0.0399), (1.95, 128, 0.015), (0.814, 64, 0.0133), (2.63, 128, 0.104),
          (2.63, 64, 0.0199), (3.41, 128, 0.024), (0.813, 64, 0.0201), (1.46, 128, 0.0525)],
    OFUSION: [(1.7, 64, 0.00428), (2.37, 128, 0.00263), (0.82, 64, 0.00115), (4.86, 128, 0.0299), (1.07, 64, 0.0013), (2.09, 128, 0.00117),
              (0.835, 64, 0.00417), (1.69, 128, 0.0072), (0.827, 64, 0.00083), (4.31, 128, 0.00528), (4.61, 64, 0.00526), (1.41, 128, 0.00111),
              (1.52, 64, 0.00303), (2.36, 128, 0.00395), (4.03, 64, 0.012), (3.95, 128, 0.00912)],
}

SEEDED = [dict(name=f"{'sdf' if field == SDF else 'of'}_d{dim}_n{N}_mu{mu}", W=SEEDED_W, H=SEEDED_H, frames=SEEDED_FRAMES, dim=dim, N=N, field=field,
               mu=mu, purpose="seeded mantissa", min_blocks=SEEDED_MIN_BLOCKS, min_hits=SEEDED_MIN_HITS, min_written=0, pooled=0)
          for field in (SDF, OFUSION) for dim, N, mu in SEEDED_TRIPLES[field]]

ALL_CASES = NAMED + SEEDED


def by_name(name):
    return next(c for c in NAMED if c["name"] == name)


def scale_stream(case):
    return SyntheticStream(case["W"], case["H"], case["dim"])


def voxel_mantissa(case) -> int:
    """The 23 mantissa bits of the float32 voxel size dim / N."""
    return int(np.float32(np.float32(case["dim"]) / np.float32(case["N"])).view(np.uint32)) & 0x7FFFFF
