"""Seeded cases for the bilateral filter and its exponential, shared by tests/test_exp_host.py (the definition so_exp_f32 against exp at 120
bits, on the CPU), tests/test_gpu_icp_math.py (se_exp_f32 on the device against so_exp_f32) and tests/test_gpu_bilateral.py (k_bilateral_filter
and the k_depth_pyramid pass behind it against the oracle).

  * exp_arguments()   -- arguments of so_exp_f32 / se_exp_f32, all <= 0 or NaN: the special values, the two ends of the float range of the result
                         (the smallest normal result, and 2^-150 where it rounds to 0 or to the smallest denormal), every -2^e, the odd multiples
                         of ln2 / 2 where rint changes k, the arguments the filter forms from millimetre depths, and a seeded sample;
  * exp_reference()   -- exp of them at 120 bits (mpmath), rounded once, half to even, to float32 with denormals;
  * SHAPES, images()  -- the filter's shapes (W, H) and the images filtered at each.
"""
from __future__ import annotations

import functools

import numpy as np

from tests.icp_edge_util import bits_around

LN2 = 0.693147180559945309417232121458
E_D_SQUARED_2 = np.float32(0.1) * np.float32(0.1) * np.float32(2)          # e_d * e_d * 2 of bilateralFilterKernel, in float32 as there


# ------------------------------------------------------------------------------------------------ the exponential
def workload_arguments(bases: int = 240) -> np.ndarray:
    """-((a - b) * (a - b)) / 0.02f in float32, as the kernel forms it, for millimetre-grid depths a, b in 0.4 .. 4.0 m with |a - b| <= 1.5 m:
    every difference on the millimetre grid at `bases` seeded base depths."""
    rng = np.random.default_rng(20251020)
    base_mm = np.unique(np.concatenate([[400, 401, 1000, 2047, 2048, 3999, 4000], rng.integers(400, 4001, bases)]))[:, None]
    other_mm = base_mm + np.arange(-1500, 1501)[None, :]
    keep = (other_mm >= 400) & (other_mm <= 4000)
    a = (np.broadcast_to(base_mm, other_mm.shape)[keep].astype(np.float32) / np.float32(1000.0)).astype(np.float32)     # mm2metersKernel: mm / 1000.0f
    b = (other_mm[keep].astype(np.float32) / np.float32(1000.0)).astype(np.float32)
    mod = (b - a) * (b - a)
    return (-mod / E_D_SQUARED_2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exp_arguments() -> np.ndarray:
    """Sorted ascending by value (-inf first, the zeros last), unique by bit pattern, and one NaN at the end."""
    f32 = np.float32
    parts = [np.asarray([0.0, -0.0, -np.inf, -3.4e38, -1e3], f32), bits_around(-104.0, 4)]
    parts += [bits_around(-87.33655, 64), bits_around(-103.97208, 64)]
    parts += [-np.exp2(np.arange(-149, 7, dtype=np.float64)).astype(f32)]
    parts += [bits_around(-(2 * j + 1) * LN2 / 2, 4) for j in range(0, 151) if (2 * j + 1) * LN2 / 2 <= 104.5]
    parts += [workload_arguments()]
    rng = np.random.default_rng(20251021)
    parts += [rng.uniform(-104.0, 0.0, 120_000).astype(f32), rng.uniform(-1.0, 0.0, 60_000).astype(f32),
              (-np.exp(rng.uniform(-40.0, np.log(104.0), 40_000))).astype(f32), rng.uniform(-104.0, -87.0, 30_000).astype(f32)]
    x = np.concatenate(parts).astype(f32)
    assert not np.isnan(x).any() and (x <= 0).all()
    x = np.unique(x.view(np.uint32)).view(f32)                  # by bit pattern: -0.0 and +0.0 both stay
    order = np.lexsort((np.signbit(x), x))                      # by value, -0.0 after +0.0 does not matter: both give 1
    x = np.concatenate([x[order], np.asarray([np.nan], f32)])
    x = np.ascontiguousarray(x, f32)
    x.setflags(write=False)
    return x


def round_to_f32(m) -> np.float32:
    """A non-negative mpmath number rounded once, half to even, to float32 -- denormals included (results here never overflow)."""
    import math

    import mpmath
    if m == 0:
        return np.float32(0)
    _, e = mpmath.frexp(m)                                      # m = f * 2^e, 0.5 <= f < 1
    q = max(int(e) - 24, -149)                                  # the exponent of the float's last place
    n = m / mpmath.mpf(2) ** q
    lo = int(mpmath.floor(n))
    frac = n - lo
    if frac > 0.5 or (frac == 0.5 and lo & 1):
        lo += 1
    return np.float32(math.ldexp(lo, q))                        # lo <= 2^24: exact


@functools.lru_cache(maxsize=None)
def exp_reference() -> np.ndarray:
    """exp(x) of exp_arguments() at 120 bits, rounded once to float32.  NaN gives NaN, -inf gives +0."""
    import mpmath
    x = exp_arguments()
    out = np.empty(x.size, np.float32)
    with mpmath.workprec(120):
        for i, v in enumerate(x.tolist()):
            if v != v:
                out[i] = np.nan
            elif v == -np.inf:
                out[i] = 0.0
            else:
                out[i] = round_to_f32(mpmath.exp(mpmath.mpf(v)))
    out.setflags(write=False)
    return out


# the Gaussian table exp(-x^2 / 32), x = -2 .. 2 (DenseSLAMSystem.cpp:111-118: radius 2, delta 4), correctly rounded, as float32 bit patterns
GAUSSIAN_BITS = (0x3F61EB51, 0x3F781FAB, 0x3F800000, 0x3F781FAB, 0x3F61EB51)
GAUSSIAN_ARGUMENTS = np.asarray([-(x * x) / np.float32(32.0) for x in range(-2, 3)], np.float32)


# ------------------------------------------------------------------------------------------------ the filter's shapes and images
# (W, H).  2x1 .. 5x3: the window is wider than the image, both clamps act on one pixel; 255 / 256 / 257: the last lane of one workgroup of 256,
# an exact fit, one lane of a second; 163x101 and 160x120: the scalar and the float4 path of the pyramid pass behind the filter.
SHAPES = ((2, 1), (2, 2), (3, 5), (5, 3), (4, 4), (8, 7), (255, 2), (256, 2), (257, 3), (163, 101), (160, 120))
E_DELTA = 0.1


def levels_of(W: int, H: int) -> int:
    """Pyramid levels to track with, three at the most: every level keeps at least one pixel a side (se_hip_track refuses more)."""
    n = 1
    while n < 3 and (W >> n) >= 1 and (H >> n) >= 1:
        n += 1
    return n


def mm_image(W: int, H: int, seed: int = 7, holes: float = 0.10) -> np.ndarray:
    """A seeded millimetre-grid image in 0.4 .. 4 m with `holes` zeros: mostly a smooth ramp with a few millimetres of noise (so that the range
    kernel's weights take every size), a quarter of the pixels anywhere in the range."""
    rng = np.random.default_rng(seed + 1000 * W + H)
    yy, xx = np.mgrid[0:H, 0:W]
    mm = 1200 + 7 * xx + 11 * yy + rng.integers(-40, 41, (H, W))
    wild = rng.random((H, W)) < 0.25
    mm = np.where(wild, rng.integers(400, 4001, (H, W)), mm)
    mm = np.clip(mm, 400, 4000)
    mm[rng.random((H, W)) < holes] = 0
    return (mm.astype(np.float32) / np.float32(1000.0)).astype(np.float32)


def images(W: int, H: int) -> dict:
    """name -> image (H, W) float32, the images of every shape.  The mirrored ones are images of their own: a mirrored window is summed in
    another order, so the filter of a mirror image is not the mirror image of the filter bit for bit, and each is compared with the oracle's
    output of that same image.  The constant is a power of two: every product weight * c is then exact, t = c * sum, and the output is the
    input whatever the weights are."""
    out = {}
    rnd = mm_image(W, H)
    out["random"] = rnd
    out["constant"] = np.full((H, W), 2.0, np.float32)
    out["zeros"] = np.zeros((H, W), np.float32)
    one = np.zeros((H, W), np.float32)
    one[H // 2, W // 2] = 1.732
    out["single"] = one
    v = np.full((H, W), 1.25, np.float32)
    v[:, (W + 1) // 2:] = 1.75                                    # a vertical edge: left 1.25, right 1.75
    h = np.full((H, W), 1.25, np.float32)
    h[(H + 1) // 2:, :] = 1.75                                    # a horizontal edge
    # on top of each step a few millimetres of seeded noise on the low side, so that the weights across rows and columns differ
    rng = np.random.default_rng(11 + W * 7 + H)
    noise = (rng.integers(0, 30, (H, W)).astype(np.float32) / np.float32(1000.0)).astype(np.float32)
    out["step_vertical"], out["step_horizontal"] = v + noise, h + noise
    out["mirror_lr"] = np.ascontiguousarray(rnd[:, ::-1])
    out["mirror_tb"] = np.ascontiguousarray(rnd[::-1, :])
    return out
