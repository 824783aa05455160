"""The scalar core of the device-resident ICP against the oracle where no scene takes it: se_sincos_f32, se_solve6_wave and se_icp_finalize
(strip and segment sums, solve, SE(3) exponential, pose product, convergence test), and the bilateral filter's se_exp_f32, of
supereight_amd/csrc/se_track_kernels.h, called
through tests/cpp/icp_math_check.hip on the argument lists of tests/icp_edge_util.py.  Everything is compared bit for bit; where the oracle's
value is a NaN the device's must be a NaN (payload and sign are not part of the contract).  tests/test_icp_math_host.py asserts, on the oracle
alone, that the lists reach what they are there for: every failing column of the factorisation, every quadrant of the sine, both small-angle
branches of the exponential on either side, the convergence test on either side of its threshold."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import oracle_exp, oracle_sincos
from tests import bilateral_util as B
from tests import icp_edge_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "cpp", "libse_icp_math_check.so")
SRC = os.path.join(ROOT, "tests", "cpp", "icp_math_check.hip")


def build_icp_math_check(force: bool = False) -> str:
    from supereight_amd import build as hb
    deps = [SRC, os.path.join(hb.SRC_DIR, "se_track_kernels.h"), os.path.join(hb.SRC_DIR, "se_device.h")]
    if force or not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run([hb.hipcc()] + hb.FLAGS + ["-o", SO, SRC], check=True, capture_output=True)
    return SO


@pytest.fixture(scope="module")
def chk():
    from supereight_amd.pipeline import load_library
    load_library()      # (one HIP runtime per process: see pipeline._share_torch_hip_runtime)
    lib = C.CDLL(build_icp_math_check())
    f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    lib.se_icp_math_sincos.argtypes = [f32p, C.c_int, f32p, f32p]
    lib.se_icp_math_exp.argtypes = [f32p, C.c_int, f32p]
    lib.se_icp_math_solve6.argtypes = [f32p, C.c_int, f32p, i32p]
    lib.se_icp_math_finalize.argtypes = [f32p, f32p, f32p, C.c_int, f32p, f32p, i32p]
    assert lib.se_icp_math_segments() == U.SEGMENTS
    return lib


def _first_bad(same, *columns):
    i = int(np.flatnonzero(~same.reshape(len(same), -1).all(axis=1))[0])
    return (i,) + tuple(c[i] for c in columns)


def test_sine_and_cosine_in_every_quadrant(chk):
    x = U.sincos_arguments()
    s_c, c_c = oracle_sincos(x)
    s_g, c_g = np.full_like(x, np.nan), np.full_like(x, np.nan)
    assert chk.se_icp_math_sincos(x, x.size, s_g, c_g) == 0
    same = U.same_bits(s_g, s_c) & U.same_bits(c_g, c_c)
    print(f"{x.size} arguments, {(~same).sum()} differ")
    assert same.all(), _first_bad(same, x, s_g, s_c, c_g, c_c)


def test_exponential_of_the_bilateral_filter(chk):
    """se_exp_f32 on the device against so_exp_f32 on every argument tests/test_exp_host.py holds the definition to: the ends of the float
    range of the result, denormal results, every scale 2^k, the filter's own arguments, NaN."""
    x = B.exp_arguments()
    e_c = oracle_exp(x)
    e_g = np.full_like(x, -1.0)
    assert chk.se_icp_math_exp(x, x.size, e_g) == 0
    same = U.same_bits(e_g, e_c)
    print(f"{x.size} arguments, {(~same).sum()} differ")
    assert same.all(), _first_bad(same, x, e_g, e_c)


def test_wave_solve_gives_up_where_the_oracle_does(chk):
    vals, _ = U.solve_systems()
    x_c, col = U.oracle_solve_all(vals)
    x_g = np.full((len(vals), 6), np.nan, np.float32)
    agree = np.zeros(len(vals), np.int32)
    assert chk.se_icp_math_solve6(vals, len(vals), x_g, agree) == 0
    same = U.same_bits(x_g, x_c)
    print(f"{len(vals)} systems, failing columns {np.bincount(col, minlength=7).tolist()}, {(~same.all(axis=1)).sum()} differ")
    assert same.all(), _first_bad(same, col, vals, x_g, x_c)
    assert (agree == 1).all(), np.flatnonzero(agree != 1)[:8]           # "x: the solution, in every lane"


def test_finalize_sums_solves_and_updates_the_pose(chk):
    fc = U.finalize_cases()
    ref = U.finalize_reference(fc["partial"], fc["pose"], fc["thr"])
    n = len(fc["thr"])
    strip0, pose = np.full((n, 32), np.nan, np.float32), np.full((n, 16), np.nan, np.float32)
    conv = np.full(n, -1, np.int32)
    assert chk.se_icp_math_finalize(fc["partial"].reshape(-1), fc["pose"].reshape(-1), fc["thr"], n, strip0.reshape(-1), pose.reshape(-1), conv) == 0
    same = U.same_bits(strip0, ref["strip0"])
    assert same.all(), _first_bad(same, strip0, ref["strip0"])
    same = U.same_bits(pose, ref["pose"])
    print(f"{n} cases ({fc['n_twists']} twists), {(~same.all(axis=1)).sum()} poses differ, conv differs on {(conv != ref['conv']).sum()}")
    assert same.all(), _first_bad(same, ref["x"], pose, ref["pose"])
    assert (conv == ref["conv"]).all(), _first_bad(conv == ref["conv"], ref["norm"], fc["thr"], conv, ref["conv"])
