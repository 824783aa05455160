"""Segment traces, host side (no GPU): the header declares both entries, the output struct and the bound; the build lists the kernel header;
the Python truths (tests/trace_util.py: the integer DDA and the literal enumeration) agree with each other on every segment family and give
the hand-worked answers; the host restatement (include/se/segment_trace.hpp) gives them too and its walk equals its literal definition on
random maps with absent octants, also under AddressSanitizer and UBSan; the metric-to-fixed-point rules; the argument refusals of trace and
view_gain; and the seeded segment set of the GPU test holds every kind of segment on the map that test uses."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.golden_util import load
from tests.host_util import ROOT, bare_pipeline, build_kats
from tests.trace_util import (EMPTY, FREE, HAND_CASES, INVALID, KINDS, LIMIT, NONE, OCC, SUB, UNSEEN, census, degenerate, grids_from_octree,
                              hand_grids, seeded_segments, trace_literal_truth, trace_truth, valid)


def test_header_declares_the_trace_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_trace_segments(se_hip_pipeline* p, const int32_t* device_segments, int64_t n, const se_hip_collide_test* test, int32_t stop_at, "
            "const se_hip_trace_out* device_out);") in flat
    assert ("int se_hip_trace_segments_host(se_hip_pipeline* p, const int32_t* host_segments, int64_t n, const se_hip_collide_test* test, int32_t stop_at, "
            "const se_hip_trace_out* host_out);") in flat
    body = re.search(r"typedef struct se_hip_trace_out \{(.*?)\} se_hip_trace_out;", h, re.S).group(1)
    assert re.findall(r"(uint8_t|float|int32_t)\* (\w+);", body) == [("uint8_t", "status"), ("float", "t_first"), ("int32_t", "first"), ("int32_t", "counts")]
    assert "#define SE_HIP_SEGMENT_LIMIT (1 << 22)" in h and "2^47" in h
    assert "#define SE_HIP_K_COUNT 5" in h           # no new launch counter
    from supereight_amd import pipeline as P
    assert P.SEGMENT_LIMIT == LIMIT and P.ORIENTED_SUB == SUB and P.TRACE_NONE == NONE[0]
    assert [f[0] for f in P._TraceOut._fields_] == ["status", "t_first", "first", "counts"]
    for name in ("se_hip_trace_segments", "se_hip_trace_segments_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 6 and args[2] is C.c_int64 and args[4] is C.c_int32


def test_build_lists_the_trace_kernel_header():
    from supereight_amd import build
    assert "se_trace_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_trace_kernels.h"' in src
    k = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_trace_kernels.h")).read()
    assert "k_trace_segments" in k and "bounded" in k           # the header comment states why the walk ends


# ------------------------------------------------------------------ the truths
def test_python_truths_give_the_hand_answers():
    grids = hand_grids()
    for name, (mp, a, b, occ, uns) in HAND_CASES.items():
        seg = list(a) + list(b)
        assert trace_truth(grids[mp], seg, OCC) == occ and trace_truth(grids[mp], seg, UNSEEN) == uns, name
        if max(abs(c) for c in seg) < 4096:
            assert trace_literal_truth(grids[mp], seg, OCC) == occ and trace_literal_truth(grids[mp], seg, UNSEEN) == uns, name


def test_dda_equals_the_literal_definition_on_every_family():
    rng = np.random.default_rng(1)
    grid = rng.choice(np.array([OCC, UNSEEN, EMPTY, EMPTY, EMPTY, EMPTY, EMPTY, EMPTY], np.uint8), (32, 32, 32))
    grid[8:24, 8:24, 8:24] = EMPTY
    grid[12:14, 12:20, 10:20] = UNSEEN
    segs = [s for s in seeded_segments(grid, 3).tolist() if not valid(s) or max(abs(s[k] - s[3 + k]) for k in range(3)) <= 14 * SUB]
    assert len(segs) > 400
    seen = set()
    for s in segs:
        for stop in (OCC, UNSEEN):
            t = trace_truth(grid, s, stop)
            assert t == trace_literal_truth(grid, s, stop), (s, stop)
            seen.add((t[0], t[1] == FREE))
    assert {(OCC, False), (UNSEEN, False), (UNSEEN, True), (EMPTY, True), (INVALID, False)} <= seen


# ------------------------------------------------------------------ the host restatement
def _parse(stdout):
    got = {}
    for f in (line.split() for line in stdout.splitlines()):
        v = [int(t) for t in f[1:]]
        got[f[0]] = (v[0], [(v[1 + 8 * s], Fraction(v[2 + 8 * s], v[3 + 8 * s]), tuple(v[4 + 8 * s:7 + 8 * s]), tuple(v[7 + 8 * s:9 + 8 * s])) for s in range(2)],
                     [(v[2 + 8 * s], v[3 + 8 * s]) for s in range(2)])
    return got


def test_hand_cases_on_the_host_mirror(tmp_path):
    """The program itself ends with 1 if the walk with and without counts, or the walk and the literal definition, differ on a case."""
    exe = build_kats("trace_kats", tmp_path)
    r = subprocess.run([exe, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _parse(r.stdout)
    assert sorted(got) == sorted(HAND_CASES)
    for name, (_, _, _, occ, uns) in HAND_CASES.items():
        is_valid, answers, terms = got[name]
        assert is_valid == (occ[0] != INVALID), name
        assert answers == [occ, uns], (name, answers)
        assert terms == [(occ[1].numerator, occ[1].denominator), (uns[1].numerator, uns[1].denominator)], name      # lowest terms


def test_walk_equals_the_definition_on_random_maps(tmp_path):
    exe = build_kats("trace_kats", tmp_path)
    r = subprocess.run([exe, "random", "14", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    assert f[0] == "checked" and int(f[1]) == 4200 and f[2] == "mismatches" and int(f[3]) == 0


def test_host_mirror_is_clean_under_the_sanitizers(tmp_path):
    """The same program, stand-alone, with AddressSanitizer and UBSan compiled in: host code with its own main, run directly."""
    exe = str(tmp_path / "trace_kats_san")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "trace_kats.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for args in (["kats"], ["random", "4", "3"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_cpp_mirror_trace_program_compiles(tmp_path):
    """tests/cpp/trace_mirror.cpp (run on the GPU by test_gpu_trace_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"tm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "trace_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ metric to fixed point
def test_segments_from_points_rounds_to_odd_sub_units():
    from supereight_amd.pipeline import segments_from_points
    rng = np.random.default_rng(5)
    dim, size = 4.8, 512
    a, b = rng.uniform(-1.0, dim + 1.0, (4000, 3)), rng.uniform(-1.0, dim + 1.0, (4000, 3))
    a[:500] = np.round(a[:500] * size / dim) * dim / size          # on voxel boundaries
    b[:1500, 1:] = a[:1500, 1:]                                    # parallel to x, a third of them in a grid plane before the rounding
    seg = segments_from_points(a, b, dim, size)
    assert seg.dtype == np.int32 and seg.shape == (4000, 6) and seg.flags.c_contiguous
    assert (seg % 2 != 0).all()
    exact = np.concatenate([a, b], 1) * (SUB * size / dim)
    assert (np.abs(seg - exact) <= 1.0 + 1e-9).all() and (np.abs(seg - exact) > 0.9).any()
    assert not any(degenerate(s) for s in seg.tolist())
    assert (seg[:1500, 1:3] == seg[:1500, 4:6]).all()             # still axis-parallel
    huge = segments_from_points(np.array([[1e12, -1e12, 0.0]]), np.array([[0.0, 0.0, 0.0]]), dim, size)
    assert huge[0, 0] == 2 ** 31 - 1 and huge[0, 1] == -(2 ** 31 - 1) and huge[0, 2] == 1
    for bad in ((np.zeros((2, 2)), np.zeros((2, 2))), (np.zeros((2, 3)), np.zeros((3, 3))), (np.full((1, 3), np.nan), np.zeros((1, 3)))):
        with pytest.raises(ValueError):
            segments_from_points(bad[0], bad[1], dim, size)
    with pytest.raises(ValueError):
        segments_from_points(np.zeros((1, 3)), np.zeros((1, 3)), 0.0, size)


def _look(eye, target):
    z = np.asarray(target, float) - np.asarray(eye, float)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def test_view_segments_stay_inside_the_cube_and_report_the_misses():
    from supereight_amd.pipeline import view_segments
    dim, size, k = 4.8, 512, (300.0, 300.0, 159.5, 119.5)
    S = SUB * size
    inside, missed = view_segments(_look([2.4, 2.4, 2.0], [4.0, 3.0, 1.5]), k, 320, 240, 8, 0.4, 4.0, dim, size)
    assert len(missed) == 0 and inside.shape == (40 * 30, 6) and inside.dtype == np.int32
    assert (inside > 0).all() and (inside < S).all() and (inside % 2 != 0).all()
    # the centre ray: from the eye + 0.4 along the axis
    mid = inside[15 * 40 + 20]
    axis = np.array([1.6, 0.6, -0.5]) / np.linalg.norm([1.6, 0.6, -0.5])
    assert (np.abs(mid[0:3] - (np.array([2.4, 2.4, 2.0]) + 0.4 * axis) * S / dim) < 3).all()
    # an eye outside the cube looking along its face: some rays enter and are clipped to it, the others are reported
    part, missed = view_segments(_look([-1.0, 2.4, 2.4], [1.0, 6.0, 2.4]), k, 320, 240, 8, 0.4, 6.0, dim, size)
    assert 0 < len(missed) < 1200 and len(part) + len(missed) == 1200 and len(np.unique(missed)) == len(missed)
    assert (part > 0).all() and (part < S).all()
    away, missed = view_segments(_look([-1.0, 2.4, 2.4], [-3.0, 2.4, 2.4]), k, 320, 240, 8, 0.4, 6.0, dim, size)
    assert away.shape == (0, 6) and (missed == np.arange(1200)).all()
    for bad in (dict(stride=0), dict(near=2.0, far=1.0), dict(near=-0.1), dict(k=(0.0, 300.0, 1.0, 1.0)), dict(width=0), dict(far=float("inf"))):
        kw = dict(pose=np.eye(4), k=k, width=320, height=240, stride=8, near=0.4, far=4.0, dim=dim, size=size)
        kw.update(bad)
        with pytest.raises(ValueError):
            view_segments(**kw)


# ------------------------------------------------------------------ the argument refusals
def _pipeline():
    return bare_pipeline(field=0, dim=4.8, size=512, _device=0)


@pytest.mark.parametrize("segments,exc", [
    (np.zeros((4, 6), np.int64), TypeError),
    (np.zeros((4, 6), np.float32), TypeError),
    (np.zeros((4, 9), np.int32), ValueError),
    (np.zeros(24, np.int32), ValueError),
    (np.zeros((2, 2, 6), np.int32), ValueError),
    ([[0, 0, 0, 1, 1, 1]], TypeError),
    (None, TypeError),
], ids=["int64", "float32", "n_by_9", "flat", "3d", "list", "none"])
def test_trace_refuses_bad_segments_before_any_library_call(segments, exc):
    with pytest.raises(exc):
        _pipeline().trace(segments)


def test_trace_and_view_gain_refuse_bad_arguments_before_any_library_call():
    p = _pipeline()
    ok = np.zeros((4, 6), np.int32)
    for kw, exc in ((dict(stop_at="empty"), ValueError), (dict(stop_at=0), ValueError), (dict(threshold=float("nan")), ValueError),
                    (dict(threshold=1e39), ValueError), (dict(occupied_above=2), TypeError), (dict(occupied_above="yes"), TypeError)):
        with pytest.raises(exc):
            p.trace(ok, **kw)
    poses, k = np.eye(4)[None], (300.0, 300.0, 159.5, 119.5)
    for args, kw, exc in (((np.eye(4), k, 320, 240), {}, ValueError), ((np.zeros((2, 3, 4)), k, 320, 240), {}, ValueError),
                          ((poses, (300.0, 0.0, 1.0, 1.0), 320, 240), {}, ValueError), ((poses, k, 320, 0), {}, ValueError),
                          ((poses, k, 320, 240), dict(stride=0), ValueError), ((poses, k, 320, 240), dict(near=3.0, far=1.0), ValueError),
                          ((poses, k, 320, 240), dict(threshold=float("inf")), ValueError), ((poses, k, 320, 240), dict(occupied_above=1), TypeError),
                          ((poses, k, 320, 240), dict(device=1), TypeError), ((np.full((1, 4, 4), np.nan), k, 320, 240), {}, ValueError)):
        with pytest.raises(exc):
            p.view_gain(*args, **kw)


def test_trace_refuses_bad_torch_segments():
    torch = pytest.importorskip("torch")
    p = _pipeline()
    with pytest.raises(TypeError):
        p.trace(torch.zeros((4, 6), dtype=torch.int64))
    with pytest.raises(ValueError):
        p.trace(torch.zeros((4, 5), dtype=torch.int32))
    with pytest.raises(ValueError):
        p.trace(torch.zeros((6, 4), dtype=torch.int32).t())          # [4, 6], not contiguous
    with pytest.raises(ValueError):
        p.trace(torch.zeros((4, 6), dtype=torch.int32))              # a CPU tensor: the device entry reads device memory


# ------------------------------------------------------------------ the GPU test's segment set is not vacuous
def test_seeded_set_holds_every_kind_of_segment():
    """On the map of tests/test_gpu_trace.py -- the first two frames of the golden room fixture, rebuilt here through the oracle -- the seeded
    set has at least 16 segments of each kind, by the truth alone."""
    from oracle.binding import OraclePipeline
    from tests.trace_util import SEED
    g = load("sdf_80x60_128.npz")
    W, H, N, _ = (int(v) for v in g["dims"])
    o = OraclePipeline(0, N, float(g["dim"]), W, H)
    for f in range(2):
        o.integrate(g["depth"][f], g["pose"][f], g["k"], float(g["mu"]), f)
    grid, side_of = grids_from_octree(N, o.blocks(), o.nodes(), (1.0, 0.0), 0.0, False)
    o.close()
    assert {OCC, UNSEEN, EMPTY} <= set(np.unique(grid).tolist()) and (side_of >= 32).any()
    segs = seeded_segments(grid, SEED)
    assert 1800 <= len(segs) <= 2400
    _, kinds = census(grid, segs, side_of)
    assert all(kinds[k] >= 16 for k in KINDS), kinds
