"""Oriented box collision queries, host side (no GPU): the predicate -- numpy truth (tests/oriented_util.py) and host restatement
(include/se/oriented_collision.hpp) alike -- against a definition that uses no separating axis, in exact rationals; the hand-worked cases; the
host traversal against the literal definition on random maps; the rounding helper; the Python argument checks; the header text and the build
list."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.host_util import bare_pipeline, build_kats
from tests.oriented_util import (BRUTE_CASES, C_LIMIT, H_LIMIT, HAND_CASES, INVALID, SUB, aligned_boxes, bounding_boxes, hand_box, oriented_hand_grid,
                                 oriented_truth, random_rotations, shuffled_axes, touched, valid)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the rational definition
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def rational_touched(box, v, s):
    """Whether the open box meets the open cube (corner v, side s in voxels), without a separating axis: the vertices of
    closed box ∩ closed cube are the box vertices in the cube, the cube vertices in the box, and the crossings of the edges of one with the
    face planes of the other that lie in both; the open sets meet iff that set is non-empty and its mean lies strictly inside both.  (The
    intersection of the closed sets is the convex hull of those points; its interior is the intersection of the two open sets, and the mean
    of the vertices of a polytope with an interior lies in it.)  Points are exact rationals (X / w: integer X, integer w > 0), in doubled
    sub-units; the mean is a Fraction."""
    b = [int(t) for t in box]
    c2 = tuple(2 * t for t in b[0:3])
    h = [tuple(b[3 + 3 * i:6 + 3 * i]) for i in range(3)]
    lo = tuple(2 * SUB * int(t) for t in v)
    side = 2 * SUB * int(s)
    hi = tuple(t + side for t in lo)
    normals = [_cross(h[1], h[2]), _cross(h[2], h[0]), _cross(h[0], h[1])]
    det2 = 2 * abs(_dot(h[0], normals[0]))                  # |n_i . (x - 2c)| <= 2 |det| on the closed box (n_i . 2 h_i = +-2 det)
    assert det2 != 0

    def in_cube(X, w, strict):
        return all((lo[k] * w < X[k] < hi[k] * w) if strict else (lo[k] * w <= X[k] <= hi[k] * w) for k in range(3))

    def in_box(X, w, strict):
        r = tuple(X[k] - c2[k] * w for k in range(3))
        return all((abs(_dot(n, r)) < det2 * w) if strict else (abs(_dot(n, r)) <= det2 * w) for n in normals)

    pts = []

    def add(X, w):
        if w < 0:
            X, w = tuple(-t for t in X), -w
        if in_cube(X, w, False) and in_box(X, w, False):
            pts.append((X, w))

    signs = [(a, b_, c_) for a in (-1, 1) for b_ in (-1, 1) for c_ in (-1, 1)]
    for sg in signs:                                        # the vertices of both
        add(tuple(c2[k] + 2 * (sg[0] * h[0][k] + sg[1] * h[1][k] + sg[2] * h[2][k]) for k in range(3)), 1)
        add(tuple(hi[k] if sg[k] > 0 else lo[k] for k in range(3)), 1)
    for i in range(3):                                      # box edges (along h_i, from s_i = -1 to +1) x cube face planes x_k = p
        j, l = (i + 1) % 3, (i + 2) % 3
        D = tuple(4 * t for t in h[i])
        for sj in (-1, 1):
            for sl in (-1, 1):
                A = tuple(c2[k] + 2 * (-h[i][k] + sj * h[j][k] + sl * h[l][k]) for k in range(3))
                for k in range(3):
                    if D[k] == 0:
                        continue
                    for p in (lo[k], hi[k]):
                        num = p - A[k]                      # t = num / D[k]
                        if (num >= 0 and num <= D[k]) if D[k] > 0 else (num <= 0 and num >= D[k]):
                            add(tuple(A[m] * D[k] + num * D[m] for m in range(3)), D[k])
    for k in range(3):                                      # cube edges (along e_k) x box face planes n . (x - 2c) = +-2 |det|
        j, l = (k + 1) % 3, (k + 2) % 3
        for pj in (lo[j], hi[j]):
            for pl in (lo[l], hi[l]):
                B = [0, 0, 0]
                B[k], B[j], B[l] = lo[k], pj, pl
                for n in normals:
                    nE = n[k] * side
                    if nE == 0:
                        continue
                    base = _dot(n, tuple(B[m] - c2[m] for m in range(3)))
                    for q in (-det2, det2):
                        num = q - base                      # t = num / nE
                        if (num >= 0 and num <= nE) if nE > 0 else (num <= 0 and num >= nE):
                            X = [B[m] * nE for m in range(3)]
                            X[k] += num * side
                            add(tuple(X), nE)
    if not pts:
        return False
    mean = [sum(Fraction(X[k], w) for X, w in pts) / len(pts) for k in range(3)]
    W = 1
    for f in mean:
        W *= f.denominator
    Xm = tuple(int(f * W) for f in mean)
    assert all(Fraction(Xm[k], W) == mean[k] for k in range(3))
    return in_cube(Xm, W, True) and in_box(Xm, W, True)


def _exact_rotation(rng):
    """A 3-4-5 or 5-12-13 rotation about one axis, as integer columns and their common length."""
    a, b, r = ((3, 4, 5), (5, 12, 13))[int(rng.integers(0, 2))]
    if rng.integers(0, 2):
        a, b = b, a
    if rng.integers(0, 2):
        a = -a
    k = int(rng.integers(0, 3))
    i, j = (k + 1) % 3, (k + 2) % 3
    cols = np.zeros((3, 3), np.int64)      # cols[axis] = that half-axis direction times r
    cols[k, k] = r
    cols[i, i], cols[i, j] = a, b
    cols[j, i], cols[j, j] = -b, a
    return cols


def _pairs(rng, n):
    """n box / cube pairs, a quarter each of: general skew; axis-permuted boxes with faces on voxel boundaries; exact 3-4-5 / 5-12-13
    rotations about one axis; one half-axis parallel to a cube edge.  Cube sides 1, 2, 4, the cube near the box's surface."""
    out = []
    while len(out) < n:
        kind = len(out) % 4
        c = rng.integers(-40 * SUB, 40 * SUB, 3)
        if kind == 0:
            h = rng.integers(-3 * SUB, 3 * SUB + 1, (3, 3))
        elif kind == 1:
            side = rng.integers(1, 7, 3)
            lo = rng.integers(-20, 20, 3)
            c = SUB * lo + (SUB // 2) * side
            h = np.diag((SUB // 2) * side)[rng.permutation(3)] * rng.choice([-1, 1], (3, 1))
        elif kind == 2:
            h = _exact_rotation(rng) * rng.integers(1, 8, (3, 1))
        else:
            h = rng.integers(-3 * SUB, 3 * SUB + 1, (3, 3))
            h[0] = 0
            h[0, int(rng.integers(0, 3))] = int(rng.integers(1, 4 * SUB)) * int(rng.choice([-1, 1]))
        box = np.concatenate([c, h.reshape(-1)]).astype(np.int64)
        if not valid(box):
            continue
        s = int((1, 2, 4)[int(rng.integers(0, 3))])
        # a cube whose centre is near a point of the box's closure or just beyond it
        t = rng.uniform(-1.3, 1.3, 3)
        if kind == 1 or rng.random() < 0.3:
            t = np.where(rng.random(3) < 0.5, np.sign(t), t)      # on the faces
        q = (c + t @ h) / SUB
        v = np.floor(q - s / 2 + rng.uniform(-0.5, 0.5, 3)).astype(np.int64)
        if kind == 1 and rng.random() < 0.5:
            v = np.rint(q).astype(np.int64) - rng.integers(0, 2, 3) * s       # shares boundary planes with the box
        out.append((box, v, s))
    return out


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    return build_kats("oriented_kats", tmp_path_factory.mktemp("oriented_kats"))


def test_predicate_equals_the_rational_definition(kats):
    rng = np.random.default_rng(1507)
    pairs = _pairs(rng, 1000)
    truth = [rational_touched(b, v, s) for b, v, s in pairs]
    for kind in range(4):
        assert 25 <= sum(truth[kind::4]) <= 225, (kind, sum(truth[kind::4]))       # both outcomes in every quarter
    assert sum(truth) >= 100 and len(truth) - sum(truth) >= 100
    got = [touched(b, v, s) for b, v, s in pairs]
    bad = [i for i in range(len(pairs)) if got[i] != truth[i]]
    assert not bad, (bad[:5], [pairs[i] for i in bad[:3]])
    # the host restatement's predicate on the same pairs
    text = "".join(" ".join(str(int(t)) for t in list(b) + list(v) + [s]) + "\n" for b, v, s in pairs)
    r = subprocess.run([kats, "pairs"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    host = [t == "1" for t in r.stdout.split()]
    assert host == truth
    # the same sets, whatever the order and the signs of the half-axes
    boxes = np.stack([b for b, _, _ in pairs]).astype(np.int32)
    again = shuffled_axes(rng, boxes)
    assert [touched(again[i], pairs[i][1], pairs[i][2]) for i in range(len(pairs))] == truth


def test_rational_definition_on_cases_worked_by_hand():
    unit = [8, 8, 8, 8, 0, 0, 0, 8, 0, 0, 0, 8]                 # the voxel (0, 0, 0) itself
    assert rational_touched(unit, (0, 0, 0), 1) and touched(unit, (0, 0, 0), 1)
    for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (1, 1, 1), (0, 0, -1)):          # shares a face, an edge or a vertex only
        assert not rational_touched(unit, v, 1) and not touched(unit, v, 1)
    assert rational_touched(unit, (-1, -1, -1), 2) and rational_touched(unit, (0, 0, 0), 4) and not rational_touched(unit, (1, 0, 0), 4)
    diamond = hand_box("DiamondVertexOnCorner")
    assert not rational_touched(diamond, (10, 10, 10), 1) and rational_touched(diamond, (9, 10, 10), 1) and rational_touched(diamond, (9, 9, 10), 1)
    assert rational_touched(hand_box("DiamondVertexInside"), (10, 10, 10), 1)
    assert rational_touched(hand_box("ThinPlate"), (10, 10, 10), 1) and not rational_touched(hand_box("SkewMisses"), (10, 10, 10), 1)


def test_numpy_truth_gives_the_hand_answers():
    from tests.oriented_util import OCC, bounding_voxels
    for name in BRUTE_CASES:
        mp, status, bound = HAND_CASES[name][0], HAND_CASES[name][5], HAND_CASES[name][6]
        grid = oriented_hand_grid(mp)
        assert oriented_truth(grid, hand_box(name)) == status, name
        if bound is not None:                                  # the strict status of the bounding axis-aligned box
            b = bounding_boxes(np.array([hand_box(name)]))[0].astype(np.int64)
            lo, hi = b[0:3], b[0:3] + b[3:6]
            inside = (lo >= 0).all() and (hi <= 64).all()
            i0, i1 = np.clip(lo, 0, 64), np.clip(hi, 0, 64)
            cells = grid[i0[2]:i1[2], i0[1]:i1[1], i0[0]:i1[0]]
            got = min(int(cells.min()) if cells.size else 2, 2 if inside else 1)
            assert got == bound, name
    # the diamond's bounding box reports a collision that is not there
    assert HAND_CASES["DiamondMissesCorner"][5] != OCC and HAND_CASES["DiamondMissesCorner"][6] == OCC
    lo, hi = bounding_voxels(hand_box("DiamondMissesCorner"))
    assert (lo == (3, 3, 10)).all() and (hi == (11, 11, 11)).all()


def test_numpy_truth_of_aligned_boxes_is_the_half_open_box():
    rng = np.random.default_rng(4)
    grid = rng.choice(np.array([0, 1, 2, 2, 2, 2, 2, 2], np.uint8), (32, 32, 32))
    o, ls = aligned_boxes(rng, 200, 32, max_side=5)
    for box, b in zip(o.tolist(), ls.astype(np.int64)):
        lo, hi = b[0:3], b[0:3] + b[3:6]
        i0, i1 = np.clip(lo, 0, 32), np.clip(hi, 0, 32)
        cells = grid[i0[2]:i1[2], i0[1]:i1[1], i0[0]:i1[0]] if (i0 < i1).all() else np.zeros(0, np.uint8)
        want = min(int(cells.min()) if cells.size else 2, 2 if ((lo >= 0).all() and (hi <= 32).all()) else 1)
        assert oriented_truth(grid, box) == want


def test_hand_cases_on_the_host_mirror(kats):
    """The program itself ends with 1 if the traversal and the brute-force definition differ on a case."""
    r = subprocess.run([kats, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = {f[0]: int(f[1]) for f in (line.split() for line in r.stdout.splitlines())}
    assert sorted(got) == sorted(HAND_CASES)
    for name, case in HAND_CASES.items():
        assert got[name] == case[5], (name, got[name])
    # the cases of the program are the cases of oriented_util
    src = open(os.path.join(ROOT, "tests", "cpp", "oriented_kats.cpp")).read()
    sym = {"CL": C_LIMIT, "HL": H_LIMIT, "MIN": -(1 << 31)}
    for name in HAND_CASES:
        m = re.search(r'\{"%s", "(\w+)", \{([^}]*)\}\}' % name, src)
        vals = [eval(t, {}, sym) for t in m.group(2).split(",")]
        assert m.group(1) == HAND_CASES[name][0] and vals == hand_box(name), name


def test_traversal_equals_the_definition_on_random_maps(kats):
    r = subprocess.run([kats, "random", "26", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    res = dict(zip(f[0::2], (int(t) for t in f[1::2])))
    assert res["checked"] == 10400 and res["mismatches"] == 0
    assert res["occupied"] > 500 and res["unseen"] > 500 and res["empty"] > 500


def test_cpp_mirror_oriented_program_compiles(tmp_path):
    """tests/cpp/oriented_mirror.cpp (run on the GPU by test_gpu_oriented_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"om_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "oriented_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------------- the rounding helper
def test_oriented_boxes_rounds_to_the_nearest_sub_unit():
    from supereight_amd.pipeline import ORIENTED_SUB, oriented_boxes
    assert ORIENTED_SUB == SUB
    dim, size = 4.8, 256
    scale = SUB * size / dim
    rng = np.random.default_rng(12)
    n = 500
    c = rng.uniform(-0.5, dim + 0.5, (n, 3))
    R = random_rotations(rng, n)
    e = rng.uniform(0.01, 0.3, (n, 3))
    b = oriented_boxes(c, R, e, dim, size)
    assert b.dtype == np.int32 and b.shape == (n, 12)
    assert np.abs(b[:, 0:3] - c * scale).max() <= 0.5
    for i in range(3):
        assert np.abs(b[:, 3 + 3 * i:6 + 3 * i] - R[:, :, i] * e[:, i:i + 1] * scale).max() <= 0.5
    # every point of the rounded box within sqrt(3) / 8 voxel of the corresponding point of the box asked for
    corners = np.array([[1, a, b_, c_] for a in (-1, 1) for b_ in (-1, 1) for c_ in (-1, 1)], np.float64)
    exact = np.concatenate([c * scale] + [R[:, :, i] * e[:, i:i + 1] * scale for i in range(3)], 1).reshape(n, 4, 3)
    moved = np.einsum("vj,njk->nvk", corners, b.reshape(n, 4, 3) - exact)
    assert np.linalg.norm(moved, axis=2).max() / SUB <= np.sqrt(3) / 8
    # an axis-aligned metric box on voxel boundaries comes out exactly
    one = oriented_boxes([[0.3, 0.6, 0.9]], [np.eye(3)], [[0.15, 0.075, 0.3]], 4.8, 256)
    assert one.tolist() == [[256, 512, 768, 128, 0, 0, 0, 64, 0, 0, 0, 256]]
    assert oriented_boxes(np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)), 4.8, 256).shape == (0, 12)
    far = oriented_boxes([[1e9, 0, 0]], [np.eye(3)], [[1, 1, 1]], 4.8, 256)
    assert far[0, 0] == 2 ** 31 - 1                              # clamped: invalid, not wrapped
    for bad in (([[0, 0]], [np.eye(3)], [[1, 1, 1]]), ([[0, 0, 0]], [np.eye(2)], [[1, 1, 1]]), ([[0, 0, 0]], [np.eye(3)], [[1, 1]]),
                ([[0, 0, np.nan]], [np.eye(3)], [[1, 1, 1]])):
        with pytest.raises(ValueError):
            oriented_boxes(*bad, 4.8, 256)
    import supereight_amd.pipeline as P
    assert "exact for the rounded box" in P.oriented_boxes.__doc__


# ---------------------------------------------------------------------------------------------------- the Python argument checks
def _pipeline():
    return bare_pipeline(field=0)


@pytest.mark.parametrize("boxes,exc", [
    (np.zeros((4, 12), np.int64), TypeError),
    (np.zeros((4, 12), np.float32), TypeError),
    (np.zeros((4, 6), np.int32), ValueError),
    (np.zeros(48, np.int32), ValueError),
    (np.zeros((2, 2, 12), np.int32), ValueError),
    ([[0] * 12], TypeError),
    (None, TypeError),
], ids=["int64", "float32", "n_by_6", "flat", "3d", "list", "none"])
def test_collides_oriented_refuses_bad_boxes_before_any_library_call(boxes, exc):
    with pytest.raises(exc):
        _pipeline().collides_oriented(boxes)


def test_collides_oriented_refuses_bad_arguments_before_any_library_call():
    p = _pipeline()
    ok = np.zeros((4, 12), np.int32)
    with pytest.raises(ValueError):
        p.collides_oriented(ok, threshold=float("nan"))
    with pytest.raises(ValueError):
        p.collides_oriented(ok, threshold=float("inf"))
    with pytest.raises(ValueError):
        p.collides_oriented(ok, threshold=1e39)           # not finite as a float32
    with pytest.raises(TypeError):
        p.collides_oriented(ok, occupied_above=2)
    with pytest.raises(TypeError):
        p.collides_oriented(ok, occupied_above="yes")


def test_collides_oriented_refuses_bad_torch_boxes():
    torch = pytest.importorskip("torch")
    p = _pipeline()
    with pytest.raises(TypeError):
        p.collides_oriented(torch.zeros((4, 12), dtype=torch.int64))
    with pytest.raises(ValueError):
        p.collides_oriented(torch.zeros((4, 9), dtype=torch.int32))
    with pytest.raises(ValueError):
        p.collides_oriented(torch.zeros((12, 4), dtype=torch.int32).t())       # [4, 12], not contiguous
    with pytest.raises(ValueError):
        p.collides_oriented(torch.zeros((4, 12), dtype=torch.int32))           # a CPU tensor: the device entry reads device memory


# ---------------------------------------------------------------------------------------------------- header text and build list
def test_header_declares_the_oriented_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_collide_oriented(se_hip_pipeline* p, const int32_t* device_boxes, int64_t n, const se_hip_collide_test* test, "
            "uint8_t* device_status);") in flat
    assert ("int se_hip_collide_oriented_host(se_hip_pipeline* p, const int32_t* host_boxes, int64_t n, const se_hip_collide_test* test, "
            "uint8_t* host_status);") in flat
    assert "#define SE_HIP_ORIENTED_SUB 16" in h
    assert "#define SE_HIP_ORIENTED_CENTRE_LIMIT (1 << 20)" in h and "#define SE_HIP_ORIENTED_AXIS_LIMIT (1 << 14)" in h
    for bound in ("2^29", "2^53", "2^49", "8192"):             # the bit budget is stated with its arithmetic
        assert bound in h
    assert "#define SE_HIP_K_COUNT 5" in h                     # no new launch counter
    from supereight_amd import pipeline as P
    assert (P.ORIENTED_SUB, P.ORIENTED_CENTRE_LIMIT, P.ORIENTED_AXIS_LIMIT) == (16, 1 << 20, 1 << 14) == (SUB, C_LIMIT, H_LIMIT)
    for name in ("se_hip_collide_oriented", "se_hip_collide_oriented_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 5 and args[2] is C.c_int64
    host = open(os.path.join(ROOT, "include", "se", "oriented_collision.hpp")).read()
    assert "oriented_sub = 16" in host and "oriented_centre_limit = 1 << 20" in host and "oriented_axis_limit = 1 << 14" in host
    assert INVALID == P.COLLISION_INVALID


def test_build_lists_the_oriented_kernel_header():
    from supereight_amd import build
    assert "se_oriented_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_oriented_kernels.h"' in src
    k = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_oriented_kernels.h")).read()
    assert "k_collide_oriented" in k and "bounded" in k          # the header comment states why every loop ends
    tool = open(os.path.join(ROOT, "tools", "kernel_resources.py")).read()
    assert "k_collide_oriented" in tool
