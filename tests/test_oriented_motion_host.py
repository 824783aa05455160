"""Oriented motion collision queries, host side (no GPU): the header declares both entries, the output struct and the bound; the build lists
the kernel header, whose comment states why every loop ends; the numpy truth (tests/oriented_motion_util.py) gives the hand-worked answers,
holds the interval form and the 21-axis form together, and equals motion_util.motion_truth on axis-aligned boxes; the host restatement
(include/se/oriented_motion.hpp) gives the hand answers too, and its traversal equals its literal definition on random maps, also under
AddressSanitizer and UBSan; oriented_motions() rounds as oriented_boxes() does; collides_oriented_moving turns its arguments into what the
library receives by the rules of the other occupancy readers and refuses the rest before any library call; and the seeded motion set of the
GPU test holds every kind of answer on the maps that test uses."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, _CollideTest
from tests import motion_util
from tests.golden_util import load
from tests.host_util import ROOT, bare_pipeline, build_kats
from tests.oriented_motion_util import (BRUTE_CASES, EMPTY, FREE, HAND_CASES, INVALID, MOVE_LIMIT, OCC, SEED, SUB, UNSEEN, aligned_hand_cases, aligned_motions,
                                        census, entry_cubes, expected_float, from_aligned, hand_motion, motion_hand_grid, oriented_motion_truth,
                                        seeded_motions, shortened, sweep_voxels, valid)

MOTIONS = np.array([[64, 64, 64, 16, 0, 0, 0, 16, 0, 0, 0, 16, 40, -24, 8]], np.int32)


def test_header_declares_the_oriented_motion_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_collide_oriented_motions(se_hip_pipeline* p, const int32_t* device_motions, int64_t n, const se_hip_collide_test* test, "
            "int32_t stop_at, const se_hip_oriented_motion_out* device_out);") in flat
    assert ("int se_hip_collide_oriented_motions_host(se_hip_pipeline* p, const int32_t* host_motions, int64_t n, const se_hip_collide_test* test, "
            "int32_t stop_at, const se_hip_oriented_motion_out* host_out);") in flat
    body = re.search(r"typedef struct se_hip_oriented_motion_out \{(.*?)\} se_hip_oriented_motion_out;", h, re.S).group(1)
    assert re.findall(r"(uint8_t|float|int64_t)\* (\w+);", body) == [("uint8_t", "status"), ("float", "t_first"), ("int64_t", "t_exact")]
    assert "#define SE_HIP_ORIENTED_MOVE_LIMIT (1 << 18)" in h
    assert "t_in is an infimum" in flat and "2^54" in h and "2^59" in h          # the infimum and the arithmetic are stated
    assert "#define SE_HIP_K_COUNT 5" in h           # no new launch counter
    from supereight_amd import pipeline as P
    assert P.ORIENTED_MOVE_LIMIT == MOVE_LIMIT and P.ORIENTED_SUB == SUB
    assert [f[0] for f in P._OrientedMotionOut._fields_] == ["status", "t_first", "t_exact"]
    for name in ("se_hip_collide_oriented_motions", "se_hip_collide_oriented_motions_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 6 and args[2] is C.c_int64 and args[4] is C.c_int32


def test_build_lists_the_kernel_header_and_it_states_why_every_loop_ends():
    from supereight_amd import build
    assert "se_oriented_motion_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_oriented_motion_kernels.h"' in src
    assert "launch_wave_per_item(p, n, k_collide_oriented_motions<true>, k_collide_oriented_motions<false>, a)" in src
    assert 'collide_test_args("se_hip_collide_oriented_motions", test, &stop_at)' in src
    k = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_oriented_motion_kernels.h")).read()
    assert "k_collide_oriented_motions" in k and "se_frontier_pop" in k
    head = re.sub(r"\s*\n//\s*", " ", k[:k.index("#pragma once")])          # the header comment as running text
    assert "Every loop is bounded" in head and "se_frontier.h" in head and "Euclid" in head and "64 blocks" in head
    assert "asm" not in k


# ------------------------------------------------------------------ the truth
def test_numpy_truth_gives_the_hand_answers():
    seen = {}
    for name, (mp, _, _, _, occ, uns) in HAND_CASES.items():
        assert occ[0] == uns[0], name
        assert oriented_motion_truth(motion_hand_grid(mp), hand_motion(name), seen) == (occ[0], occ[1], uns[1]), name
    assert seen["cubes"] > 40000 and seen["touched"] > 10000                 # (the 21-axis form was held to the interval form on each)
    assert {c[0] for c in HAND_CASES.values()} == {"a", "free", "wall", "octant"}
    # the table holds: blocked at the start, strictly between, free, leaving by each face, absent octants, the bounds and what lies beyond them
    ts = [c[4][1] for c in HAND_CASES.values()]
    assert Fraction(0) in ts and FREE in ts and any(0 < t < 1 for t in ts) and sum(c[4][0] == INVALID for c in HAND_CASES.values()) >= 8
    assert all(abs(hand_motion(k)[12 + a]) == MOVE_LIMIT for k, a in (("LimitMoveUp", 0), ("LimitMoveDown", 0)))


def test_vertex_that_slides_on_has_entry_zero_though_the_static_query_says_empty():
    from tests.oriented_util import oriented_truth
    m = hand_motion("VertexSlidesOn")
    grid = motion_hand_grid("a")
    assert oriented_truth(grid, m[:12]) == EMPTY
    assert oriented_motion_truth(grid, m) == (OCC, Fraction(0), Fraction(0))


def test_interval_form_equals_the_21_axis_form_on_cubes_full_of_tangencies():
    """Boxes whose faces, edges and vertices lie on the lattice, moved along lattice directions, against cubes of every side: degenerate axes
    (d = 0, d parallel to a half-axis, zero components) and open ends that only meet."""
    rng = np.random.default_rng(2)
    shapes = [((16, 0, 0), (0, 16, 0), (0, 0, 16)), ((32, 32, 0), (-32, 32, 0), (0, 0, 8)), ((16, 0, 0), (16, 16, 0), (0, 0, 8)),
              ((40, 30, 0), (-30, 40, 0), (0, 0, 50)), ((16, 16, 16), (-16, 16, 0), (8, 8, -16)), ((3, 1, 0), (-1, 3, 1), (1, 0, 4))]
    moves = [(0, 0, 0), (64, 0, 0), (0, -48, 0), (32, 32, 0), (16, 16, 16), (-64, 64, 0), (48, 0, -16), (33, -17, 5)]
    cubes = touched = 0
    for h in shapes:
        for d in moves + [tuple(2 * v for v in h[0]), tuple(-v for v in h[1])]:
            c = (16 * rng.integers(4, 12, 3) + rng.choice([0, 8], 3)).tolist()
            m = c + [v for hi in h for v in hi] + list(d)
            assert valid(m)
            for s in (1, 2, 4, 8):
                lo, hi = sweep_voxels(m)
                v0 = (lo // s - 1) * s
                counts = tuple(int((hi[k] - v0[k]) // s + 2) for k in range(3))
                t, _, _, swept = entry_cubes(m, v0, counts, s)
                assert (t == swept).all(), (m, s)
                cubes += t.size
                touched += int(t.sum())
    assert cubes > 60000 and touched > 10000 and touched < cubes


def test_truth_on_aligned_boxes_equals_the_motion_truth():
    cases = aligned_hand_cases()
    assert len(cases) >= 20 and sum(c[2][0] == INVALID for c in cases.values()) >= 3
    for name, (mp, m, occ, uns) in cases.items():
        assert oriented_motion_truth(motion_hand_grid(mp), m) == (occ[0], occ[1], uns[1]), name
    rng = np.random.default_rng(4)
    grid = np.full((32, 32, 32), EMPTY, np.uint8)
    r = rng.random(grid.shape)
    grid[r < 0.01], grid[r > 0.98] = OCC, UNSEEN
    om, m9 = aligned_motions(rng, 200, 32)
    seen = set()
    for a, b in zip(om.tolist(), m9.tolist()):
        want = motion_util.motion_truth(grid, b)
        assert oriented_motion_truth(grid, a) == want, (a, b)
        seen.add((want[0], want[1] == FREE, want[1] == 0))
    assert seen == {(OCC, False, False), (OCC, False, True), (UNSEEN, True, False), (EMPTY, True, False)}


def test_shortened_motions_are_free_by_the_truth():
    """The identity the GPU test uses: a blocked motion cut at t_exact, rounded down along the segment to the sub-unit lattice, is free."""
    rng = np.random.default_rng(8)
    grid = np.full((32, 32, 32), EMPTY, np.uint8)
    grid[rng.random(grid.shape) < 0.02] = OCC
    mo = seeded_motions(grid, 3, 120)
    truth = [oriented_motion_truth(grid, m) for m in mo.tolist()]
    te = np.array([[t[1].numerator, t[1].denominator] for t in truth], np.int64)
    idx, cut = shortened(mo, te)
    assert len(idx) >= 10
    for m in cut.tolist():
        st, t_occ, _ = oriented_motion_truth(grid, m)
        assert st != OCC and t_occ == FREE, m


# ------------------------------------------------------------------ the host restatement
def _parse(stdout):
    got = {}
    for f in (line.split() for line in stdout.splitlines()):
        v = [int(t) for t in f[1:]]
        got[f[0]] = (v[0], [(v[1 + 3 * s], v[2 + 3 * s], v[3 + 3 * s]) for s in range(2)])
    return got


def test_hand_cases_on_the_host_mirror(tmp_path):
    """The program itself ends with 1 if the traversal and the literal definition, or the two forms of the predicate, differ on a case."""
    exe = build_kats("oriented_motion_kats", tmp_path)
    r = subprocess.run([exe, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _parse(r.stdout)
    assert sorted(got) == sorted(HAND_CASES) and len(BRUTE_CASES) >= len(HAND_CASES) - 3
    for name, (_, _, _, _, occ, uns) in HAND_CASES.items():
        is_valid, answers = got[name]
        assert is_valid == (occ[0] != INVALID), name
        assert answers == [(a[0], a[1].numerator, a[1].denominator) for a in (occ, uns)], (name, answers)      # lowest terms


def test_traversal_equals_the_definition_on_random_maps(tmp_path):
    exe = build_kats("oriented_motion_kats", tmp_path)
    r = subprocess.run([exe, "random", "8", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = dict(zip(r.stdout.split()[0::2], (int(v) for v in r.stdout.split()[1::2])))
    assert f["checked"] == 1200 and f["mismatches"] == 0 and f["differ"] == 0 and f["forms"] > 1000000
    assert min(f["occupied"], f["unseen"], f["empty"], f["blocked"]) >= 20


def test_host_mirror_is_clean_under_the_sanitizers(tmp_path):
    """The same program, stand-alone, with AddressSanitizer and UBSan compiled in: host code with its own main, run directly."""
    exe = str(tmp_path / "oriented_motion_kats_san")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "oriented_motion_kats.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for args in (["kats"], ["random", "2", "3"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_cpp_mirror_program_compiles(tmp_path):
    """tests/cpp/oriented_motion_mirror.cpp (run on the GPU by test_gpu_oriented_motion_mirror.py) compiles against the headers for both fields."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"omm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "oriented_motion_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ metric to fixed point
def test_oriented_motions_rounds_like_oriented_boxes_and_appends_the_displacement():
    from supereight_amd.pipeline import oriented_boxes, oriented_motions
    from tests.oriented_util import random_rotations
    rng = np.random.default_rng(5)
    n, dim, size = 200, 4.8, 512
    c, r, e = rng.uniform(0, dim, (n, 3)), random_rotations(rng, n), rng.uniform(0.01, 0.5, (n, 3))
    d = rng.uniform(-1.0, 1.0, (n, 3))
    d[0] = [0.25 * dim / size / SUB * 2, -0.25 * dim / size / SUB * 6, 0.0]      # exactly half a sub-unit and one and a half: ties go to even
    m = oriented_motions(c, r, e, d, dim, size)
    assert m.dtype == np.int32 and m.shape == (n, 15) and m.flags["C_CONTIGUOUS"]
    assert (m[:, :12] == oriented_boxes(c, r, e, dim, size)).all()
    assert (m[:, 12:] == np.rint(d * (SUB * size / dim)).astype(np.int32)).all()
    assert m[0, 12:].tolist() == [0, -2, 0]
    assert oriented_motions(np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 3)), dim, size).shape == (0, 15)
    assert (oriented_motions(c[:1], r[:1], e[:1], [[1e12, -1e12, 0]], dim, size)[0, 12:] == [2 ** 31 - 1, -2 ** 31, 0]).all()      # clamped: invalid anyway
    for bad in (np.zeros((n, 2)), np.zeros((n + 1, 3)), np.zeros(3)):
        with pytest.raises(ValueError, match="displacements_m"):
            oriented_motions(c, r, e, bad, dim, size)
    with pytest.raises(ValueError, match="non-finite"):
        oriented_motions(c[:1], r[:1], e[:1], [[0.0, float("nan"), 0.0]], dim, size)
    with pytest.raises(ValueError, match="rotations"):
        oriented_motions(c, r[:5], e, d, dim, size)


# ------------------------------------------------------------------ the arguments of collides_oriented_moving
class _Recorder:
    """Stands in for libse_hip.so: keeps the name and the arguments of the one call made."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(h, *args):
            self.calls.append((name, args))
            return 0
        return entry


def _recorded(field, **kw):
    p = bare_pipeline(field=field, _device=0)
    p.lib = _Recorder()
    res = p.collides_oriented_moving(MOTIONS, **kw)
    assert [name for name, _ in p.lib.calls] == ["se_hip_collide_oriented_motions_host"]
    args = p.lib.calls[0][1]
    return args[2]._obj, args, res


@pytest.mark.parametrize("threshold", [float("nan"), float("inf"), 1e39], ids=["nan", "inf", "beyond_float32"])
def test_a_threshold_that_is_not_finite_as_a_float32_is_refused(threshold):
    with pytest.raises(ValueError, match="collides_oriented_moving: threshold"):          # (bare_pipeline: a library call would be an AssertionError)
        bare_pipeline(field=SDF, _device=0).collides_oriented_moving(MOTIONS, threshold=threshold)


@pytest.mark.parametrize("above", [2, "yes"], ids=["int", "str"])
def test_an_occupied_above_that_is_no_bool_is_refused(above):
    with pytest.raises(TypeError, match="collides_oriented_moving: occupied_above"):
        bare_pipeline(field=SDF, _device=0).collides_oriented_moving(MOTIONS, occupied_above=above)


def test_occupied_above_defaults_by_field_and_the_threshold_arrives():
    for field, default in ((SDF, 0), (OFUSION, 1)):
        t, _, _ = _recorded(field)
        assert isinstance(t, _CollideTest) and (t.threshold, t.occupied_above) == (0.0, default)
        assert _recorded(field, occupied_above=None)[0].occupied_above == default
        for above in (False, True, np.bool_(True)):
            t, _, _ = _recorded(field, threshold=0.3, occupied_above=above)
            assert (t.threshold, t.occupied_above) == (C.c_float(0.3).value, int(above))


@pytest.mark.parametrize("stop_at", ["empty", 0, None], ids=["empty", "code", "none"])
def test_a_stop_at_that_names_no_class_is_refused(stop_at):
    with pytest.raises(ValueError, match="collides_oriented_moving: stop_at"):
        bare_pipeline(field=SDF, _device=0).collides_oriented_moving(MOTIONS, stop_at=stop_at)


def test_stop_at_arrives_as_its_status_code_and_the_outputs_asked_for_are_passed():
    assert _recorded(SDF)[1][3] == 0                                               # the default: "occupied"
    for name, code in (("occupied", 0), ("unseen", 1)):
        assert _recorded(SDF, stop_at=name)[1][3] == code
    for kw, shapes in ((dict(), ("status", "t_first")), (dict(t_first=False), ("status",)), (dict(exact=True), ("status", "t_first", "t_exact")),
                       (dict(t_first=False, exact=True), ("status", "t_exact"))):
        _, args, res = _recorded(SDF, **kw)
        assert args[1] == 1                                                       # n
        out = args[4]._obj
        assert out.status and bool(out.t_first) == ("t_first" in shapes) and bool(out.t_exact) == ("t_exact" in shapes)
        res = res if isinstance(res, tuple) else (res,)
        want = {"status": ((1,), np.uint8), "t_first": ((1,), np.float32), "t_exact": ((1, 2), np.int64)}
        assert [(r.shape, r.dtype) for r in res] == [(want[k][0], np.dtype(want[k][1])) for k in shapes]


@pytest.mark.parametrize("motions,exc", [
    (np.zeros((4, 15), np.int64), TypeError),
    (np.zeros((4, 15), np.float32), TypeError),
    (np.zeros((4, 12), np.int32), ValueError),
    (np.zeros((4, 9), np.int32), ValueError),
    (np.zeros(15, np.int32), ValueError),
    (np.zeros((2, 2, 15), np.int32), ValueError),
    ([[0] * 15], TypeError),
    (None, TypeError),
], ids=["int64", "float32", "n_by_12", "n_by_9", "flat", "3d", "list", "none"])
def test_bad_motions_are_refused_before_any_library_call(motions, exc):
    with pytest.raises(exc):
        bare_pipeline(field=SDF, _device=0).collides_oriented_moving(motions)


def test_bad_torch_motions_are_refused():
    torch = pytest.importorskip("torch")
    p = bare_pipeline(field=SDF, _device=0)
    with pytest.raises(TypeError):
        p.collides_oriented_moving(torch.zeros((4, 15), dtype=torch.int64))
    with pytest.raises(ValueError):
        p.collides_oriented_moving(torch.zeros((4, 12), dtype=torch.int32))
    with pytest.raises(ValueError):
        p.collides_oriented_moving(torch.zeros((15, 4), dtype=torch.int32).t())          # [4, 15], not contiguous
    with pytest.raises(ValueError):
        p.collides_oriented_moving(torch.zeros((4, 15), dtype=torch.int32))              # a CPU tensor: the device entry reads device memory


# ------------------------------------------------------------------ the GPU test's motion set is not vacuous
@pytest.mark.parametrize("field,name", [(SDF, "sdf_80x60_128.npz"), (OFUSION, "ofusion_80x60_128.npz")], ids=["sdf", "ofusion"])
def test_seeded_set_holds_every_kind_of_answer(field, name):
    """On the maps of tests/test_gpu_oriented_motion.py -- the first three frames of the golden room fixtures, rebuilt here through the oracle --
    the seeded set has at least 16 motions of each kind, by the truth alone."""
    from oracle.binding import OraclePipeline
    from tests.trace_util import grids_from_octree
    g = load(name)
    W, H, N, _ = (int(v) for v in g["dims"])
    o = OraclePipeline(field, N, float(g["dim"]), W, H)
    for f in range(3):
        o.integrate(g["depth"][f], g["pose"][f], g["k"], float(g["mu"]), f)
    grid, _ = grids_from_octree(N, o.blocks(), o.nodes(), (0.0, 0.0) if field == OFUSION else (1.0, 0.0), 0.0, field == OFUSION)
    o.close()
    mo = seeded_motions(grid, SEED)
    assert mo.shape == (300, 15) and all(valid(m) for m in mo.tolist())
    d = mo[:, 12:15].astype(np.int64)
    assert (np.abs(d) <= 16 * SUB).all() and (d[:30] == 0).all() and ((d[60:120] == 0).sum(1) >= 1).all()
    h = mo[30:60, 3:12].reshape(-1, 3, 3).astype(np.int64)
    assert all(any((np.cross(hi, di) == 0).all() for hi in hh) for hh, di in zip(h, d[30:60]))          # parallel to a half-axis
    kinds = census([oriented_motion_truth(grid, m) for m in mo.tolist()])
    assert all(v >= 16 for v in kinds.values()), kinds
    assert expected_float(Fraction(1, 3)) == np.float32(1 / 3)
