"""CPU side of tests/test_gpu_depth_domain.py.  On the oracle alone: the tables of tests/depth_domain_frames.py hold what they say, every class
of float depth stands in its stated relation to the run with holes in its place (so that no comparison on the device can turn vacuous), stores
no NaN in a map, leaves the raycast something to hit and reads nothing out of bounds while integrating.  And tests/cpp/depth_domain_replay.cpp,
a program of its own built with the address and undefined-behaviour sanitizers, replays the same frames through every entry point the GPU tests
compare against: it ends clean on every class of every stage's table, and in a report on exactly the (stage, class) pairs of STAGE_EXCLUDES --
that run, not bit-equality with whatever an out-of-bounds read returns, is what draws each stage's boundary.  (float-cast-overflow is named
beside `undefined` because g++ leaves it out of that group, and a NaN cast to int is the undefined behaviour in question.)"""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import depth_domain_frames as D
from tests.edge_frames import _render_room, render_room_m, render_room_mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, LARGE = list(D.SHAPES)


def _f32(bits):
    return np.asarray([b for b in bits], np.uint32).view(np.float32)


def test_classes_hold_what_they_are_named_for():
    nan = np.asarray(D.CLASSES["nan"], np.uint32)
    assert np.isnan(nan.view(np.float32)).all() and ((nan >> 22) & 1).all()                    # quiet
    assert len(set(nan >> 31)) == 2 and len(set(nan & 0x3FFFFF)) >= 4                            # both signs, several payloads
    assert _f32(D.CLASSES["pinf"])[0] == np.inf and _f32(D.CLASSES["ninf"])[0] == -np.inf
    neg = _f32(D.CLASSES["negative"])
    assert (neg < 0).all() and neg.max() == np.float32(-1e-3) and neg.min() == -5
    z = _f32(D.CLASSES["negzero"])
    assert z[0] == 0 and np.signbit(z[0])
    tiny = _f32(D.CLASSES["tiny"])
    flt_min = np.finfo(np.float32).tiny
    assert (tiny > 0).all() and tiny.min() == np.float32(1e-45) and flt_min in tiny and (tiny < flt_min).sum() == 2 and tiny.max() == np.float32(1e-6)
    far = _f32(D.CLASSES["far"])
    assert far.min() == np.float32(65.536) > np.float32(65.535) and far.max() == D.CAP_M          # beyond what uint16 millimetres hold, up to the cap
    planes = _f32(D.CLASSES["planes"])
    for p, plane in ((planes[:3], D.NEAR_PLANE), (planes[3:], D.FAR_PLANE)):
        assert p[1] == plane and p[0] == np.nextafter(plane, np.float32(0)) and p[2] == np.nextafter(plane, np.float32(np.inf))
    assert D.CLASSES["offgrid"] == (D.OFFGRID,) and D.CASES[-1] == "mixed" and "holes" not in D.CLASSES
    for (stage, c), reason in D.STAGE_EXCLUDES.items():
        assert stage in D.STAGES and c in D.CLASSES and reason


def test_the_cap_is_asserted():
    D.check_cap(np.float32([0, -1000, 1000, np.inf, -np.inf, np.nan]))
    for bad in (np.nextafter(np.float32(1000), np.float32(np.inf)), -1001.0, 1e30):
        with pytest.raises(AssertionError):
            D.check_cap(np.float32([1.0, bad]))
    for case in D.CASES:
        for d in D.domain_frames(case, SMALL).depths:                                            # (built through check_cap; once more from outside)
            fin = np.isfinite(d)
            assert np.abs(d[fin]).max() <= D.CAP_M


@pytest.mark.parametrize("W,H,k", [(80, 60, None), (163, 101, (150.0, 130.0, 70.3, 55.1))])
def test_render_room_m_is_the_room_between_the_millimetres(W, H, k):
    from supereight_amd.synthetic import intrinsics
    k = intrinsics(W) if k is None else k
    for f in (2, 3):          # (frame 0 looks straight at the far wall, 1.704 m away in every pixel that sees it: on the grid by itself)
        m, mm = render_room_m(f, W, H, D.DIM, k), render_room_mm(f, W, H, D.DIM, k)
        assert m.dtype == np.float32 and m.shape == (H, W) and np.isfinite(m).all() and (m > 0).all()
        assert (m == _render_room(f, W, H, D.DIM, k).astype(np.float32)).all()
        below = m.astype(np.float64) * 1000.0 - mm
        assert (below > -1e-3).all() and (below < 1 + 1e-3).all()                                # mm is its floor, give or take the float32 rounding
        on_grid = m == mm.astype(np.float32) / np.float32(1000.0)
        assert on_grid.mean() < 0.05


@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_frames_are_built_as_stated(shape):
    W, H, _ = D.SHAPES[shape]
    holes = D.domain_frames("holes", shape)
    assert len(holes) == D.FRAMES == 4 and D.FIRST == 2
    for f in range(D.FRAMES):
        m = D.mask_of(W, H, f)
        ys, xs = np.nonzero(m)
        # a whole 16 x 16 square on the 8 x 8 tile grid, and a tenth of the rest
        full = [(x0, y0) for y0 in range(0, H - 15, 8) for x0 in range(0, W - 15, 8) if m[y0:y0 + 16, x0:x0 + 16].all()]
        assert len(full) == 1, (f, full)
        assert 0.08 < (m.sum() - 256) / (W * H - 256) < 0.12
        assert (holes.masks[f] == m).all() if f >= D.FIRST else not holes.masks[f].any()
    for case in D.CASES:
        s = D.domain_frames(case, shape)
        vals = D.class_values(D.classes_of(case))
        for f in range(D.FRAMES):
            same = s.depths[f].view(np.uint32) == holes.depths[f].view(np.uint32)
            if f < D.FIRST:
                assert same.all(), (case, f)
                continue
            m = s.masks[f]
            if case != "offgrid":
                assert same[~m].all(), (case, f)
            got = s.depths[f][m].view(np.uint32)
            fixed = vals[vals != D.OFFGRID].astype(np.uint32)
            if len(fixed):
                assert set(fixed.tolist()) <= set(got.tolist()), (case, f)                     # every pattern of the class occurs
            if case == "mixed":
                assert len(set(got.tolist()) - set(fixed.tolist())) > 20                          # ... and the off-grid share
            if case == "offgrid":
                room = render_room_m(f, W, H, D.DIM, s.k)
                keep = holes.depths[f] != 0
                assert (s.depths[f][keep | m] == room[keep | m]).all() and (s.depths[f][~(keep | m)] == 0).all()


def _nan_in(run):
    return int(sum(np.isnan(a).sum() for a in (run["blocks"][1], run["blocks"][2], run["nodes"][2], run["nodes"][3])))


@pytest.mark.parametrize("shape", [SMALL, LARGE])
@pytest.mark.parametrize("field_name", list(D.FIELDS))
@pytest.mark.parametrize("case", D.CASES)
def test_relation_to_the_holes_run(case, field_name, shape):
    run, holes = D.oracle_run(case, field_name, shape), D.oracle_run("holes", field_name, shape)
    got, want = D.relation(run, holes), D.expected_relation(case, field_name, shape)
    print(case, field_name, shape, "relation", got, "pinned", want, "hits", run["hits"], "blocks", len(run["blocks"][0]))
    for key, floor in want.items():
        if floor == 0:
            assert got[key] == 0, (key, got)
        elif floor is not None:
            assert got[key] >= floor, (key, got, floor)
    if all(v == 0 for v in want.values()):                    # identical to holes: the whole map and the raycast, bit for bit
        for a, b in zip(run["blocks"] + run["nodes"], holes["blocks"] + holes["nodes"]):
            assert a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()
        assert (run["vertex"].view(np.uint32) == holes["vertex"].view(np.uint32)).all()
    assert _nan_in(run) == 0
    assert run["hits"] >= 50
    assert run["truncated"] == 0 and run["oob_ub_integration"] == 0
    assert len(run["blocks"][0]) >= 300 and run["swept"][-1] > 0


def test_every_class_changes_something_somewhere():
    """No row of RELATION is all "identical" for both fields except the three that are holes by definition."""
    for case in D.CASES:
        changes = any(v for f in D.FIELDS for v in D.RELATION[case][f][SMALL] if v)
        assert changes == (case not in ("ninf", "negzero")), case
    # the rows that tell a comparison from its cheaper look-alike
    assert D.RELATION["nan"]["ofusion"][SMALL][1] > 0 and D.RELATION["nan"]["sdf"][SMALL] == (0, 0, 0)         # !(d <= 0) against d > 0
    assert D.RELATION["negative"]["ofusion"][SMALL][2] > 0 and D.RELATION["negative"]["sdf"][SMALL][2] > 0    # !(d == 0) against d > 0
    assert D.RELATION["tiny"]["sdf"][SMALL][2] > 0                                                             # denormals kept


# ------------------------------------------------------------------ the stand-alone replay under the sanitizers
SANITIZE = "-fsanitize=address,undefined,float-cast-overflow"


@functools.lru_cache(maxsize=None)
def _replay_exe():
    d = tempfile.mkdtemp(prefix="depth_domain_replay_")
    exe = os.path.join(d, "depth_domain_replay_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", SANITIZE, "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "cpp", "depth_domain_replay.cpp"), "-o", exe], capture_output=True, text=True)      # (no -fopenmp)
    assert r.returncode == 0, r.stderr
    return d, exe


def _sequence(case, stage):
    """What a stage is given: the scan / sweep / raycast and the image stages take the case's four frames; the tracker four clean frames and
    a fifth that holds the case.  `mixed` holds every class of the stage's table."""
    W, H, N = D.SHAPES[SMALL]
    classes = D.stage_classes(stage) if case == "mixed" else (case,)
    if stage == "track":
        return (case, D.ConsumerFrames(classes, W, H, D.DIM), N, D.DIM)
    if case == "mixed" and classes != D.ALONE:
        return (case, D.DomainStream(classes, W, H), N, D.DIM)
    return (case, D.domain_frames(case, SMALL), N, D.DIM)


def _lines(stdout):
    out = {}
    for line in stdout.splitlines():
        f = line.split()
        out[(f[0], f[1])] = dict(zip(f[2::2], (int(v) for v in f[3::2])))
    return out


def test_sanitized_replay_ends_clean_on_every_stage_table():
    d, exe = _replay_exe()
    seen = {}
    for stage in D.STAGES:
        cases = [c for c in D.CASES if (stage, c) not in D.STAGE_EXCLUDES]
        path = os.path.join(d, f"{stage}.bin")
        D.write_replay_file(path, [_sequence(c, stage) for c in cases])
        r = subprocess.run([exe, path, stage], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (stage, r.stderr[-2000:])
        got = _lines(r.stdout)
        assert sorted(c for c, _ in got) == sorted(cases * (2 if stage == "track" else 1)), (stage, r.stdout)
        seen[stage] = got
    # the program replays what the Python side runs: the same maps and raycasts, by their counts
    for field_name in D.FIELDS:
        for case in D.ALONE:
            run, line = D.oracle_run(case, field_name, SMALL), seen[field_name][(case, field_name)]
            assert line["blocks"] == len(run["blocks"][0]) and line["nodes"] == len(run["nodes"][0]), (case, line)
            assert line["hits"] == run["hits"] >= 50 and line["probes"] == sum(run["probes"]) and line["raycast"] == 3, (case, line)
            assert line["nan"] == 0 and line["truncated"] == 0 and line["oob_ub_integration"] == 0, (case, line)
    # the consumers see the values: NaN centres give NaN pyramid pixels, and every tracked frame is tracked
    assert seen["pyramid"][("nan", "pyramid")]["nan1"] > 50 and seen["pyramid"][("negative", "pyramid")]["nan1"] == 0
    assert seen["filter"][("nan", "filter")]["nan"] > 500 and seen["filter"][("offgrid", "filter")]["nan"] == 0
    for (case, stage), line in seen["track"].items():
        assert line["tracked"] == 1 and line["iterations"] >= 3 and line["inliers"] > 1000, (case, stage, line)


@pytest.mark.parametrize("stage,case", list(D.STAGE_EXCLUDES), ids=[f"{s}-{c}" for s, c in D.STAGE_EXCLUDES])
def test_sanitized_replay_reports_the_excluded_pairs(stage, case):
    """The reference is not defined there: the exclusion is a finding of this run, not a convenience."""
    d, exe = _replay_exe()
    path = os.path.join(d, f"excluded_{stage}_{case}.bin")
    D.write_replay_file(path, [_sequence(case, stage)])
    r = subprocess.run([exe, path, stage], capture_output=True, text=True, timeout=600)
    print(stage, case, [line for line in r.stderr.splitlines() if "runtime error" in line][:1])
    assert r.returncode != 0 and "runtime error" in r.stderr and "se_oracle.cpp" in r.stderr, r.stderr[-2000:]
