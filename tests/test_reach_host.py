"""The reachability field, host side (no GPU): the header declares both entries and the constants, the build lists the kernel header, the
host definition (include/se/reach_field.hpp) gives the hand-worked answers and equals the restatement of the device's tile scheme under every
tile order on random maps of both fields -- also as a stand-alone program under the host sanitizers --, the numpy truth of the GPU tests gives
the same hand answers and the table of counts on the `comb` map, the hand requests are not vacuous, reach_path follows hand arrays, and the
Python wrapper refuses every request the C entry refuses before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from supereight_amd.pipeline import REACH_AT_SEED, REACH_MAX_SEEDS, REACH_MOVES, REACH_NONE, reach_path
from tests.clearance_util import OCC, UNSEEN
from tests.host_util import bare_pipeline, build_kats
from tests.reach_util import (AT_SEED, COMB_SEEDS, COMB_TABLE, DEVICE_REQUESTS, HAND_CASES, LIMIT, MOVES, NONE, REACH_MAPS, equidistant, hand_truth,
                              next_choices, reach_grid, reach_truth, valid)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_reach_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_reach_field(se_hip_pipeline* p, const se_hip_reach_request* request, const se_hip_collide_test* test, "
            "const se_hip_reach_out* device_out);") in flat
    assert ("int se_hip_reach_field_host(se_hip_pipeline* p, const se_hip_reach_request* request, const se_hip_collide_test* test, "
            "const se_hip_reach_out* host_out);") in flat
    assert "#define SE_HIP_REACH_NONE (-1)" in h and "#define SE_HIP_REACH_AT_SEED 6" in h and "#define SE_HIP_REACH_MAX_SEEDS 255" in h
    assert (REACH_NONE, REACH_AT_SEED, REACH_MAX_SEEDS) == (-1, 6, 255) == (NONE, AT_SEED, 255) and REACH_MOVES == MOVES
    body = re.search(r"typedef struct se_hip_reach_request \{(.*?)\} se_hip_reach_request;", h, re.S).group(1)
    assert re.findall(r"int32_t\*? (\w+)(?:\[3\])?;", body) == ["lo", "side", "robot", "stop_at", "n_seeds", "seeds"]
    body = re.search(r"typedef struct se_hip_reach_out \{(.*?)\} se_hip_reach_out;", h, re.S).group(1)
    assert re.findall(r"\w+_t\* (\w+);", body) == ["steps", "seed", "next", "counts"]
    text = re.sub(r"\s*\n \*\s*", " ", h)                                                       # the comment's lines joined
    assert "2^24 positions" in text and "rounds <= max steps + 2" in text
    assert "NEITHER ENTRY IS ASYNCHRONOUS" in text and "both entries have synchronised the handle's stream when they return" in text
    assert "#define SE_HIP_K_COUNT 5" in h                                                        # no new launch counter
    from supereight_amd import pipeline as P
    assert [f[0] for f in P._ReachRequest._fields_] == ["lo", "side", "robot", "stop_at", "n_seeds", "seeds"] and C.sizeof(P._ReachRequest) == 56
    assert P._ReachRequest.seeds.offset == 48
    assert [f[0] for f in P._ReachOut._fields_] == ["steps", "seed", "next", "counts"]
    for name in ("se_hip_reach_field", "se_hip_reach_field_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 4
    mirror = open(os.path.join(ROOT, "include", "se", "DenseSLAMSystem.h")).read()
    assert "bool reachField(const se_hip_reach_request& request, const se_hip_collide_test& test, se_hip_reach_out& host_out)" in mirror


def test_build_lists_the_reach_kernel_header():
    from supereight_amd import build
    assert "se_reach_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_reach_kernels.h"' in src
    k = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_reach_kernels.h")).read()
    for name in ("k_reach_free", "k_reach_seed", "k_reach_relax", "k_reach_finish", "__syncthreads_or"):
        assert name in k
    assert "k_field_classify" in src.split("int run_reach")[1].split("int se_hip_reach_field(")[0]       # the classification pass is reused
    # termination belongs to the host: nothing in the kernels waits for another workgroup
    code = k.split("#pragma once")[1]
    assert "while" not in code and "cooperative" not in code and "grid.sync" not in code


def _parse(stdout):
    got = {}
    for f in (line.split() for line in stdout.splitlines()):
        if f[1] == "invalid":
            got[f[0]] = None
            continue
        v = [int(t) for t in f[1:]]
        got.setdefault(f[0], ([], []))
        got[f[0]][0].append(tuple(v[0:3]))
        got[f[0]][1].append(tuple(v[3:6]))
    return got


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    return build_kats("reach_kats", tmp_path_factory.mktemp("reach_kats"))


def test_hand_cases_on_the_host_mirror(kats):
    """The program itself ends with 1 if the definition and a run of the tile scheme differ on a case, or a run exceeds the round bound."""
    r = subprocess.run([kats, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _parse(r.stdout)
    assert sorted(got) == sorted(HAND_CASES)
    for name, (_, lo, side, robot, seeds, occ, uns) in HAND_CASES.items():
        if occ is None:
            assert got[name] is None and not valid(lo, side, robot, len(seeds)), name
        else:
            assert got[name] == (occ, uns), (name, got[name])
            assert valid(lo, side, robot, len(seeds)) and len(occ) == side[0] * side[1] * side[2]
    assert not valid((0, 0, 0), (1, 1, 1), (1, 1, 1), 0) and not valid((0, 0, 0), (1, 1, 1), (1, 1, 1), 256) and valid((0, 0, 0), (1, 1, 1), (1, 1, 1), 255)


def _random_line(stdout):
    f = stdout.split()
    return {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}


def _check_random(res):
    assert res["sdf"] >= 2000 and res["ofusion"] >= 2000
    assert res["runs"] == 12 * (res["sdf"] + res["ofusion"])                 # two tile shapes x three orders x current and stale halos
    assert res["mismatches"] == 0 and res["late"] == 0
    assert res["positions"] > 500000 and 0 < res["cut"] < res["free"] < res["positions"] and res["reached"] > 100000
    assert res["most_rounds"] >= 4                                          # keys crossed tile faces round after round


def test_tile_scheme_equals_the_definition_on_random_maps(kats):
    r = subprocess.run([kats, "random", "80", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    _check_random(_random_line(r.stdout))


def test_kats_are_clean_under_the_host_sanitizers(tmp_path):
    """tests/cpp/reach_kats.cpp as a stand-alone program, built with -fsanitize=address,undefined: both modes run clean."""
    exe = str(tmp_path / "reach_kats_san")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "reach_kats.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr
    r = subprocess.run([exe, "random", "80", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stderr + r.stdout
    _check_random(_random_line(r.stdout))


def test_numpy_truth_gives_the_hand_answers():
    """reach_truth (what the GPU tests use as truth) on the same cases."""
    checked = 0
    for name, (mp, lo, side, robot, seeds, occ, uns) in HAND_CASES.items():
        if occ is None:
            continue
        for stop, exp in ((OCC, occ), (UNSEEN, uns)):
            free, steps, seed, nxt, counts = reach_truth(reach_grid(mp), (lo, side, robot), seeds, stop)
            assert steps.shape == (side[2], side[1], side[0]) and steps.dtype == np.int32 and seed.dtype == np.uint8 and nxt.dtype == np.uint8
            assert list(zip(steps.reshape(-1).tolist(), seed.reshape(-1).tolist(), nxt.reshape(-1).tolist())) == exp, (name, stop)
            reached = [e for e in exp if e[0] >= 0]
            assert counts == (int(free.sum()), len(reached), max((e[0] for e in reached), default=-1))
        checked += 1
    assert checked == 7


@pytest.mark.parametrize("row", range(len(COMB_TABLE)))
def test_numpy_truth_gives_the_table_of_the_comb(row):
    rq, stop, counts, usable = COMB_TABLE[row]
    free, steps, seed, nxt, got = hand_truth("comb", rq, COMB_SEEDS, stop)
    assert got == counts
    assert sorted(set(seed[steps == 0].tolist())) == list(usable)
    # following next from the farthest position arrives at its seed after steps moves
    k, j, i = np.argwhere(steps == counts[2])[0]
    path = reach_path(nxt, rq[0], (rq[0][0] + i, rq[0][1] + j, rq[0][2] + k))
    assert len(path) == counts[2] + 1 and tuple(path[-1]) == COMB_SEEDS[seed[k, j, i]]
    assert (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()
    lo = np.asarray(rq[0])
    assert all(free[tuple((p - lo)[::-1])] for p in path)


def test_the_hand_requests_are_not_vacuous():
    """Over the requests the device is held to on the hand maps, the truths contain every kind of position and every rule at work."""
    blocked = cut = tie = choice = most = 0
    seeds_seen, outside_seed, unfree_seed, duplicate, beyond = set(), 0, 0, 0, set()
    for mp in REACH_MAPS:
        for lo, side, robot, seeds in DEVICE_REQUESTS[mp]:
            for stop in (OCC, UNSEEN):
                free, steps, seed, nxt, counts = hand_truth(mp, (lo, side, robot), seeds, stop)
                blocked += int((~free).sum()); cut += int((free & (steps < 0)).sum())
                most = max(most, counts[2])
                if len(set(seed[steps >= 0].tolist())) >= 2:
                    seeds_seen.add((mp, lo, stop))
                    if side[0] * side[1] * side[2] <= 40000:
                        tie += int(equidistant(reach_grid(mp), (lo, side, robot), seeds, stop).sum())
                choice += int((next_choices(steps, seed) >= 2).sum())
                duplicate += len(set(seeds)) < len(seeds)
                for s in seeds:
                    r = [s[k] - lo[k] for k in range(3)]
                    if not all(0 <= r[k] < side[k] for k in range(3)):
                        outside_seed += 1
                    elif not free[r[2], r[1], r[0]]:
                        unfree_seed += 1
                for k in range(3):
                    if lo[k] < 0:
                        beyond.add((k, 0))
                    if lo[k] + side[k] > 64:
                        beyond.add((k, 1))
    assert blocked > 0 and cut > 0 and len(seeds_seen) > 0
    assert tie >= 20 and choice >= 20
    assert outside_seed > 0 and unfree_seed > 0 and duplicate > 0
    assert beyond == {(k, f) for k in range(3) for f in range(2)}            # a region beyond every face of the volume
    assert most >= 400


def test_reach_path_on_hand_arrays():
    X = 255
    nxt = np.full((1, 3, 4), X, np.uint8)
    nxt[0, 0] = [6, 0, 0, X]            # a row towards -x
    nxt[0, 1] = [2, X, X, X]            # (0, 1) steps -y onto the seed
    nxt[0, 2] = [2, 0, 0, 0]
    lo = (10, 20, 30)
    assert reach_path(nxt, lo, (12, 20, 30)).tolist() == [[12, 20, 30], [11, 20, 30], [10, 20, 30]]
    assert reach_path(nxt, lo, (13, 22, 30)).tolist() == [[13, 22, 30], [12, 22, 30], [11, 22, 30], [10, 22, 30], [10, 21, 30], [10, 20, 30]]
    assert reach_path(nxt, lo, (10, 20, 30)).tolist() == [[10, 20, 30]]
    for start in ((13, 20, 30), (11, 21, 30), (9, 20, 30), (10, 20, 31)):        # no move there, or outside the region
        p = reach_path(nxt, lo, start)
        assert p.shape == (0, 3) and p.dtype == np.int64
    loop = np.array([[[1, 0]]], np.uint8)                                        # +x, -x: no navigation function; bounded by the array size
    with pytest.raises(ValueError):
        reach_path(loop, (0, 0, 0), (0, 0, 0))
    with pytest.raises(ValueError):
        reach_path(np.array([[[1, X]]], np.uint8), (0, 0, 0), (0, 0, 0))          # leads to a position without a move
    with pytest.raises(ValueError):
        reach_path(np.array([[[0, 6]]], np.uint8), (0, 0, 0), (0, 0, 0))          # leads out of the region
    with pytest.raises(ValueError):
        reach_path(nxt.astype(np.int32), lo, lo)


def test_cpp_mirror_reach_program_compiles(tmp_path):
    """tests/cpp/reach_mirror.cpp (run on the GPU by test_gpu_reach_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"rm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "reach_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _pipeline():
    return bare_pipeline(field=0, _device=0)


OK = dict(lo=(0, 0, 0), side=(4, 4, 4), seeds=[(1, 1, 1)])

# every refusal of the C entry that a Python caller can express, one case each
REFUSED = {
    "side_zero": dict(side=(4, 0, 4)),
    "robot_zero": dict(robot=(1, 1, 0)),
    "robot_257": dict(robot=(257, 1, 1)),
    "lo_below_limit": dict(lo=(-LIMIT - 1, 0, 0)),
    "lo_above_limit": dict(lo=(0, LIMIT + 1, 0)),
    "end_above_limit": dict(lo=(0, 0, LIMIT - 5), side=(4, 4, 4), robot=(1, 1, 2)),
    "positions_above_2_24": dict(side=(256, 256, 257)),
    "no_seed": dict(seeds=np.zeros((0, 3), np.int32)),
    "seeds_256": dict(seeds=np.zeros((256, 3), np.int32)),
    "seed_beyond_int32": dict(seeds=[(1 << 31, 0, 0)]),
    "stop_at_empty": dict(stop_at="empty"),
    "stop_at_int": dict(stop_at=0),
    "threshold_nan": dict(threshold=float("nan")),
    "threshold_inf": dict(threshold=float("inf")),
    "threshold_beyond_float32": dict(threshold=1e39),
}
WRONG_TYPE = {
    "occupied_above_int": dict(occupied_above=2),
    "occupied_above_str": dict(occupied_above="yes"),
    "lo_float": dict(lo=(0.0, 0.0, 0.0)),
    "side_none": dict(side=None),
    "seeds_float": dict(seeds=[(1.0, 1.0, 1.0)]),
    "seeds_none": dict(seeds=None),
    "robot_bool": dict(robot=True),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_reach_field_refuses_before_any_library_call(name):
    with pytest.raises(ValueError):
        _pipeline().reach_field(**{**OK, **REFUSED[name]})


@pytest.mark.parametrize("name", sorted(WRONG_TYPE))
def test_reach_field_refuses_wrong_types_before_any_library_call(name):
    with pytest.raises(TypeError):
        _pipeline().reach_field(**{**OK, **WRONG_TYPE[name]})


def test_reach_field_refuses_wrong_shapes():
    for kw in (dict(lo=(0, 0)), dict(side=(4, 4, 4, 4)), dict(robot=2), dict(lo=[[0, 0, 0]]), dict(seeds=(1, 1, 1)), dict(seeds=[(1, 1)]), dict(seeds=[[(1, 1, 1)]])):
        with pytest.raises(ValueError):
            _pipeline().reach_field(**{**OK, **kw})


class _Recorder:
    """Stands in for libse_hip.so where a test wants to see what the wrapper passes: keeps the request of the host entry."""
    def __init__(self):
        self.rq, self.test, self.seeds, self.wanted = None, None, None, None

    def se_hip_reach_field_host(self, h, rq, test, out):
        r, t, o = rq._obj, test._obj, out._obj
        self.rq = (tuple(r.lo), tuple(r.side), tuple(r.robot), r.stop_at, r.n_seeds)
        self.seeds = np.ctypeslib.as_array(C.cast(r.seeds, C.POINTER(C.c_int32)), (r.n_seeds, 3)).copy()
        self.test, self.wanted = (t.threshold, t.occupied_above), (bool(o.steps), bool(o.seed), bool(o.next), bool(o.counts))
        return 0


def test_the_bounds_themselves_pass_the_check():
    """A side product of exactly 2^24, 255 seeds, seeds at the ends of int32, a robot of 256 and coordinates on +-2^19 reach the library (here: a
    recorder in its place)."""
    p = _pipeline()
    p.lib = _Recorder()
    ends = np.array([[-(1 << 31), (1 << 31) - 1, 0]] * 255, np.int64)
    got = p.reach_field((0, 0, 0), (256, 256, 256), ends)
    assert set(got) == {"steps"} and got["steps"].shape == (256, 256, 256) and got["steps"].dtype == np.int32
    assert p.lib.rq == ((0, 0, 0), (256, 256, 256), (1, 1, 1), 0, 255) and p.lib.wanted == (True, False, False, False)
    assert (p.lib.seeds == ends).all()
    assert valid((0, 0, 0), (256, 256, 256), (1, 1, 1), 255) and not valid((0, 0, 0), (256, 256, 257), (1, 1, 1), 255)
    got = p.reach_field((-LIMIT, 5, LIMIT - 258), (2, 3, 2), [(1, 2, 3), (4, 5, 6)], robot=(1, 1, 256), stop_at="unseen", threshold=0.5, occupied_above=True,
                        seed=True, next=True, counts=True)
    assert got["steps"].shape == got["seed"].shape == got["next"].shape == (2, 3, 2) and got["seed"].dtype == got["next"].dtype == np.uint8
    assert got["counts"].shape == (4,) and got["counts"].dtype == np.int64
    assert p.lib.rq == ((-LIMIT, 5, LIMIT - 258), (2, 3, 2), (1, 1, 256), 1, 2) and p.lib.test == (0.5, 1) and p.lib.wanted == (True, True, True, True)
    assert p.lib.seeds.tolist() == [[1, 2, 3], [4, 5, 6]]
    p.field = 1
    p.reach_field(np.array([1, 2, 3], np.int64), np.array([1, 1, 1], np.uint8), np.array([[7, 8, 9]], np.uint16), next=True)
    assert p.lib.rq == ((1, 2, 3), (1, 1, 1), (1, 1, 1), 0, 1) and p.lib.test == (0.0, 1) and p.lib.wanted == (True, False, True, False)   # OFusion: occupied above by default
