"""The oracle's value setter (OraclePipeline.set_values, the inverse of blocks() / nodes()) and the oracle alone over the frame-number schedules
and edit lists of tests/time_axis_util.py: the conditions under which the device comparisons of test_gpu_time_axis.py and
test_gpu_fuse_after_edit.py mean something -- every regime of OFusion's time axis is entered by at least 1000 updated voxels, the backwards
schedule stores both -1000 and +1000, no NaN is ever stored, the key buffer never saturates, the gates follow the rate."""
import numpy as np
import pytest

from oracle.binding import OFUSION, SDF, OraclePipeline
from tests import time_axis_util as T
from tests.time_axis_util import DIM, H, MU, N, W, bits, snapshot

FIELDS = [SDF, OFUSION]
FIELD_IDS = ["sdf", "ofusion"]


def _same(a, b):
    return all(u.shape == w.shape and (bits(u) == bits(w)).all() if u.dtype == np.float32 else (u == w).all() for u, w in zip(a, b))


def _fused(field, frames=4):
    k, depths, poses = T.stream_frames()
    cpu = OraclePipeline(field, N, DIM, W, H)
    for i in range(frames):
        cpu.integrate(depths[i], poses[i], k, MU[field], i)
    return cpu


# ------------------------------------------------------------------ the setter
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_setting_what_was_read_is_the_identity(field):
    cpu = _fused(field)
    before = snapshot(cpu)
    assert len(before[0]) > 100 and len(before[4]) > 20
    assert cpu.set_values(cpu.blocks(), cpu.nodes()) == (len(before[0]), len(before[4]))
    assert _same(before, snapshot(cpu))
    assert cpu.set_values() == (0, 0) and _same(before, snapshot(cpu))
    cpu.close()


@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_random_bits_read_back(field):
    """Any float32 bit pattern but a NaN's (what a NaN's payload becomes on its way through the oracle's double y is the host's business), in a
    shuffled subset of the blocks and nodes plus some that do not exist: the subset reads back bit for bit, the rest is untouched, the count
    says how many were found, and block set, node set, sides and active flags stay."""
    rng = np.random.default_rng(3 + field)
    cpu = _fused(field)
    c, x, y, a, code, side, nx, ny = snapshot(cpu)

    def rand(shape):
        u = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
        u[(u & 0x7F800000) == 0x7F800000] &= np.uint32(0xFF800000)       # NaN -> the infinity of its sign
        return u.view(np.float32)

    rows = rng.permutation(len(c))[: len(c) // 2]
    nrows = rng.permutation(len(code))[: len(code) // 2]
    absent = np.array([[N - 8, N - 8, N - 8], [-8, 0, 0], [0, N, 0]], np.int32)
    assert not (c[:, None, :] == absent[None]).all(2).any()
    sc = np.concatenate([c[rows], absent])
    sx, sy = rand((len(sc), 512)), rand((len(sc), 512))
    scode = np.concatenate([code[nrows], np.array([np.uint64(0xFFFFFFFFFFFF)])])
    snx, sny = rand((len(scode), 8)), rand((len(scode), 8))
    assert cpu.set_values(blocks=(sc, sx, sy), nodes=(scode, snx, sny)) == (len(rows), len(nrows))
    c2, x2, y2, a2, code2, side2, nx2, ny2 = snapshot(cpu)
    assert (c2 == c).all() and (a2 == a).all() and (code2 == code).all() and (side2 == side).all()
    assert (bits(x2[rows]) == bits(sx[: len(rows)])).all() and (bits(y2[rows]) == bits(sy[: len(rows)])).all()
    assert (bits(nx2[nrows]) == bits(snx[: len(nrows)])).all() and (bits(ny2[nrows]) == bits(sny[: len(nrows)])).all()
    rest, nrest = np.setdiff1d(np.arange(len(c)), rows), np.setdiff1d(np.arange(len(code)), nrows)
    assert (bits(x2[rest]) == bits(x[rest])).all() and (bits(y2[rest]) == bits(y[rest])).all()
    assert (bits(nx2[nrest]) == bits(nx[nrest])).all() and (bits(ny2[nrest]) == bits(ny[nrest])).all()
    cpu.close()


@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_identity_setter_between_frames_changes_nothing(field):
    """The lists, the active flags and the key buffer are left alone: a run that sets what it has just read after every frame ends where the
    undisturbed run ends, images included."""
    k, depths, poses = T.stream_frames()
    runs = []
    for disturb in (False, True):
        cpu = OraclePipeline(field, N, DIM, W, H)
        imgs = []
        for i in range(8):
            cpu.integrate(depths[i], poses[i], k, MU[field], i)
            if disturb:
                cpu.set_values(cpu.blocks(), cpu.nodes())
            imgs.append(cpu.raycast(poses[i], k, MU[field], i)[1:])
        runs.append((snapshot(cpu), imgs))
        cpu.close()
    assert _same(runs[0][0], runs[1][0])
    for (v0, n0), (v1, n1) in zip(runs[0][1], runs[1][1]):
        assert (bits(v0) == bits(v1)).all() and (bits(n0) == bits(n1)).all()


# ------------------------------------------------------------------ the schedules on the oracle alone
def test_ofusion_at_mu_002_saturates_the_key_buffer():
    """Why OFusion runs at mu = 0.015 here: at 0.02 the first scan of this shape emits more keys than the reference reserves, the oracle counts
    the scan as truncated and its block set depends on the thread interleaving -- nothing to compare a device with."""
    k, depths, poses = T.stream_frames()
    cpu = OraclePipeline(OFUSION, N, DIM, W, H)
    cpu.count_stats(True)
    cpu.integrate(depths[0], poses[0], k, 0.02, 0)
    st = cpu.stats()
    assert st["keys_emitted"] > (N // 8) * W * H and st["truncated"] == 1, st
    cpu.close()
    assert MU[OFUSION] < 0.02 and MU[SDF] == 0.02


REGIME = {   # schedule -> [(frame, regime, at least)]
    "gapped": [(200, "dt_ge4", 1000), (700, "dt_ge4", 1000)],
    "backwards": [(380, "dt_lt0", 1000), (100, "dt_lt0", 1000), (381, "pole", 1)],
    "plateau_2p24": [(2 ** 24 - 1, "dt_eq0", 1000), (2 ** 24 + 1, "dt_eq0", 1000)],
    "top_2p32": [(f, "dt_eq0", 1000) for f in range(2 ** 32 - 5, 2 ** 32)],
    "three_million": [],
    "rate3": [],
    "rate7": [],
}


def test_timestamps_of_the_schedules():
    """The frame numbers do to the float timestamp what the schedules are there for."""
    ts = T.timestamp
    assert ts(2 ** 24 - 1) == ts(2 ** 24 - 2) != ts(2 ** 24 - 3) and ts(2 ** 24 + 1) == ts(2 ** 24) != ts(2 ** 24 + 2)
    assert len({float(ts(f)) for f in range(2 ** 32 - 6, 2 ** 32)}) == 1
    assert len({float(ts(f)) for f in range(3000000, 3000006)}) == 6
    assert np.float32(np.float64(ts(381)) - np.float64(ts(501))) == -4          # the pole of 1 / (1 + dt / 4)
    assert np.float32(np.float64(ts(200)) - np.float64(ts(61))) >= 4 and np.float32(np.float64(ts(61)) - np.float64(ts(3))) < 4
    for name, (frames, _) in T.SCHEDULES.items():
        s = T.ring_slots(frames)
        assert len({f % s for f in frames}) == len(frames), name


@pytest.mark.parametrize("name", list(T.SCHEDULES))
def test_ofusion_schedule_enters_its_regime(name):
    recs, stats = T.oracle_schedule(OFUSION, name)
    frames, rate = T.SCHEDULES[name]
    by_frame = {r["frame"]: r for r in recs}
    for f, regime, least in REGIME[name]:
        assert by_frame[f]["regimes"][regime] >= least, (f, regime, by_frame[f]["regimes"])
    for r in recs:
        assert r["ran_i"] == (r["frame"] % rate == 0 or r["frame"] <= 3) and r["ran_r"] == (r["frame"] > 2)
        assert r["node_nans"] == 0 and (r["regimes"] is None or (r["regimes"]["nan"] == 0 and r["regimes"]["updated"] > 100000)), r["frame"]
        assert not r["ran_r"] or (r["n"][..., 0] != -2).sum() > 10000
    assert stats["truncated"] == 0, stats
    if name == "backwards":
        last = recs[-1]["regimes"]
        assert last["plus1000"] > 0 and last["minus1000"] > 0, last
    if name == "three_million":
        assert all(r["regimes"]["dt_eq0"] == 0 and r["regimes"]["dt_lt0"] == 0 for r in recs)
    if name == "rate3":
        assert [r["ran_i"] for r in recs] == [f in (0, 1, 2, 3, 6, 9) for f in frames]
    if name == "rate7":
        assert [r["ran_i"] for r in recs] == [f in (0, 1, 2, 3, 7, 14, 21) for f in frames]


@pytest.mark.parametrize("name", ["gapped", "top_2p32", "rate3", "rate7"])
def test_sdf_schedule_follows_the_gates(name):
    recs, stats = T.oracle_schedule(SDF, name)
    frames, rate = T.SCHEDULES[name]
    for r in recs:
        assert r["ran_i"] == (r["frame"] % rate == 0 or r["frame"] <= 3) and r["ran_r"] == (r["frame"] > 2)
        assert r["node_nans"] == 0 and (r["regimes"] is None or (r["regimes"]["nan"] == 0 and r["regimes"]["updated"] > 10000))
        assert not r["ran_r"] or (r["n"][..., 0] != -2).sum() > 10000
    assert stats["truncated"] == 0, stats


# ------------------------------------------------------------------ the edit lists that depth is fused over, on the oracle alone
EDIT_CASES = [(f, k, N) for f in FIELDS for k in T.EDIT_KINDS] + [(OFUSION, "list", 256)]


@pytest.mark.parametrize("field,kind,n", EDIT_CASES, ids=[f"{FIELD_IDS[f]}_{k}_{n}" for f, k, n in EDIT_CASES])
def test_edit_list_engages(field, kind, n):
    o = T.oracle_fuse_after_edit(field, kind, n)
    first = o["frames"][0]["regimes"]
    print(kind, o["counts"].tolist(), o["info"], first, o["node_written"], o["node_touched"])
    assert o["stats"]["truncated"] == 0
    assert not _same(o["before"], o["edited"])                                            # the edit changed the map
    assert (o["image"][1][..., 0] != -2).sum() > 50                                       # and something is still seen
    for fr in o["frames"]:                                                                 # no NaN is ever stored
        assert fr["regimes"]["nan"] == 0 and fr["node_nans"] == 0, fr["frame"]
        assert (fr["n"][..., 0] != -2).sum() > 10000
    assert np.isnan(o["edited"][1]).sum() == 0 and np.isnan(o["edited"][2]).sum() == 0
    if kind == "reset":
        assert o["counts"][0] > 10000 and o["counts"][1] > 0 and o["counts"][3] == 0
        if field == OFUSION:
            assert first["dt_ge4"] > 10000, first          # y = 0 met at frame 304: the clamp
    if kind == "boxes":
        assert o["counts"][2] == len(o["rec"]) and o["counts"][3] == 0
        ex, ey = o["edited"][1], o["edited"][2]
        for x in (T.SDF_X if field == SDF else T.OF_X):                                    # every value is in the map, sign and denormals kept
            assert (bits(ex) == bits(np.float32(x))).any(), x
        if field == SDF:
            assert all((ey == w).any() for w in T.SDF_Y)
            assert first["weight_fell"] > 100 and first["clamped"] > 100, first
        else:
            assert min(first["dt_ge4"], first["dt_eq0"], first["dt_lt0"], first["pole"], first["clamped"]) > 100, first
            assert first["plus1000"] > 0 and first["minus1000"] > 0
    if kind == "nodes":
        assert o["counts"][0] == 0 and o["counts"][1] > 0 and o["node_touched"] > 0, (o["counts"], o["node_touched"])
    if kind == "list":
        assert len(o["rec"]) >= 200 and o["counts"][0] > 0 and o["counts"][1] > 0 and o["info"]["rewritten"] > 0 and o["info"]["suppressed"] > 0
        assert o["node_touched"] > 0
