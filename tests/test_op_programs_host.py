"""The model of tests/op_program_util.py on its own, without a GPU: (a) an oracle seeded from a snapshot goes on exactly like the oracle the
snapshot came from; (b) every program of the table engages what it is there for -- conditions, not measurements; (c) the seeded random
programs are stable.  tests/test_gpu_op_programs.py runs the same programs on the device beside this model."""
import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF
from tests import op_program_util as P
from tests.gpu_state_util import bits

FIELDS = [SDF, OFUSION]
FIELD_IDS = ["sdf", "ofusion"]


def _same_state(a, b):
    for u, w in zip(a, b):
        if u.shape != w.shape or not ((bits(u) == bits(w)).all() if u.dtype.kind == "f" else (u == w).all()):
            return False
    return True


# ------------------------------------------------------------------ (a) the splice
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_a_seeded_oracle_goes_on_like_the_one_its_snapshot_came_from(field):
    base = P.base_frame(field)
    a, b = P.Model(field), P.Model(field)
    try:
        for i in range(4):
            a.frame(i, base + i)
        st = a.state()
        assert st[3].min() == 0 and st[3].max() == 1          # some blocks are inactive: the seeded oracle holds them active until its first sweep
        b.seed(st[:4], st[4:])
        b.last = a.last
        assert _same_state(st, b.state())
        for u, w in zip(a.raycast()[1:], b.raycast()[1:]):
            assert (bits(u) == bits(w)).all()
        for i in range(4, 8):
            ra, rb = a.frame(i, base + i), b.frame(i, base + i)
            assert ra[0] and rb[0] and (ra[2][..., 0] != -2).sum() >= 50
            assert (bits(ra[1]) == bits(rb[1])).all() and (bits(ra[2]) == bits(rb[2])).all(), i
            assert _same_state(a.state(), b.state()), i
        assert a.stats_truncated() == 0 and b.stats_truncated() == 0
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_a_map_whose_first_octant_is_a_childless_node_can_be_seeded(field):
    """Octree::allocate would walk the list's smallest key down along child 0 to a block (the keys[0] rule of unique_multiscale); the
    device's shift, merge, allocation and load create no such chain, so the model seeds with Octree::insert."""
    m = P.Model(field)
    try:
        _, counts = m.allocate([((0, 0, 0), (32, 32, 32), 2), ((64, 64, 64), (72, 72, 72), 0)])
        assert counts.tolist() == [1, 2 + 3, 2, 0] and m.counts() == (1, 6)          # root; (0,0,0) of levels 1, 2; (64,64,64) of levels 1 .. 3; one block
        st = m.state()
        m.seed(st[:4], st[4:])
        assert _same_state(st, m.state())
    finally:
        m.close()


# ------------------------------------------------------------------ (b) every program engages
CASES = [(name, f) for name in P.PROGRAMS for f in FIELDS]


@pytest.mark.parametrize("name,field", CASES, ids=[f"{n}-{FIELD_IDS[f]}" for n, f in CASES])
def test_every_program_engages(name, field):
    recs, summary = P.model_run(name, field)
    steps = P.PROGRAMS[name][1]
    print(name, FIELD_IDS[field], P.figures(recs, summary))
    releases, has_all = [], False
    assert len(recs) == len(steps) <= 14 and [r["kind"] for r in recs] == [s[0] for s in steps]
    assert steps[-1] == ("frame",) and steps[-2] == ("frame",)
    seen = set()
    for j, r in enumerate(recs):
        o = r["inner"] if r["kind"] == "staged" else r
        seen |= {r["kind"], o["kind"]}
        if o["kind"] == "shift":
            assert o["counts"][0] > 0 and o["counts"][1] > 0, (j, o["counts"])
            assert o["flags_before"] == (0, 1), (j, o["flags_before"])
            if o.get("node64"):
                assert all(v % 64 == 0 for v in o["s"]) and o["counts"][2] > 0
        elif o["kind"] == "merge":
            assert o["counts"][1] > 0, (j, o["counts"])
            if o["mode"] != "replace":
                assert o["both_observed"] > 0, j
        elif o["kind"] == "edit":
            assert o["counts"][0] + o["counts"][1] > 0 and o["counts"][3] == 0, (j, o["counts"])
        elif o["kind"] == "allocate":
            assert o["counts"][0] > 0 and o["counts"][3] == 0, (j, o["counts"])
        elif o["kind"] == "release":
            kept, released, nodes_kept, nodes_released, observed = (int(v) for v in o["counts"][:5])
            assert released > 0, (j, o["counts"])
            if any(what == "all" for _, _, what in o["rows"]):
                has_all = True
                assert observed > 0, (j, o["counts"])
            if r["kind"] == "staged":                           # the "unseen" release takes blocks the scan had just created with it
                assert o["fresh_released"] > 0, (j, o["fresh_released"])
            releases.append((nodes_released, o["info"]["reset_valued"]))
        elif o["kind"] == "merge_rigid":
            combined, created, observed, both = (int(v) for v in o["counts"][:4])
            assert created > 0 and combined > 0 and observed > 0, (j, o["counts"])
            if o["mode"] != "replace":
                assert both > 0, (j, o["counts"])
        for kind, changed in r.get("changed_inside", []):
            assert changed > 0, (j, kind)                       # the frame after an operation meets what the operation touched
        if r["image"][0] and (r["kind"] in ("frame", "staged") or r["fused_before"]):
            assert r["hits"] >= 50, (j, r["hits"])
        if r["kind"] in ("frame", "staged"):
            assert r["image"][0] == (r["number"] > 2)
    assert seen == P.kinds_of(steps)
    assert summary["truncated"] == 0
    if name in ("pool_churn", "pool_churn_release"):
        assert summary["created"] > P.POOL >= summary["peak"], summary
    # a program that forgets observed content hands nodes back and resets a parent entry that held a value, at least once.  (Under an
    # "unseen" release alone both depend on what the scans happened to leave empty: a node goes only if all eight entries are initValue()
    # and everything beneath it is empty, and the entry above an empty block holds a value only if it was written before the block came.)
    if has_all:
        assert any(n > 0 for n, _ in releases) and any(v > 0 for _, v in releases), releases
    _reader_conditions(name, field, recs)


def _reader_conditions(name, field, recs):
    truths = [r["readers"] for r in recs if "readers" in r]
    if not truths:                                              # the staged programs: every operation stands inside a frame
        assert all(r["kind"] in ("frame", "staged") for r in recs)
        return
    fig = P.reader_figures(truths)
    print(name, FIELD_IDS[field], "readers", fig)
    assert fig["project"] == {0, 1, 2}, fig["project"]
    assert min(fig["field"].values()) > 0, fig["field"]
    assert min(fig["t_first"].values()) > 0, fig["t_first"]
    assert fig["oriented"] == {0, 1, 2}, fig["oriented"]
    assert fig["rays"]["hits"] >= 50 and fig["rays"]["entered_missed"] >= 1, fig["rays"]
    assert fig["query"]["allocated"] > 0 and fig["query"]["unallocated"] > 0, fig["query"]


def test_the_table_holds_every_step_kind_in_every_position():
    kinds, staged = set(), set()
    for _, steps in P.PROGRAMS.values():
        kinds |= P.kinds_of(steps)
        staged |= {s[1][0] for s in steps if s[0] == "staged"}
    assert kinds == set(P.STEP_KINDS) == {"frame", "shift", "merge", "allocate", "edit", "save_load", "staged", "release", "merge_rigid"}
    assert staged == {"edit", "allocate", "shift", "merge", "release", "merge_rigid"}
    assert all(purpose and "\n" not in purpose for purpose, _ in P.PROGRAMS.values())


# ------------------------------------------------------------------ (c) the random programs are stable
def test_random_programs_are_stable():
    for name, seed in P.RANDOM_SEEDS.items():
        a, b = P.random_program(seed), P.random_program(seed)
        assert a == b == P.PROGRAMS[name][1] and len(a) <= 14 and a[-2:] == [("frame",), ("frame",)]
    assert P.PROGRAMS["random_a"][1] != P.PROGRAMS["random_b"][1]
    every = P.OLD_KINDS + ("release", "merge_rigid")
    for name, seed in P.RANDOM_SEEDS_ALL.items():
        a, b = P.random_program(seed, every), P.random_program(seed, kinds=every)
        assert a == b == P.PROGRAMS[name][1] and len(a) <= 14 and a[-2:] == [("frame",), ("frame",)]
        assert {"release", "merge_rigid"} & P.kinds_of(a)
    assert P.PROGRAMS["random_c"][1] != P.PROGRAMS["random_d"][1]


def _kinds(steps):
    return [s[0] if s[0] != "staged" else "staged:" + s[1][0] for s in steps]


def test_the_programs_of_before_are_the_same():
    """The step lists of the eight programs that existed before the release and the rigid merge became step kinds: their kinds, literally."""
    f = "frame"
    want = {
        "rolling_submap": [f, f, f, f, "shift", f, f, "merge", f, "edit", "shift", f, f],
        "declare_free": ["allocate", "edit", f, f, f, f, "edit", "merge", f, "shift", "allocate", "edit", f, f],
        "merge_first": ["merge", f, "shift", "merge", f, f, f, "save_load", f, f],
        "pool_churn": [f, f, "allocate", f, "shift", "merge", "allocate", f, "shift", "merge", "allocate", f, f],
        "staged_edit_allocate": [f, f, f, f, "staged:edit", f, "staged:allocate", f, f],
        "staged_shift_merge": [f, f, f, f, "staged:shift", f, "staged:merge", f, f],
        "random_a": [f, f, f, "merge", f, "save_load", f, "allocate", f, "edit", f, f, f],
        "random_b": [f, f, f, "staged:edit", "allocate", f, "edit", f, "shift", f, f, f],
    }
    assert {n: _kinds(P.PROGRAMS[n][1]) for n in want} == want
    box = [((40, 48, 24), (88, 80, 56), 0)]
    assert [s for s in P.PROGRAMS["random_a"][1] if s != ("frame",)] == [
        ("merge", "src64", ("registered", (8, 0, -8)), "fuse"), ("save_load",), ("allocate", box), ("edit", "reset")]
    assert [s for s in P.PROGRAMS["random_b"][1] if s != ("frame",)] == [
        ("staged", ("edit", "boxes")), ("allocate", box), ("edit", "boxes"), ("shift", (0, 8, 8))]


def test_the_numpy_class_grid_reads_nodes_where_blocks_are_absent():
    """class_grid on a hand-made state: one occupied block, one childless node with two values, the rest unseen."""
    m = P.Model(SDF)
    try:
        m.allocate([((32, 32, 32), (48, 48, 48), 3), ((64, 64, 64), (72, 72, 72), 0)])
        c, x, y, a, code, side, nx, ny = m.state()
        x, y, nx, ny = x.copy(), y.copy(), nx.copy(), ny.copy()
        x[0, :], y[0, :] = -0.5, 1.0                                               # the block: occupied
        k = int(np.nonzero(side == 16)[0][0])
        nx[k, 1], ny[k, 1], nx[k, 6], ny[k, 6] = -0.25, 2.0, 0.5, 2.0               # child 1 (x high): occupied; child 6 (y, z high): empty
        g = P.class_grid(SDF, 128, (c, x, y, a, code, side, nx, ny))
        assert (g[64:72, 64:72, 64:72] == 0).all() and (g[32:40, 32:40, 40:48] == 0).all() and (g[40:48, 40:48, 32:40] == 2).all()
        assert (g == 0).sum() == 2 * 512 and (g == 2).sum() == 512
        boxes = np.array([[60, 60, 60, 5, 5, 5], [60, 60, 60, 4, 4, 4], [33, 41, 41, 3, 3, 3], [-2, 0, 0, 3, 3, 3]], np.int32)
        assert P.collides_truth(g, boxes).tolist() == [0, 1, 2, 1] and P.collides_truth(g, np.array([[32, 40, 40, 8, 8, 8]])).tolist() == [2]
    finally:
        m.close()
