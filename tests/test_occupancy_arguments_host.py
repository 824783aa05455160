"""The occupancy test's arguments, host side (no GPU): every entry of DenseSLAMPipeline that classifies voxels -- collides, collides_moving,
collides_oriented, clearance, project, distance_field, reach_field, edit -- turns threshold / occupied_above / stop_at into what the library
receives by one rule, and refuses the same things before it calls the library.  One table over the entries, a recorder in the library's place."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, _CollideTest
from tests.host_util import bare_pipeline

BOXES = np.array([[0, 0, 0, 4, 4, 4], [8, 8, 8, 1, 2, 3]], np.int32)
MOTIONS = np.array([[0, 0, 0, 4, 4, 4, 5, -6, 7]], np.int32)
ORIENTED = np.array([[64, 64, 64, 16, 0, 0, 0, 16, 0, 0, 0, 16]], np.int32)
REGION = dict(lo=(0, 0, 0), side=(4, 3, 2))


def _stop_of_request(args):
    return next(a._obj.stop_at for a in args if hasattr(getattr(a, "_obj", None), "stop_at"))


def _stop_after_test(args):
    at = next(i for i, a in enumerate(args) if isinstance(getattr(a, "_obj", None), _CollideTest))
    return args[at + 1]


# entry -> (the call with good arguments, the host entry it reaches, where stop_at arrives -- None: the entry takes none)
ENTRIES = {
    "collides": (lambda p, **kw: p.collides(BOXES, **kw), "se_hip_collide_boxes_host", None),
    "collides_moving": (lambda p, **kw: p.collides_moving(MOTIONS, **kw), "se_hip_collide_motions_host", _stop_after_test),
    "collides_oriented": (lambda p, **kw: p.collides_oriented(ORIENTED, **kw), "se_hip_collide_oriented_host", None),
    "clearance": (lambda p, **kw: p.clearance(BOXES, 4, **kw), "se_hip_clearance_boxes_host", _stop_after_test),
    "project": (lambda p, **kw: p.project(2, (0, 0), (4, 3), [(0, 8)], **kw), "se_hip_project_columns_host", _stop_of_request),
    "distance_field": (lambda p, **kw: p.distance_field(r_max=3, **REGION, **kw), "se_hip_distance_field_host", _stop_of_request),
    "reach_field": (lambda p, **kw: p.reach_field(seeds=[(1, 1, 1)], **REGION, **kw), "se_hip_reach_field_host", _stop_of_request),
    "edit": (lambda p, **kw: p.edit(BOXES, 1.0, **kw), "se_hip_edit_boxes_host", None),
}
WITH_STOP = [k for k, v in ENTRIES.items() if v[2] is not None]


class _Recorder:
    """Stands in for libse_hip.so: keeps the name and the arguments of the one call made."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(h, *args):
            self.calls.append((name, args))
            return 0
        return entry


def _recorded(entry, field, **kw):
    """(the se_hip_collide_test the library received, the other arguments) of one good call of `entry` on a handle of `field`."""
    call, host_entry, _ = ENTRIES[entry]
    p = bare_pipeline(field=field, _device=0)
    p.lib = _Recorder()
    call(p, **kw)
    assert [name for name, _ in p.lib.calls] == [host_entry]
    args = p.lib.calls[0][1]
    tests = [a._obj for a in args if isinstance(getattr(a, "_obj", None), _CollideTest)]
    assert len(tests) == 1
    return tests[0], args


@pytest.mark.parametrize("threshold", [float("nan"), float("inf"), 1e39], ids=["nan", "inf", "beyond_float32"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_threshold_that_is_not_finite_as_a_float32_is_refused(entry, threshold):
    with pytest.raises(ValueError, match=entry + ": threshold"):          # (bare_pipeline: a library call would be an AssertionError)
        ENTRIES[entry][0](bare_pipeline(field=SDF, _device=0), threshold=threshold)


@pytest.mark.parametrize("above", [2, "yes"], ids=["int", "str"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_an_occupied_above_that_is_no_bool_is_refused(entry, above):
    with pytest.raises(TypeError, match=entry + ": occupied_above"):
        ENTRIES[entry][0](bare_pipeline(field=SDF, _device=0), occupied_above=above)


@pytest.mark.parametrize("entry", ENTRIES)
def test_occupied_above_defaults_by_field_and_the_threshold_arrives(entry):
    for field, default in ((SDF, 0), (OFUSION, 1)):
        t, _ = _recorded(entry, field)
        assert (t.threshold, t.occupied_above) == (0.0, default)
        t, _ = _recorded(entry, field, occupied_above=None)
        assert t.occupied_above == default
        for above in (False, True, np.bool_(True)):
            t, _ = _recorded(entry, field, threshold=0.3, occupied_above=above)
            assert (t.threshold, t.occupied_above) == (C.c_float(0.3).value, int(above))


@pytest.mark.parametrize("stop_at", ["empty", 0, None], ids=["empty", "code", "none"])
@pytest.mark.parametrize("entry", WITH_STOP)
def test_a_stop_at_that_names_no_class_is_refused(entry, stop_at):
    with pytest.raises(ValueError, match=entry + ": stop_at"):
        ENTRIES[entry][0](bare_pipeline(field=SDF, _device=0), stop_at=stop_at)


@pytest.mark.parametrize("entry", WITH_STOP)
def test_stop_at_arrives_as_its_status_code(entry):
    where = ENTRIES[entry][2]
    assert where(_recorded(entry, SDF)[1]) == 0                                  # the default: "occupied"
    for name, code in (("occupied", 0), ("unseen", 1)):
        assert where(_recorded(entry, SDF, stop_at=name)[1]) == code
