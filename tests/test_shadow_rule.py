"""CPU: known answers of the restated shadow flow (tests/shadow_rule.py), worked out by hand from flows/shadow_flow.rs, and the layout of the re_shadow_* structs."""
import ctypes as C

import pytest

from shadow_rule import ShadowFlowRule, ShadowPanic, DIRECTIONAL, POINT, SPOT

E = set()


def sets(point=(), spot=()):
    return {DIRECTIONAL: set(), POINT: set(point), SPOT: set(spot)}


def test_one_directional_light_pops_every_frame_then_panics():
    R = ShadowFlowRule(6)
    for k in range(6):
        d = R.step(sets(), sets(), dir_candidates=[7])
        assert (d["type"], d["id"], d["index"], d["kind"]) == (DIRECTIONAL, 7, k, "ortho")
    with pytest.raises(ShadowPanic) as e:
        R.step(sets(), sets(), dir_candidates=[7])
    assert e.value.entity_id == 7
    with pytest.raises(ShadowPanic):                      # the state was left as it was: the same frame fails again
        R.step(sets(), sets(), dir_candidates=[7])


def test_directional_takes_the_smallest_candidate():
    R = ShadowFlowRule(6)
    assert R.step(sets(), sets(), dir_candidates=[9, 4, 12])["id"] == 4


def test_point_light_locks_the_machine():
    R = ShadowFlowRule(6)
    assert R.step(sets(point=[3]), sets()) is None        # Directional(None) without candidates -> Point(None)
    got = [R.step(sets(point=[3]), sets()) for _ in range(6)]
    assert [(d["type"], d["id"], d["index"]) for d in got] == [(POINT, 3, k) for k in range(6)]
    for _ in range(10):                                   # the queue is empty: NoNewMapRequired for ever, Point(Some(3)) stays
        assert R.step(sets(point=[3], spot=[5]), sets(spot=[5])) is None
    assert (R.type, R.cur) == (POINT, 3) and R.maps[POINT] == {3: [None] * 6}


def test_spot_six_faces_round_robin_and_freeing():
    R = ShadowFlowRule(8)
    assert R.step(sets(spot=[2, 5]), sets()) is None      # directional -> point
    assert R.step(sets(spot=[2, 5]), sets()) is None      # no point light -> spot
    faces = [R.step(sets(spot=[2, 5]), sets()) for _ in range(6)]
    assert [(d["type"], d["id"], d["face"], d["index"]) for d in faces] == [(SPOT, 2, f, f) for f in range(6)]
    assert [d["direction"] for d in faces][3] == (1.0, 0.0, 0.0) and faces[4]["up"] == (0.0, 0.0, 1.0)
    assert R.uploads == [(2, f, f) for f in range(6)]
    assert R.step(sets(spot=[2, 5]), sets()) is None      # six faces done -> Directional(None)
    assert R.type == DIRECTIONAL and R.cur is None
    assert R.step(sets(spot=[5]), sets()) is None         # directional (two free indexes, no candidates) -> point
    assert R.step(sets(spot=[5]), sets()) is None         # point -> spot
    d = R.step(sets(spot=[5]), sets())                    # light 2 left the nearby set: its six indexes go back behind 6, 7
    assert (d["id"], d["face"], d["index"]) == (5, 0, 6)
    assert list(R.free) == [7, 0, 1, 2, 3, 4, 5] and 2 not in R.maps[SPOT]


def test_priority_is_the_largest_visible_light_without_a_map():
    R = ShadowFlowRule(6)
    R.step(sets(), sets()); R.step(sets(), sets())
    d = R.step(sets(spot=[1, 4, 9]), sets(spot=[1, 4, 9]))
    assert (d["id"], d["face"]) == (9, 0)


def test_fallback_is_the_first_nearby_light_that_is_not_visible():
    R = ShadowFlowRule(12)
    R.step(sets(), sets()); R.step(sets(), sets())
    for f in range(6):                                    # light 4 (visible) gets its six faces
        assert R.step(sets(spot=[1, 4, 9]), sets(spot=[4]))["id"] == 4
    assert R.step(sets(spot=[1, 4, 9]), sets(spot=[4])) is None
    R.step(sets(spot=[1, 4, 9]), sets(spot=[4])); R.step(sets(spot=[1, 4, 9]), sets(spot=[4]))
    d = R.step(sets(spot=[1, 4, 9]), sets(spot=[4]))      # every visible light has a map: the first nearby one that is not visible
    assert (d["id"], d["index"]) == (1, 6)


def test_missing_light_information_panics_and_keeps_the_state():
    R = ShadowFlowRule(6)
    R.step(sets(), sets()); R.step(sets(), sets())
    with pytest.raises(ShadowPanic) as e:
        R.step(sets(spot=[3]), sets(), info=lambda x: None)
    assert e.value.entity_id == 3 and R.cur is None and R.type == SPOT and list(R.free) == list(range(6))


def test_shadow_struct_layouts():
    from render_engine_amd import _capi
    assert C.sizeof(_capi.ShadowFrame) == 352
    assert C.sizeof(_capi.ShadowConfig) == 8 and C.sizeof(_capi.ShadowArgs) == 8 and C.sizeof(_capi.ShadowStats) == 12
    off = {f: getattr(_capi.ShadowFrame, f).offset for f, _ in _capi.ShadowFrame._fields_}
    assert off["n_uploads"] == 20 and off["light_projection_view"] == 24 and off["light_view"] == 88 and off["culler"] == 152
    assert off["planes"] == 216 and off["box"] == 312 and off["position"] == 336 and off["far_draw"] == 348
    for s in ("re_shadow_create", "re_shadow_destroy", "re_shadow_last_error", "re_shadow_step", "re_shadow_uploads", "re_shadow_get_stats"):
        assert s in _capi.EXPORTS
