"""CPU: the C ABI records of the from-world light upload, and the restatement of the reference's upload rule (tests/world_lights_rule.py) that the GPU
tests of re_lighting_set_lights_from_world compare against."""
import ctypes as C

import numpy as np

from world_lights_rule import RenderSystemLights, upload_slots


def test_record_layouts_match_header():
    import render_engine_amd as R
    from render_engine_amd import _capi
    assert C.sizeof(_capi.LightInformation) == 80 and R.LIGHT_INFORMATION_DT.itemsize == 80
    for f in ("radius", "diffuse", "specular", "ambient", "linear", "quadratic", "cutoff", "outer_cutoff", "direction", "fov", "present"):
        assert getattr(_capi.LightInformation, f).offset == R.LIGHT_INFORMATION_DT.fields[f][1], f
    assert _capi.LightInformation.present.offset == 76 and _capi.LightInformation.direction.offset == 60
    assert C.sizeof(_capi.WorldLightArgs) == 12
    assert C.sizeof(_capi.WorldLights) == 32 + 3 * 8 and _capi.WorldLights.slot_ids.offset == 32
    assert (_capi.C_LIGHT_INFORMATION, _capi.ECS_BIT["LIGHT_INFORMATION"]) == (11, 19)
    L = _capi.load()
    assert L.re_abi_version() == 3
    assert hasattr(L, "re_set_light_information") and hasattr(L, "re_lighting_set_lights_from_world")


def test_rule_known_answer():
    slots, prev = upload_slots({3, 7}, [1, 3, 5, 7, 9], 4)
    assert slots == [3, 7, 1, 3] and prev == {1, 3, 7}
    slots, prev = upload_slots(set(), [4, 8], 16)                   # N = |nearby| below the maximum
    assert slots == [4, 8] and prev == {4, 8}
    slots, prev = upload_slots({2, 4, 6}, [2, 4, 6, 8], 2)          # the existing part alone fills the slots
    assert slots == [2, 4] and prev == {2, 4}


def info(k):
    return dict(radius=10.0 + k, diffuse=[0.1 * k, 0.2, 0.3], specular=[0.3, 0.2, 0.1], ambient=[0.5, 0.5, 0.5, 0.25], linear=0.01, quadratic=0.001,
                cutoff=0.3, outer_cutoff=-0.2, direction=[0.0, -1.0, 0.0], fov=45.0)


def test_rule_keeps_a_type_without_nearby_lights():
    rs = RenderSystemLights(2, 4, 8)
    pos = lambda e: np.array([e, 2 * e, 3 * e], np.float32)
    slots, anyv = rs.frame([[], [5, 6], [1, 2, 3]], pos, info, (0, 0, 0))
    assert anyv and slots == [None, [5, 6], [1, 2, 3]]
    spot_before = rs.arrays["spot_pos"].copy()
    slots, anyv = rs.frame([[], [6, 7], []], pos, info, (1, 1, 1))
    assert anyv and slots[0] is None and slots[2] is None and slots[1] == [6, 6]      # 6 was taken last frame: it leads, and comes again
    assert rs.previous[2] == {1, 2, 3}                               # not cleared
    np.testing.assert_array_equal(rs.arrays["spot_pos"], spot_before)   # the arrays of last frame stay in force
    slots, anyv = rs.frame([[], [], []], pos, info, (1, 1, 1))
    assert not anyv and rs.arrays["any_light_source_visible"] == 0 and rs.arrays["n_point"] == 2


def test_rule_fills_every_spot_slot():
    rs = RenderSystemLights(1, 1, 6)
    pos = lambda e: np.array([e, e, e], np.float32)
    rs.frame([[], [], [10, 11]], pos, info, (0, 0, 0))
    A = rs.arrays
    assert A["n_spot"] == 6 and len(A["spot_pos"]) == 6                 # numberSpotLights = max_spot_lights
    np.testing.assert_array_equal(A["spot_pos"][:2], [[10, 10, 10], [11, 11, 11]])
    for f in ("spot_pos", "spot_diffuse", "spot_specular", "spot_ambient", "spot_linear", "spot_quadratic", "spot_radius"):
        assert not np.any(A[f][2:]), f
