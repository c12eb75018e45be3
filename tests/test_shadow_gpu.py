"""GPU: re_shadow_step (ShadowFlow::calculate_shadow_maps on the device) against the restatement of tests/shadow_rule.py, fed from re_visible_lights and
the lighting context's slot ids; light cameras, culler planes and candidate boxes bit-exact against the oracle's camera math."""
import re

import numpy as np
import pytest

import oracle as ro
from shadow_rule import ShadowFlowRule, ShadowPanic, DIRECTIONAL, POINT, SPOT

WINDOW = (1280, 720)
RAD = np.float32(np.pi) / np.float32(180.0)


def rc_of(err):
    return int(re.search(r"failed \((-?\d+)\)", str(err.value)).group(1))


def world(R, seed, spot_only, n=2500):
    from test_lights import lit_world
    ents = lit_world(R, n, seed, 600.0, frac=0.12)
    ents["sortable"] = 0
    if spot_only:                                          # every light a spot light: the machine never locks at Point(Some)
        lit = (ents["flags"] & 0xE000) != 0
        ents["flags"][lit] = (ents["flags"][lit] & ~np.uint32(0xE000)) | np.uint32(R.F_LIGHT_SPOT)
    lights = ents["id"][(ents["flags"] & 0xE000) != 0]
    rng = np.random.default_rng(seed)
    I = np.zeros(len(lights), R.LIGHT_INFORMATION_DT)
    I["radius"] = rng.uniform(60.0, 260.0, len(lights)); I["diffuse"] = 0.5; I["specular"] = 0.5; I["ambient"] = 0.25
    I["linear"] = 0.007; I["quadratic"] = 0.0002; I["cutoff"] = 0.3; I["outer_cutoff"] = -0.2
    I["direction"] = rng.uniform(-1.0, 1.0, (len(lights), 3)); I["direction"][:, 1] -= 1.5; I["fov"] = rng.uniform(30.0, 90.0, len(lights)); I["present"] = 15
    return ents, lights, I


def ortho(l, r, b, t, n, f):
    l, r, b, t, n, f = (np.float32(v) for v in (l, r, b, t, n, f))
    m = np.zeros(16, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        m[0] = np.float32(2) / (r - l); m[5] = np.float32(2) / (t - b); m[10] = np.float32(-2) / (f - n)
        m[12] = -(r + l) / (r - l); m[13] = -(t + b) / (t - b); m[14] = -(f + n) / (f - n); m[15] = 1
    return m


def expected_camera(d, pos, cam_pv, outline=16384):
    """the light camera of a decision of the rule (shadow_flow.rs:175-190, 227-238, 322-330) and what culls its view"""
    pos = np.asarray(pos, np.float32); direction = np.asarray(d["direction"], np.float32); far = np.float32(d["far"])
    view = ro.look_at(pos, pos + direction, d["up"])
    if d["kind"] == "ortho":
        proj = ortho(outline, outline, outline, outline, 0.1, far)
    else:
        aspect = np.float32(d["aspect"]) if "aspect" in d else np.float32(WINDOW[0]) / np.float32(WINDOW[1])
        proj = ro.perspective(aspect, np.float32(d["fov"]) * RAD, np.float32(d["near"]), far)
    lpv = ro.mat4_mul(proj, view)
    culler = lpv if d["type"] == SPOT else np.asarray(cam_pv, np.float32).reshape(16)
    h = far / np.float32(2)
    c = direction * h + pos
    box = np.array([max(c[0] - h, np.float32(0)), c[0] + h, max(c[1] - h, np.float32(0)), c[1] + h, max(c[2] - h, np.float32(0)), c[2] + h], np.float32)
    return lpv, view, culler, ro.make_planes(culler), box


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32).reshape(-1); b = np.ascontiguousarray(b, np.float32).reshape(-1)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def check(R, p, got, want, cam, info_of):
    assert got["new_map"] == (want is not None), (got, want)
    if want is None:
        assert got["entity_id"] == 0xFFFFFFFF
        return
    assert (got["light_type"], got["entity_id"], got["texture_index"]) == (want["type"], want["id"], want["index"])
    assert got["face"] == (want["face"] if want["face"] is not None else 0xFFFFFFFF)
    pos = p.read_component(want["id"], R._capi.C_POSITION)
    lpv, view, culler, planes, box = expected_camera(want, pos, cam.projection_view)
    same_bits(got["light_view"], view); same_bits(got["light_projection_view"], lpv); same_bits(got["culler"], culler)
    same_bits(got["planes"], planes); same_bits(got["box"], box); same_bits(got["position"], pos)
    assert got["far_draw"] == np.float32(info_of(want["id"])["radius"])


def info_fn(lights, I):
    by = {int(e): I[k] for k, e in enumerate(lights)}

    def f(e):
        r = by.get(int(e))
        return None if r is None else {"radius": r["radius"], "direction": tuple(r["direction"]) if r["present"] & 4 else None,
                                       "fov": r["fov"] if r["present"] & 8 else None}
    return f


def run_session(R, seed, spot_only, n_maps, cams, ticks=True):
    from render_engine_amd import lighting, shadow
    ents, lights, I = world(R, seed, spot_only)
    p = R.Pipeline(16384, 64)
    p.register_model_instances(ents); p.set_light_information(lights, I)
    A = lighting.DeferredLighting(32, 16, max_spot_lights=8, max_point_lights=4)
    S = shadow.Shadow(p, n_shadow_maps=n_maps)
    rule = ShadowFlowRule(n_maps); prev = {t: set() for t in range(3)}
    info = info_fn(lights, I)
    flags = (R.F_LIGHT_DIRECTIONAL, R.F_LIGHT_POINT, R.F_LIGHT_SPOT)
    made = {t: 0 for t in range(3)}; freed = 0
    for pos, d, far in cams:
        cam = R.Camera(pos, d, far)
        nearby = {t: set(int(x) for x in p.visible_lights(cam, flags[t])) for t in range(3)}
        n_free = len(rule.free)
        want = rule.step(nearby, prev, info=info)
        freed += max(0, len(rule.free) + (1 if want else 0) - n_free)
        got = S.step(cam, WINDOW, lighting=A)
        check(R, p, got, want, cam, info)
        assert got["n_uploads"] == len(rule.uploads)
        if want:
            made[want["type"]] += 1
        r = A.set_lights_from_world(p, cam, 2)
        for t in range(3):
            if r["n_slots"][t]:
                prev[t] = set(int(x) for x in r["slot_ids"][t])
        p.cull_and_pack(cam)
        if ticks:
            p.tick(0.05)
    m, v, idx = S.uploads(64)
    assert list(idx) == [u[2] for u in rule.uploads][-64:]
    st = p.stats()
    assert st["n_seal_waits"] == 0 and st["n_sync_fallbacks"] == 0
    S.close(); A.close(); p.close()
    return made, freed


def moving_cams(n):
    out = []
    for f in range(n):
        a = f * 0.37
        out.append(((8192.0 + 260.0 * np.cos(a), 8192.0 + 40.0 * np.sin(2 * a), 8192.0 + 260.0 * np.sin(a)), (np.cos(a + 1.0), -0.2, np.sin(a + 1.0)),
                    150.0 + 25.0 * (f % 5)))
    return out


@pytest.mark.gpu
def test_shadow_decisions_spot_lights_round_robin():
    """30 frames of a spot-light world with a moving camera and ticks: six faces per light, the round robin, freeing when lights leave the nearby set"""
    import render_engine_amd as R
    made, freed = run_session(R, 11, True, 24, moving_cams(30))
    assert made[SPOT] >= 12 and freed > 0, (made, freed)


@pytest.mark.gpu
def test_shadow_decisions_mixed_lights_lock_at_point():
    """24 frames with all light types: a point light takes the remaining indexes and the machine stays at Point(Some)"""
    import render_engine_amd as R
    made, _ = run_session(R, 12, False, 6, moving_cams(24))
    assert made[POINT] >= 1, made


@pytest.mark.gpu
def test_shadow_step_without_out_does_not_wait():
    import render_engine_amd as R
    from render_engine_amd import lighting, shadow
    ents, lights, I = world(R, 13, True)
    p = R.Pipeline(16384, 64); p.register_model_instances(ents); p.set_light_information(lights, I)
    A = lighting.DeferredLighting(32, 16, max_spot_lights=8, max_point_lights=4)
    S = shadow.Shadow(p, n_shadow_maps=12)
    for pos, d, far in moving_cams(16):
        cam = R.Camera(pos, d, far)
        S.step(cam, WINDOW, lighting=A, wait=False)
        A.set_lights_from_world(p, cam, 2, wait=False)
        p.cull_and_pack(cam, asynchronous=True)
        p.tick(0.05, asynchronous=True)
    p.wait()
    st = S.stats()
    assert st["n_steps"] == 16 and st["n_host_waits"] == 0, st
    assert st["n_column_uploads"] == 1, st                 # the fov column is rebuilt only when the LightInformation column changes
    _, _, idx = S.uploads(64)
    assert len(idx) > 0
    S.close(); A.close(); p.close()


@pytest.mark.gpu
def test_main_frame_unchanged_by_shadow_steps():
    """the same session with and without shadow steps: byte-identical frame counts, visible sections (with multiplicity), InstanceRange counts per group
    and statistics; the packed instances identical as (id, 64 matrix bytes) per group.  Instance order inside a group is not fixed by the library even
    between two runs of the same session (the scan's cursor atomics, DESIGN.md hash-order quirk (v)), so that order alone is compared as a multiset.
    Static sections whose static set changes in the session exercise the main frozen static cache."""
    import render_engine_amd as R
    from render_engine_amd import lighting, shadow
    from helpers import assert_render_equal
    ents, lights, I = world(R, 14, False)
    static = np.nonzero((ents["flags"] & R.F_STATIC) != 0)[0]
    assert len(static) > 0
    rng = np.random.default_rng(14)
    ch = np.zeros(6, R.CHANGE_DT)                          # wake up some static entities and make some dynamic ones static: the cache's snapshot semantics
    ch["kind"][:3] = R._capi.CHANGE_WAKE_UP; ch["entity_id"][:3] = ents["id"][rng.choice(static, 3, replace=False)]
    dyn = np.nonzero((ents["flags"] & R.F_STATIC) == 0)[0]
    ch["kind"][3:] = R._capi.CHANGE_MAKE_STATIC; ch["entity_id"][3:] = ents["id"][rng.choice(dyn, 3, replace=False)]
    res = []
    for with_shadow in (False, True):
        p = R.Pipeline(16384, 64); p.register_model_instances(ents); p.set_light_information(lights, I)
        A = lighting.DeferredLighting(32, 16, max_spot_lights=8, max_point_lights=4)
        S = shadow.Shadow(p) if with_shadow else None
        frames = []
        for f, (pos, d, far) in enumerate(moving_cams(10)):
            cam = R.Camera(pos, d, far)
            if S:
                S.step(cam, WINDOW, lighting=A)
            A.set_lights_from_world(p, cam, 2)
            r = p.cull_and_pack(cam)
            frames.append((r, p.visible_sections()))
            if f == 3:
                p.apply_changes(ch)
            p.tick(0.05)
        res.append((frames, p.stats()))
        if S:
            S.close()
        A.close(); p.close()
    key = lambda g: np.sort(g, order=["model_index", "render_system", "sortable"])   # noqa: E731
    for (a, va), (b, vb) in zip(res[0][0], res[1][0]):
        assert a["total"] == b["total"]
        assert va[0].tobytes() == vb[0].tobytes() and va[1].tobytes() == vb[1].tobytes()
        np.testing.assert_array_equal(key(a["groups"])[["model_index", "render_system", "sortable", "count"]],
                                      key(b["groups"])[["model_index", "render_system", "sortable", "count"]])
        assert_render_equal(b, a)
    assert res[0][1] == res[1][1]


@pytest.mark.gpu
def test_shadow_step_rejects_reserved_flags():
    import ctypes as C
    import render_engine_amd as R
    from render_engine_amd import shadow
    ents, lights, I = world(R, 16, True)
    p = R.Pipeline(16384, 64); p.register_model_instances(ents); p.set_light_information(lights, I)
    S = shadow.Shadow(p)
    cam = R.Camera((8192.0, 8192.0, 8192.0), (0.0, 0.0, -1.0), 300.0).to_c()
    args = R._capi.ShadowArgs(*WINDOW)
    assert R._capi.load().re_shadow_step(S._h, None, C.byref(cam), C.byref(args), 1, None) == -1
    assert S.stats()["n_steps"] == 0
    S.close(); p.close()


@pytest.mark.gpu
def test_shadow_errors():
    import render_engine_amd as R
    from render_engine_amd import shadow
    ents, lights, I = world(R, 15, True)
    # a spot light the machine chooses without LightInformation: RE_E_STATE naming it, the state unchanged
    p = R.Pipeline(16384, 64); p.register_model_instances(ents); p.set_light_information(lights, I)
    S = shadow.Shadow(p)
    cam = R.Camera((8192.0, 8192.0, 8192.0), (0.0, 0.0, -1.0), 300.0)
    assert not S.step(cam, WINDOW)["new_map"] and not S.step(cam, WINDOW)["new_map"]      # directional -> point -> spot
    near = p.visible_lights(cam, R.F_LIGHT_SPOT)
    assert len(near) > 0
    first = int(near[0])                                     # no visible sets: the first nearby light
    p.set_light_information([first], None)
    with pytest.raises(R.RenderEngineError) as e:
        S.step(cam, WINDOW)
    assert rc_of(e) == -5 and str(first) in str(e.value)
    p.set_light_information([first], I[list(lights).index(first)])
    f = S.step(cam, WINDOW)
    assert (f["entity_id"], f["face"], f["texture_index"]) == (first, 0, 0)
    S.close()
    # a sharded context
    p.set_shard_range(0, 1 << 40)
    S = shadow.Shadow(p)
    with pytest.raises(R.RenderEngineError) as e:
        S.step(cam, WINDOW)
    assert rc_of(e) == -6
    S.close(); p.close()
    # a directional light (sortable index 1): six indexes, then RE_E_STATE on the seventh frame, and again on the eighth
    ents2 = ents.copy(); k = int(np.nonzero(ents2["id"] == lights[0])[0][0]); ents2["sortable"][k] = 1
    p = R.Pipeline(16384, 64); p.register_model_instances(ents2); p.set_light_information(lights, I)
    S = shadow.Shadow(p)
    for i in range(6):
        f = S.step(cam, WINDOW)
        assert (f["light_type"], f["entity_id"], f["texture_index"]) == (DIRECTIONAL, int(lights[0]), i)
        want = dict(type=DIRECTIONAL, kind="ortho", direction=tuple(I[0]["direction"]), up=(0.0, 1.0, 0.0), far=I[0]["radius"])
        lpv, view, culler, planes, box = expected_camera(want, p.read_component(int(lights[0]), R._capi.C_POSITION), cam.projection_view)
        same_bits(f["light_view"], view); same_bits(f["planes"], planes); same_bits(f["box"], box)
        np.testing.assert_array_equal(f["light_projection_view"], lpv)   # ortho with left == right, top == bottom: inf / NaN entries
    for _ in range(2):
        with pytest.raises(R.RenderEngineError) as e:
            S.step(cam, WINDOW)
        assert rc_of(e) == -5 and str(int(lights[0])) in str(e.value)
    S.close(); p.close()
