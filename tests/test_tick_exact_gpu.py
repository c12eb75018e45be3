"""The device's tick (k_tick / tick_body / place_core), registration transform (k_transform_assign) and sin/cos (sincos_det) against the float64
rule of kinematics_ref.py, and its section decision on exact section edges against the answers written out in test_kinematics_ref.py -- by the
tick's path (with its stays-in-its-section short cut) and by the change-request path (k_apply_rows, the full decision), in worlds with a
power-of-two and with a non-power-of-two atomic length.  The inputs, bounds and answers are those of the CPU tests, fixed there on the oracle."""
import numpy as np
import pytest

import oracle as ro
import kinematics_ref as K
from helpers import to_oracle, oracle_camera
from test_gpu_parity import R, build_pair, check_frame, check_sections, check_entities, assert_clean_publication  # noqa: F401  (R: fixture)
from test_kinematics_ref import WORLDS, edge_answers

pytestmark = pytest.mark.gpu
F32 = np.float32
DEAD = 0x80000000


def device_state(R, p, body):
    """the components of one entity as the device holds them, in the shape kinematics_ref.check_body reads"""
    C = R._capi
    out = dict(pos=p.read_component(body.id, C.C_POSITION), mat=p.read_component(body.id, C.C_TRANSFORMATION), aabb=p.read_component(body.id, C.C_STATIC_AABB),
               flags=int(p.read_component(body.id, C.C_FLAGS)[0]))
    for has, comp, key in ((body.has_vel, C.C_VELOCITY, "vel"), (body.has_rot, C.C_ROTATION, "rot"), (body.has_rotvel, C.C_ROTATION_VEL, "rotvel")):
        if has:
            out[key] = p.read_component(body.id, comp)
        else:
            with pytest.raises(R.RenderEngineError):
                p.read_component(body.id, comp)
    return out


def show(measured):
    print(", ".join(f"{key} {v:.3g}" for key, v in sorted(measured.items())))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. sin/cos read from the device
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_device_sincos(R):
    """static entities with a Rotation about (0, 0, 1) or (0, 0, 3) and no Scale, one per level-0 section: m[0] = cos, m[1] = sin, m[4] = -sin,
    m[5] = cos of the angle.  Bounds as on the CPU; bit equality with the oracle's ro_sincosf for every argument."""
    small, high, beyond = K.sincos_arguments(n_uniform=700, kmax=200, n_mid=500, n_high=400, n_beyond=200)
    x = np.concatenate([small, high, beyond])
    for must in (999999.9, 1e6, np.nextafter(F32(1e6), F32(np.inf)), 0.0, 1e-45, 1e-30):
        assert F32(must) in x
    assert 2900 <= len(x) <= 3100 and len(beyond) == 200
    n = len(x)
    e = K.blank_entities(n)
    e["id"] = np.arange(n); e["flags"] = K.F_STATIC | K.F_HAS_ROT
    e["original"][:] = (-1, 1, -1, 1, -1, 1)
    i = np.arange(n)
    e["pos"] = np.stack([120 + i % 15, 120 + (i // 15) % 15, 120 + i // 225], axis=1) * 64 + 32
    e["rot_axis"][:] = (0, 0, 1); e["rot_axis"][1::2] = (0, 0, 3)
    e["rot_angle"] = x
    p = R.Pipeline(16384, 64)
    assert p.register_model_instances(e) == 0
    m = np.stack([p.read_component(int(k), R._capi.C_TRANSFORMATION) for k in range(n)])
    p.close()
    s, c = m[:, 1].copy(), m[:, 0].copy()
    np.testing.assert_array_equal(m[:, 5], c); np.testing.assert_array_equal(m[:, 4], -s)
    np.testing.assert_array_equal(m[:, 12:15], e["pos"])
    measured = K.check_sincos(x, s, c)
    show(measured)
    want = np.array([ro.sincos(v) for v in x], F32)
    zero = x == 0                                                    # a rotation by +-0 is the identity: sin reads +0 where ro_sincosf(-0) is -0
    np.testing.assert_array_equal(s[~zero].view(np.uint32), want[~zero, 0].view(np.uint32))
    np.testing.assert_array_equal(c[~zero].view(np.uint32), want[~zero, 1].view(np.uint32))
    assert np.all(s[zero] == 0) and np.all(c[zero] == 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. registration
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_device_registration_against_the_rule(R):
    ents = K.random_bodies(256, seed=17)
    p = R.Pipeline(16384, 64)
    assert p.register_model_instances(ents) == 0
    measured = {}
    for r in ents:
        b = K.Body(r)
        K.check_body(device_state(R, p, b), b, 0, measured, "device")
    show(measured)
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. three ticks of the 96-entity world, and of entities that become dynamic after the upload
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_three_ticks(R, p, bodies, expect_changed):
    cam = R.Camera(K.WORLD96_CAMERA["position"], K.WORLD96_CAMERA["direction"], K.WORLD96_CAMERA["far"])
    dt = float(F32(K.WORLD96_DT))
    measured = {}
    sections = p.sections()
    for k in (1, 2, 3):
        g = p.cull_and_pack(cam)
        assert g["total"] == len(bodies)                              # the camera sees all of them
        t = p.tick(K.WORLD96_DT)
        flags = [b.tick(dt) for b in bodies]
        assert t["n_changed"] == sum(any(f) for f in flags) == expect_changed[k - 1], t
        assert t["n_rebucket"] == 0 and t["n_out_of_bounds"] == 0, t
        for b, (moved, rotated) in zip(bodies, flags):
            d = device_state(R, p, b)
            K.check_body(d, b, k, measured, "device")
            assert bool(d["flags"] & K.F_HAS_MOVED) == moved and bool(d["flags"] & K.F_HAS_ROTATED) == rotated, b.id
        print(f"after {k} ticks: ", end=""); show(measured)
    after = p.sections()
    np.testing.assert_array_equal(after["keys"], sections["keys"]); np.testing.assert_array_equal(after["n_local"], sections["n_local"])
    assert_clean_publication(p)


def test_device_three_ticks_against_the_rule(R):
    ents = K.world96()
    p = R.Pipeline(16384, 64)
    assert p.register_model_instances(ents) == 0
    bodies = [K.Body(r) for r in ents]
    for b in bodies:
        K.check_body(device_state(R, p, b), b, 0, {}, "device")
    run_three_ticks(R, p, bodies, K.WORLD96_CHANGED)
    p.close()


def test_device_entities_that_become_dynamic_later(R):
    """the rows k_tick reaches through its list of late movers: an entity added with a Velocity after the upload and the first frame, and one that
    was uploaded without a Velocity and is given one by a change request.  They move by the same rule."""
    C = R._capi
    ents = K.world96()
    late = K.blank_entities(2); late["id"] = (500, 501)
    late["original"][:] = (-1.5, 1, -0.5, 0.75, -1, 2)
    late["pos"] = ((121 * 64 + 30.5, 133 * 64 + 28.25, 127 * 64 + 35.0), (134 * 64 + 33.0, 122 * 64 + 30.5, 131 * 64 + 29.75))
    late["vel"] = ((11.5, -7.25, 3.0), (-9.0, 4.5, 13.75))
    added = late[:1].copy(); added["flags"] = K.F_HAS_VEL
    plain = late[1:].copy(); plain["flags"] = 0
    p = R.Pipeline(16384, 64)
    assert p.register_model_instances(np.concatenate([ents, plain])) == 0
    cam = R.Camera(K.WORLD96_CAMERA["position"], K.WORLD96_CAMERA["direction"], K.WORLD96_CAMERA["far"])
    assert p.cull_and_pack(cam)["total"] == len(ents) + 1
    assert p.register_model_instances(added) == 0
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (C.CHANGE_MODIFY, 501, C.C_VELOCITY, 0, tuple(late["vel"][1]) + (0,))
    p.apply_changes(ch)
    given = plain.copy(); given["flags"] = K.F_HAS_VEL
    bodies = [K.Body(r) for r in np.concatenate([ents, added, given])]
    run_three_ticks(R, p, bodies, tuple(n + 2 for n in K.WORLD96_CHANGED))
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. / 6. the exact-edge table, by the tick and by change requests
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_edge_device(R, p, w, outline, atomic, axis, rows, end, t, start_keys):
    """the device against the written answers (edge_answers), then against the oracle bit for bit"""
    C = R._capi
    answers, oob_ids = edge_answers(outline, atomic, axis, rows, end)
    assert t == K.EDGE_TOTALS, t
    assert sorted(int(i) for i in p.out_of_bounds()) == oob_ids
    unique, shared = {}, []
    for i, (alive, keys, box) in enumerate(answers):
        fl = int(p.read_component(i + 1, C.C_FLAGS)[0])
        assert bool(fl & DEAD) == (not alive), rows[i]
        if not alive:
            continue
        np.testing.assert_array_equal(p.read_component(i + 1, C.C_STATIC_AABB), box, err_msg=rows[i][0])       # unclipped where it sticks out of the world
        np.testing.assert_array_equal(p.read_component(i + 1, C.C_POSITION), end[i], err_msg=rows[i][0])
        if len(keys) == 1:
            unique[keys[0]] = unique.get(keys[0], 0) + 1
        else:
            shared.append((keys, i + 1))
    s = p.sections()
    n_local = {int(k): int(n) for k, n in zip(s["keys"], s["n_local"])}
    for key, n in unique.items():
        assert n_local.get(key) == n, (ro.unpack_key(key), n_local.get(key))
    for (alive, keys, box), start in zip(answers, start_keys):
        if alive and keys != [start]:
            assert n_local.get(start, 0) == 0, ro.unpack_key(start)           # the section it left holds nobody
    got = sorted((sorted(g["keys"]), [int(i) for i in g["active"]], len(g["static"])) for g in p.shared_sections())
    assert got == sorted((keys, [eid], 0) for keys, eid in shared), got
    check_sections(p, w)
    cam = K.edge_camera(outline, atomic)
    g, o = check_frame(R, p, w, R.Camera(cam["position"], cam["direction"], cam["far"]), False)
    assert g["total"] >= 7                                                     # the cases in the middle of the world are in the picture


def edge_pair(R, outline, atomic, axis, moving):
    e, end, rows = K.edge_world(outline, atomic, axis, moving=moving)
    p, w = build_pair(R, e, outline, atomic)
    check_sections(p, w)
    start_keys = []
    for i in range(len(e)):
        kind, keys = w.lookup(i + 1)
        assert kind == 1
        start_keys.append(keys[0])
    return e, end, rows, p, w, start_keys


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("outline,atomic", WORLDS)
def test_device_edges_by_tick(R, outline, atomic, axis):
    e, end, rows, p, w, start_keys = edge_pair(R, outline, atomic, axis, True)
    cam = K.edge_camera(outline, atomic)
    cam = R.Camera(cam["position"], cam["direction"], cam["far"])
    check_frame(R, p, w, cam, False)
    n, oob = w.tick(oracle_camera(cam), K.EDGE_DT)
    t = p.tick(K.EDGE_DT)
    assert n == t["n_changed"] and len(oob) == t["n_out_of_bounds"]
    check_edge_device(R, p, w, outline, atomic, axis, rows, end, t, start_keys)
    p.close(); w.close()


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("outline,atomic", WORLDS)
def test_device_edges_by_change_request(R, outline, atomic, axis):
    """the same end positions through apply_changes (k_apply_rows): the full decision.  Same answers: the two paths agree."""
    C = R._capi
    e, end, rows, p, w, start_keys = edge_pair(R, outline, atomic, axis, False)
    cam = K.edge_camera(outline, atomic)
    check_frame(R, p, w, R.Camera(cam["position"], cam["direction"], cam["far"]), False)      # change requests are applied inside a frame, after its render
    ch = np.zeros(len(e), R.CHANGE_DT)
    for i in range(len(e)):
        ch[i] = (C.CHANGE_MODIFY, i + 1, C.C_POSITION, 0, tuple(end[i]) + (0,))
    n, oob = w.apply_changes(ch.view(ro.CHANGE_DT))
    t = p.apply_changes(ch)
    assert n == t["n_changed"] and len(oob) == t["n_out_of_bounds"]
    check_edge_device(R, p, w, outline, atomic, axis, rows, end, t, start_keys)
    p.close(); w.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. a world whose atomic length is not a power of two, end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_device_world_of_atomic_length_96(R):
    """(12288, 96): the divisions by a section length take their general branch (div_len, udiv_len) and the tick never its short cut"""
    ents = R.synthetic.mixed_world(1500, seed=61, centre=(6144.0, 6144.0, 6144.0), spread=700.0, atomic=96)
    p, w = build_pair(R, ents, 12288, 96)
    check_sections(p, w)
    assert p.stats()["n_shared_sections"] > 5
    cam = R.Camera((6144, 6144, 6500), (0, 0, -1), 1200.0)
    total_changed = 0
    for f, dups in enumerate((False, True, False)):
        g, o = check_frame(R, p, w, cam, dups)
        assert g["total"] > 100
        if f < 2:
            n, oob = w.tick(oracle_camera(cam), 0.05)
            t = p.tick(0.05)
            assert t["n_changed"] == n and t["n_out_of_bounds"] == len(oob), (t, n, len(oob))
            total_changed += n
            check_sections(p, w)
    assert total_changed > 100
    check_entities(R, p, w, ents)
    p.close(); w.close()
