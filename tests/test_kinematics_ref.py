"""The CPU oracle's tick, registration transform and sin/cos against the float64 rule of kinematics_ref.py (written from the reference's source,
not from the oracle), and the oracle's section decision on boxes whose edges lie exactly on section walls and on the world's faces, against
answers written out here.  The same inputs and bounds run on the device in test_tick_exact_gpu.py."""
import numpy as np
import pytest

import oracle as ro
import kinematics_ref as K
from helpers import to_oracle

F32 = np.float32


def oracle_camera(position, direction, far):
    return ro.make_camera(position, direction, far)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the rule against the oracle: 96 entities, three ticks
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_world96_keeps_clear_of_section_walls():
    """in float64: every box edge after every tick is at least 0.05 away from a multiple of 64, so no rounding can move a box across a wall and
    the known answer of the section decision is that nothing changes section"""
    bodies = [K.Body(r) for r in K.world96()]
    dt = float(F32(K.WORLD96_DT))
    for k in range(4):
        for b in bodies:
            d = np.abs(b.box / 64.0 - np.round(b.box / 64.0)) * 64.0
            assert d.min() >= 0.05, (b.id, k, b.box)
            assert np.all(np.floor(b.box[0::2] / 64.0) == np.floor(b.box[1::2] / 64.0))          # and every box lies inside one level-0 section
        changed = sum(any(b.tick(dt)) for b in bodies)
        assert changed == K.WORLD96_CHANGED[min(k, 2)]


def test_oracle_three_ticks_against_the_rule():
    ents = K.world96()
    bodies = [K.Body(r) for r in ents]
    w = ro.World(16384, 64)
    assert w.register(to_oracle(ents)) == 0
    cam = oracle_camera(**K.WORLD96_CAMERA)
    measured = {}
    state = lambda b: w.entity(b.id)
    for b in bodies:
        K.check_body(state(b), b, 0, measured, "oracle")
    sections = {b.id: w.lookup(b.id) for b in bodies}
    assert all(kind == 1 and len(keys) == 1 for kind, keys in sections.values())
    dt = float(F32(K.WORLD96_DT))
    for k in (1, 2, 3):
        assert len(w.cull(cam)) > 0
        assert w.render(cam)["total"] == len(ents)                    # the camera sees all of them
        n, oob = w.tick(cam, K.WORLD96_DT)
        flags = [b.tick(dt) for b in bodies]
        assert n == sum(any(f) for f in flags) == K.WORLD96_CHANGED[k - 1] and len(oob) == 0
        for b, (moved, rotated) in zip(bodies, flags):
            o = state(b)
            K.check_body(o, b, k, measured, "oracle")
            assert bool(o["flags"] & K.F_HAS_MOVED) == moved and bool(o["flags"] & K.F_HAS_ROTATED) == rotated, b.id
            assert w.lookup(b.id) == sections[b.id], b.id             # n_rebucket == 0: every entity keeps its section
        print(f"after {k} ticks: " + ", ".join(f"{key} {v:.3g}" for key, v in sorted(measured.items())))
    w.close()


def test_oracle_registration_against_the_rule():
    """256 random TRS cases with every combination of the components present"""
    ents = K.random_bodies(256, seed=17)
    w = ro.World(16384, 64)
    assert w.register(to_oracle(ents)) == 0
    measured = {}
    for r in ents:
        K.check_body(w.entity(int(r["id"])), K.Body(r), 0, measured, "oracle")
    print(", ".join(f"{key} {v:.3g}" for key, v in sorted(measured.items())))
    w.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. sin/cos
# ---------------------------------------------------------------------------------------------------------------------------------------
def oracle_sincos(x):
    import ctypes as C
    L = ro.lib()
    s, c = C.c_float(), C.c_float()
    out = np.zeros((len(x), 2), F32)
    for i, v in enumerate(x):
        L.ro_sincosf(C.c_float(float(v)), C.byref(s), C.byref(c))
        out[i] = (s.value, c.value)
    return out[:, 0], out[:, 1]


def test_oracle_sincos_domains():
    """below 1e6: one f32 ulp of the rounded float64 value [measured 0.50 ulp of the exact one].  1e6..2^26: 2^-25 + |x| * 3.9e-17 absolute, half an
    ulp of 1 plus the rounding error of the double 2 pi that the fmod adds, 2.449e-16 per turn [measured 3.12e-8 where the bound is 3.24e-8, at most
    0.999 of the bound anywhere].  Beyond 2^26 an f32 angle is spaced more than a turn apart and carries no phase: finite values in [-1, 1], nothing more."""
    small, high, beyond = K.sincos_arguments()
    assert len(small) > 60000 and len(high) > 19000 and len(beyond) == 200
    measured = {}
    for x in (small, high, beyond):
        s, c = oracle_sincos(x)
        K.check_sincos(x, s, c, measured)
    s, c = oracle_sincos(np.array([0.0, -0.0], F32))
    assert list(s) == [0.0, 0.0] and list(c) == [1.0, 1.0]
    print(", ".join(f"{key} {v:.3g}" for key, v in sorted(measured.items())))


def test_z_rotation_exposes_sincos():
    """a Rotation about +z without Scale: m[0] = cos, m[1] = sin, m[4] = -sin, m[5] = cos of the angle, exactly (also with the axis given as
    (0, 0, 3)): how the device's sin/cos is read in test_tick_exact_gpu.py"""
    small, high, beyond = K.sincos_arguments(n_uniform=600, kmax=100, n_mid=600, n_high=300)
    for axis in ((0, 0, 1), (0, 0, 3)):
        for x in np.concatenate([small[::2], high, beyond]):
            m = ro.trs_matrix((100.5, 200.25, 300.75), axis, x)
            s, c = ro.sincos(x)
            if x == 0:
                s, c = F32(0), F32(1)
            assert m[0] == c and m[1] == s and m[4] == -s and m[5] == c, (axis, x)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. exact edges
# ---------------------------------------------------------------------------------------------------------------------------------------
# the moving coordinate of every case, written out: (start, end, OutOfBoundsLogic, cells it lies in after the tick; () = removed, out of bounds)
EDGES_16384_64 = {
    "A": (8224, 8247, 0, (128,)), "A1": (8224, 8255, 0, (128,)), "B": (8224, 8257, 0, (129,)), "C": (8224, 8256, 0, (128, 129)),
    "D": (8224, 8255.5, 0, (128, 129)), "G": (8224, 8225, 0, (128,)), "H": (8224, 8352, 0, (130,)),
    "E0": (16352, 16383, 0, (255,)), "E1": (16352, 16384, 0, ()), "E2": (16352, 16384, 1, (255,)),
    "F0": (32, 1, 0, (0,)), "F1": (32, 0, 0, ()), "F2": (32, 0, 1, (0,)),
}
EDGES_12288_96 = {
    "A": (6192, 6231, 0, (64,)), "A1": (6192, 6239, 0, (64,)), "B": (6192, 6241, 0, (65,)), "C": (6192, 6240, 0, (64, 65)),
    "D": (6192, 6239.5, 0, (64, 65)), "G": (6192, 6193, 0, (64,)), "H": (6192, 6384, 0, (66,)),
    "E0": (12240, 12287, 0, (127,)), "E1": (12240, 12288, 0, ()), "E2": (12240, 12288, 1, (127,)),
    "F0": (48, 1, 0, (0,)), "F1": (48, 0, 0, ()), "F2": (48, 0, 1, (0,)),
}
EDGES_16384_16 = {
    "A": (8200, 8199, 0, (512,)), "A1": (8200, 8207, 0, (512,)), "B": (8200, 8209, 0, (513,)), "C": (8200, 8208, 0, (512, 513)),
    "D": (8200, 8207.5, 0, (512, 513)), "G": (8200, 8201, 0, (512,)), "H": (8200, 8232, 0, (514,)),
    "E0": (16376, 16383, 0, (1023,)), "E1": (16376, 16384, 0, ()), "E2": (16376, 16384, 1, (1023,)),
    "F0": (8, 1, 0, (0,)), "F1": (8, 0, 0, ()), "F2": (8, 0, 1, (0,)),
}
WRITTEN = {(16384, 64): EDGES_16384_64, (12288, 96): EDGES_12288_96, (16384, 16): EDGES_16384_16}
WORLDS = [(16384, 64), (12288, 96), (16384, 16)]


@pytest.mark.parametrize("outline,atomic", WORLDS)
def test_edge_table_is_the_written_one(outline, atomic):
    """the table that generates the worlds (kinematics_ref.edge_cases) is, number for number, the one written out above -- and the rule's own section
    decision gives the written cells"""
    for axis in (0, 2):
        e, end, rows = K.edge_world(outline, atomic, axis)
        written = WRITTEN[(outline, atomic)]
        assert [r[0].split()[0] for r in rows] == list(written)
        for i, (row, (start, stop, logic, cells)) in enumerate(zip(rows, written.values())):
            assert e["pos"][i][axis] == start and end[i][axis] == stop and bool(row[5] & K.F_OOB_LOGIC) == bool(logic), row
            assert tuple(row[6][1:]) == cells and (row[6][0] == "removed") == (cells == ()), row
            box = np.repeat(end[i].astype(np.float64), 2) + (-1, 1, -1, 1, -1, 1)
            oob, keys = K.section_decision(box, outline, atomic)
            assert oob == (start in (outline - atomic // 2, atomic // 2) and stop in (outline, 0)), row
            if cells:
                assert [K.pack_key(*k) for k in keys] == K.edge_expected_keys(outline, atomic, axis, i, row[6]), row


def edge_answers(outline, atomic, axis, rows, end):
    """per case: (alive, sorted section keys, stored box) and the ids reported out of bounds"""
    out, oob_ids = [], []
    for i, row in enumerate(rows):
        alive = row[6][0] != "removed"
        if not alive:
            oob_ids.append(i + 1)
        box = (np.repeat(end[i].astype(np.float64), 2) + (-1, 1, -1, 1, -1, 1)).astype(F32)       # unclipped, also where it leaves the world
        out.append((alive, K.edge_expected_keys(outline, atomic, axis, i, row[6]), box))
    return out, oob_ids


def check_edge_oracle(w, outline, atomic, axis, rows, end, n, oob, before):
    answers, oob_ids = edge_answers(outline, atomic, axis, rows, end)
    assert n == K.EDGE_TOTALS["n_changed"] and sorted(int(i) for i in oob) == oob_ids and len(oob_ids) == K.EDGE_TOTALS["n_out_of_bounds"]
    changed_section = 0
    for i, (alive, keys, box) in enumerate(answers):
        o = w.entity(i + 1)
        assert (o is not None) == alive, rows[i]
        if not alive:
            continue
        kind, got = w.lookup(i + 1)
        assert sorted(got) == keys and kind == (1 if len(keys) == 1 else 2), (rows[i], kind, [ro.unpack_key(k) for k in got])
        np.testing.assert_array_equal(o["aabb"], box, err_msg=rows[i][0])
        np.testing.assert_array_equal(o["pos"], end[i], err_msg=rows[i][0])
        changed_section += sorted(got) != sorted(before[i + 1][1])
    assert changed_section == K.EDGE_TOTALS["n_rebucket"]


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("outline,atomic", WORLDS)
def test_oracle_edges_by_tick(outline, atomic, axis):
    e, end, rows = K.edge_world(outline, atomic, axis)
    w = ro.World(outline, atomic)
    assert w.register(to_oracle(e)) == 0
    before = {int(i): w.lookup(int(i)) for i in e["id"]}
    cam = oracle_camera(**K.edge_camera(outline, atomic))
    w.cull(cam); w.render(cam)
    n, oob = w.tick(cam, K.EDGE_DT)
    check_edge_oracle(w, outline, atomic, axis, rows, end, n, oob, before)
    w.close()


@pytest.mark.parametrize("axis", [0, 2])
@pytest.mark.parametrize("outline,atomic", WORLDS)
def test_oracle_edges_by_change_request(outline, atomic, axis):
    """the same end positions as Position change requests: the full section decision, no stays-in-its-section short cut"""
    e, end, rows = K.edge_world(outline, atomic, axis, moving=False)
    w = ro.World(outline, atomic)
    assert w.register(to_oracle(e)) == 0
    before = {int(i): w.lookup(int(i)) for i in e["id"]}
    ch = np.zeros(len(e), ro.CHANGE_DT)
    for i in range(len(e)):
        ch[i] = (ro.CHANGE_MODIFY, i + 1, 0, 0, tuple(end[i]) + (0,))
    n, oob = w.apply_changes(ch)
    check_edge_oracle(w, outline, atomic, axis, rows, end, n, oob, before)
    w.close()
