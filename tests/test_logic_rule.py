"""The restatement of LogicFlow::update_logic the GPU tests of re_logic_list compare against (tests/logic_rule.py), checked against the oracle's own
tick: update_positions walks the same entities as update_logic (flows/logic_flow.rs:308-358 and :662-734 share active_world_sections, the shared-section
test and always_execute_entities), so an entity with Velocity and a nonzero velocity before the tick carries HasMoved after it exactly when the rule
lists it."""
import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from logic_rule import logic_call_counts, logic_records, BRANCHES

WORLDS = [(2500, 5, 160.0, 64), (4000, 9, 260.0, 64), (1500, 13, 150.0, 16), (300, 3, 120.0, 64)]      # n, seed, spread, atomic


def camera_draw(R, rng, spread):
    """the camera of one frame, drawn the way test_collision_broad_phase_parity draws it"""
    pos = (8192 + rng.uniform(-spread, spread) * 0.6, 8192 + rng.uniform(-spread, spread) * 0.6, 8192 + rng.uniform(-0.3, 1.2) * spread)
    d = rng.uniform(-1, 1, 3); d[2] -= 1.2
    return R.Camera(pos, tuple(d / np.linalg.norm(d)), float(rng.choice([400.0, 1500.0])))


@pytest.mark.parametrize("n,seed,spread,atomic", WORLDS)
def test_rule_lists_the_entities_the_tick_moves(n, seed, spread, atomic):
    import render_engine_amd as R
    ents = R.synthetic.mixed_world(n, seed=seed, spread=spread, atomic=atomic)
    w = ro.World(16384, atomic)
    w.register(to_oracle(ents))
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(seed)
    taken, checked = {}, 0
    for f in range(4):
        oc = oracle_camera(camera_draw(R, rng, spread))
        st = {}
        calls = logic_call_counts(w, oc, ids, st)
        for b in BRANCHES:
            taken[b] = taken.get(b, 0) + st.get(b, 0)
        if (n, seed, f) == (2500, 5, 0):                              # the counts of this frame are written down in DESIGN.md section 4.3
            assert [st.get(b, 0) for b in BRANCHES] == [433, 37, 326, 163, 23, 19], st
        pre = {e: w.entity(e) for e in ids}
        w.tick(oc, 0.05)
        for e in ids:
            o = pre[e]
            if o is None or not (o["flags"] & ro.F_HAS_VEL) or not np.any(o["vel"] != 0):
                continue
            after = w.entity(e)
            moved = after is not None and bool(after["flags"] & ro.F_HAS_MOVED)
            if after is None:                                         # left the world in this tick: it was processed
                moved = True
            assert moved == (e in calls), (f, e, moved, calls.get(e))
            checked += 1
    assert checked > 50
    need = BRANCHES if atomic == 64 else [b for b in BRANCHES if b != "twice"]           # every branch of the rule is taken
    assert all(taken[b] > 0 for b in need), taken
    w.close()


def test_sample_scene_known_answer():
    """the 45-entity sample scene at the sample camera: every entity is processed once, the user entity through a shared section in view; with the
    sample's table (the user type and MineProducer carry entity_logic: threads/render_thread.rs:108, space_logic/mine_producer.rs:23) the list is two calls"""
    import render_engine_amd as R
    from test_sample_scene import scene
    ents, world, camd = scene()
    w = ro.World(world["outline_length"], world["atomic_length"])
    assert w.register(to_oracle(ents)) == 0
    oc = ro.make_camera(camd["position"], camd["direction"], camd["far"])
    calls = logic_call_counts(w, oc, [int(i) for i in ents["id"]])
    assert dict(calls) == {i: 1 for i in range(45)}
    assert w.lookup(0)[0] != 1 and len(w.lookup(0)[1]) > 1           # the user entity sits in a shared section
    USER, ASTEROID, MINE = 0x1001, 0x1002, 0x1003
    types = {i: ASTEROID for i in range(1, 44)}; types[0] = USER; types[44] = MINE
    table = [(USER, R._capi.LOGIC_ENTITY), (MINE, R._capi.LOGIC_ENTITY)]
    assert logic_records(calls, types, table) == [(0, 0, 1, 1), (44, 1, 1, 1)]
    w.close()
