"""The chunk plan of synchronous frames (k_scan_cull_plan): the scan reads only the 2048-key chunks whose sections can lie in a candidate box --
the (level, x, z) columns of the last full build plus every chunk a section was created into since.  Every frame here is taken twice, through
the plan and through the full key stream (RE_CULL_FORCE_STREAM), and both are compared with the oracle: visible sections with multiplicity,
InstanceRange table, entity ids and matrices bit for bit."""
import os

import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera, assert_render_equal, expand_vis

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import render_engine_amd as R
    return R


def build_pair(R, ents, caps=None, flags=0):
    old = os.environ.get("RE_EXP_PLAN_CAPS")
    if caps:
        os.environ["RE_EXP_PLAN_CAPS"] = caps                  # read when the section table is built
    try:
        p = R.Pipeline(16384, 64, flags=flags)
        assert p.register_model_instances(ents) == 0
    finally:
        if caps:
            if old is None: os.environ.pop("RE_EXP_PLAN_CAPS")
            else: os.environ["RE_EXP_PLAN_CAPS"] = old
    w = ro.World(16384, 64)
    assert w.register(to_oracle(ents)) == 0
    return p, w


def both_ways(R, p, w, cam, dups=False):
    """the frame through the plan (default) and through the full stream: each bit-exact with the oracle.  Returns whether the plan was taken."""
    oc = oracle_camera(cam)
    vis_o = w.cull(oc)
    o = w.render(oc, emit_duplicates=dups)
    n0 = p.plan_stats()["n_plan_frames"]
    for force in (False, True):
        g = p.cull_and_pack(cam, emit_duplicates=dups, force_stream=force)
        keys, mult = p.visible_sections()
        np.testing.assert_array_equal(expand_vis(keys, mult), vis_o, err_msg=f"force_stream={force}")
        assert g["n_visible_vec"] == len(vis_o)
        assert_render_equal(g, o)
        if force: assert p.plan_stats()["n_plan_frames"] == n1, "a frame under RE_CULL_FORCE_STREAM took the plan"
        else: n1 = p.plan_stats()["n_plan_frames"]
    st = p.stats()
    assert st["n_seal_waits"] == 0 and st["n_sync_fallbacks"] == 0, st
    return n1 > n0, o


def test_plan_static_lattice(R):
    """a static lattice: the plan is far smaller than the table; duplicates mode, an empty view, a candidate box that wraps (the full stream)"""
    ents = R.synthetic.lattice_world(cells_per_axis=48, first_cell=104, straddler_fraction=0.02)
    p, w = build_pair(R, ents)
    nchunks = (p.stats()["n_section_slots"] + 2047) // 2048
    cams = [R.Camera((8192 + 37.5 * i, 8192 - 21.25 * i, 8500 - 40 * i), (0.1 * i - 0.3, 0.05 * i, -1), 600.0 + 150.0 * (i % 3)) for i in range(6)]
    planned = 0
    for f, cam in enumerate(cams):
        took, o = both_ways(R, p, w, cam, dups=bool(f % 2))
        planned += took
        if took: assert 0 < p.plan_stats()["last_plan_chunks"] < nchunks
    assert planned == len(cams) and o["total"] > 0
    took, o = both_ways(R, p, w, R.Camera((200.0, 200.0, 200.0), (1, 0, 0), 50.0))             # nothing in view
    assert o["total"] == 0
    took, o = both_ways(R, p, w, R.Camera((65530.0 * 64, 8192.0, 8192.0), (1, 0, 0), 1000.0))  # the level-0 box runs past index 0xFFFF: it wraps around
    assert not took
    p.close(); w.close()


def test_plan_sections_created_by_movers_and_change_requests(R):
    """sections created since the last full build sit in spare or emptied slots outside key order: the device re-bucket creates them
    behind ticks with movers, the host patch behind change-request batches the device path does not take (make-static / wake-up);
    an entity moved by such a batch far along x into a section of its own is then the only thing in view"""
    rng = np.random.default_rng(11)
    ents = R.synthetic.mixed_world(3000, seed=41, spread=500.0)
    ents["vel"] *= 6.0
    p, w = build_pair(R, ents)
    for f in range(10):                                      # movers: the device re-bucket creates and empties sections
        cam = R.Camera((8192 + rng.uniform(-300, 300), 8192 + rng.uniform(-300, 300), 8700), (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -1), rng.uniform(300, 1500))
        both_ways(R, p, w, cam, dups=bool(f % 3 == 0))
        oc = oracle_camera(cam)
        n_o, _ = w.tick(oc, 0.05); t = p.tick(0.05)
        assert t["n_changed"] == n_o
    st = p.stats()
    assert st["n_device_rebuckets"] > 0 and p.plan_stats()["n_open_chunks"] > 0, (st, p.plan_stats())
    C = R._capi
    ids = [int(i) for i in ents["id"][(ents["flags"] & R.F_STATIC) == 0][:4]]
    for k, (x, z) in enumerate([(15000.0, 1500.0), (1200.0, 15200.0)]):          # far from every other section, in x and in z
        hosts0 = p.stats()["n_host_rebuckets"]
        ch = np.zeros(3, R.CHANGE_DT)
        ch[0] = (C.CHANGE_MAKE_STATIC, ids[2 * k + 1], 0, 0, (0, 0, 0, 0))
        ch[1] = (C.CHANGE_WAKE_UP, ids[2 * k + 1], 0, 0, (0, 0, 0, 0))
        ch[2] = (C.CHANGE_MODIFY, ids[2 * k], C.C_POSITION, 0, (x, 8192.0, z, 0))
        n_a, _ = w.apply_changes(ch.view(ro.CHANGE_DT))
        g = p.apply_changes(ch)
        assert g["n_changed"] == n_a
        assert p.stats()["n_host_rebuckets"] > hosts0
        took, o = both_ways(R, p, w, R.Camera((x, 8192.0, z + 120.0), (0, 0, -1), 200.0))
        assert took and o["total"] >= 1 and ids[2 * k] in set(int(i) for i in o["ids"]), o["total"]
    # ... and a tick's movers into new sections, the camera on where they went
    for f in range(4):
        cam = R.Camera((8192 + rng.uniform(-500, 500), 8192 + rng.uniform(-500, 500), 8400), (0, 0, -1), 400.0)
        both_ways(R, p, w, cam)
        n_o, _ = w.tick(oracle_camera(cam), 0.05); p.tick(0.05)
    p.close(); w.close()


@pytest.mark.parametrize("caps", ["4,128", "256,0"])
def test_plan_caps_fall_back_to_the_stream(R, caps):
    """more chunks than the plan may hold ('4,128'), or any open chunk at all ('256,0'): those frames stream every key, with identical results"""
    ents = R.synthetic.mixed_world(3000, seed=43, spread=500.0)
    ents["vel"] *= 6.0
    p, w = build_pair(R, ents, caps=caps)
    rng = np.random.default_rng(3)
    taken = []
    for f in range(8):
        cam = R.Camera((8192 + rng.uniform(-200, 200), 8192 + rng.uniform(-200, 200), 8700), (0, 0, -1), rng.uniform(500, 1500))
        took, _ = both_ways(R, p, w, cam, dups=bool(f % 2))
        taken.append(took)
        n_o, _ = w.tick(oracle_camera(cam), 0.05); p.tick(0.05)
    if caps == "256,0":
        assert taken[0] and p.plan_stats()["n_open_chunks"] > 0 and not taken[-1]
    p.close(); w.close()


def test_plan_soak_with_movers_and_deletions(R):
    """random synchronous frames with movers and deleted entities between them, duplicates mode on and off"""
    rng = np.random.default_rng(17)
    ents = R.synthetic.mixed_world(4000, seed=47, spread=700.0)
    ents["vel"] *= 8.0
    p, w = build_pair(R, ents)
    C = R._capi
    alive = [int(i) for i in ents["id"][(ents["flags"] & R.F_STATIC) == 0]]
    for f in range(24):
        cam = R.Camera(tuple(8192 + rng.uniform(-600, 600, 3)), tuple(rng.uniform(-1, 1, 3) + np.array([0, 0, -0.5])), rng.uniform(200, 2000))
        both_ways(R, p, w, cam, dups=bool(rng.integers(2)))
        if f % 6 == 5:                                        # a delete batch: emptied slots that later creations reuse
            ch = np.zeros(3, R.CHANGE_DT)
            for i in range(3):
                ch[i] = (C.CHANGE_DELETE, alive.pop(int(rng.integers(len(alive)))), 0, 0, (0, 0, 0, 0))
            n_a, _ = w.apply_changes(ch.view(ro.CHANGE_DT)); g = p.apply_changes(ch)
            assert g["n_changed"] == n_a
        n_o, _ = w.tick(oracle_camera(cam), 0.05); t = p.tick(0.05)
        assert t["n_changed"] == n_o
    assert p.plan_stats()["n_plan_frames"] > 0
    p.close(); w.close()
