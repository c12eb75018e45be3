"""re_query_boxes on the GPU: the entities in a batch of boxes (what the logic callbacks get instead of &BoundingBoxTree) through the C ABI against
its CPU restatement over the oracle (tests/box_query_rule.py, itself checked against the oracle's section decisions in tests/test_box_query_rule.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from box_query_rule import box_hits, probe_world, probe_push_out, probe_queries, query_world, draw_boxes, overflow_world, overflow_queries
from test_gpu_parity import build_pair, check_frame, random_changes, assert_clean_publication
from test_logic_rule import camera_draw

pytestmark = pytest.mark.gpu

RE_E_ARG, RE_E_STATE = -1, -5


@pytest.fixture(scope="module")
def R():
    import render_engine_amd as R
    return R


def pairs_of(hits):
    return sorted((int(h["query"]), int(h["entity_id"])) for h in hits)


def ask(p, boxes, **k):
    """(sorted pairs, total) of one call; the pairs are distinct and as many as the total"""
    hits, n_total = p.find_entities_in_boxes(boxes, **k)
    got = pairs_of(hits)
    assert len(got) == n_total == len(set(got)), (len(got), n_total, len(set(got)))
    return got, n_total


def expect_error(R, code, text, fn, *a, **k):
    with pytest.raises(R.RenderEngineError) as e:
        fn(*a, **k)
    assert f"({code})" in str(e.value) and text in str(e.value), str(e.value)


@pytest.mark.parametrize("n,seed,spread,atomic", [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)])
def test_box_query_parity(R, n, seed, spread, atomic):
    """ten frames of cull, query, tick over a mixed world (unique sections of several levels, shared sections, entities whose maximum lies on a section
    border) with a change batch every third frame -- moves across section borders, deletes, make-static, wake-up, RemoveComponent, add-entity --:
    64 boxes a frame, the sorted pairs and the total equal the rule's; frames 4 and 7 with the filter, frame 5 behind an asynchronous cull and tick"""
    L = R._capi
    ents = query_world(n, seed, spread, atomic)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(seed)
    total = filtered = 0
    next_id = max(ids) + 1000
    for f in range(10):
        cam = camera_draw(R, rng, spread)
        oc = oracle_camera(cam)
        if f == 5:                                                     # nothing awaited: the query finishes the frame itself (resolve)
            assert p.cull_and_pack(cam, asynchronous=True, copy=False) is None
            p.tick(0.05, asynchronous=True)
            w.cull(oc); w.render(oc); w.tick(oc, 0.05)
        else:
            check_frame(R, p, w, cam, bool(f % 2))
        boxes = draw_boxes(w, ids, rng, 16384)
        flt = dict(need_flags=L.F_CAN_COLLIDE, forbid_flags=L.F_STATIC) if f in (4, 7) else {}
        want = box_hits(w, ids, boxes, need=flt.get("need_flags", 0), forbid=flt.get("forbid_flags", 0))
        got, n_total = ask(p, boxes, **flt)
        if got != want:                                                # name the entities the two sides disagree on, with both flag words
            odd = sorted({e for _, e in set(got) ^ set(want)})[:8]
            raise AssertionError((f, n_total, len(want), [(e, hex(int(p.read_component(e, L.C_FLAGS)[0])), w.lookup(e)[0], hex(w.entity(e)["flags"]) if w.entity(e) else None) for e in odd]))
        assert n_total == len(want), (f, n_total, len(want))
        total += n_total; filtered += n_total if flt else 0
        assert_clean_publication(p)
        if f != 5:
            n_o, oob_o = w.tick(oc, 0.05); t = p.tick(0.05)
            assert t["n_changed"] == n_o and t["n_out_of_bounds"] == len(oob_o)
        if f % 3 == 2:
            ch = random_changes(R, ents, rng, 40, set())
            add = ents[rng.integers(0, len(ents), 3)].copy()           # add-entity: three copies of existing entities under new ids, a little to the side
            add["id"] = next_id + np.arange(3); add["pos"] += np.float32(7.5)
            more = np.zeros(3, R.CHANGE_DT)
            for k in range(3):
                more[k] = (L.CHANGE_ADD_ENTITY, next_id + k, 0, k, (0, 0, 0, 0))
            ch = np.concatenate([ch, more])
            w.apply_changes(ch.view(ro.CHANGE_DT), added=to_oracle(add)); p.apply_changes(ch, added=add)
            ids += [next_id + k for k in range(3)]; next_id += 3
    assert total > 2000 and filtered > 100
    p.close(); w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_known_answers_on_the_device(R, atomic):
    """the hand-worked world on both key encodings (256 sections per axis: compact 32-bit stream keys; 1024: the full keys).  Coordinates in units of atomic / 64."""
    L = R._capi
    s = np.float32(atomic) / np.float32(64.0)
    ents = probe_world(atomic)
    extra = np.zeros(3, R.ENTITY_DT)
    extra[:] = ents[0]
    extra["id"] = (6, 7, 8); extra["flags"] = (0, R.F_STATIC, 0)
    extra["original"][0] = np.array([639, 641] * 3, np.float32) * s       # 6: straddles a section corner: a shared section linked from 8 sections
    extra["original"][1] = np.array([300, 310] * 3, np.float32) * s       # 7: static, in the frozen render cache once a frame has been drawn
    extra["original"][2] = np.array([400, 410] * 3, np.float32) * s       # 8: deleted and created again below
    ents = np.concatenate([ents, extra])
    p, w = build_pair(R, ents, atomic=atomic)
    ids = list(range(9))
    # change requests belong to a frame: one is drawn first (and the static render cache freezes with entity 7 in it)
    check_frame(R, p, w, R.Camera((305.0 * s, 305.0 * s, 900.0 * s), (0, 0, -1), 3000.0), False)
    ch = probe_push_out()
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)

    def cube(lo, hi):
        return [np.float32(lo) * s, np.float32(hi) * s] * 3

    # the boundary pairs, the one-float-above miss, the out-of-bounds entity one cell past the grid
    q, want = probe_queries(atomic)
    assert ask(p, q)[0] == want == box_hits(w, ids, q)
    # the shared section of 8 links: all inside the box -> once; a box over one of its sections only finds it when the boxes intersect
    assert len(w.lookup(6)[1]) == 8
    q = np.array([cube(600, 700), cube(630, 639.5), cube(630, 638), cube(641, 650), cube(641.5, 650)], np.float32)
    assert ask(p, q)[0] == [(0, 6), (1, 6), (3, 6)] == box_hits(w, ids, q)
    # the static entity of the frozen render cache is moved: reported at its live AABB, once; the ghost it leaves in the cache is no entity
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_MODIFY, 7, L.C_POSITION, 0, (500.0 * s, 0.0, 0.0, 0.0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    q = np.array([cube(290, 320), [790 * s, 820 * s, 290 * s, 320 * s, 290 * s, 320 * s]], np.float32)
    assert ask(p, q)[0] == [(1, 7)] == box_hits(w, ids, q)
    assert ask(p, q, need_flags=L.F_STATIC)[0] == [] == box_hits(w, ids, q, need=L.F_STATIC)      # (a moved entity is re-added as not static: the flag follows the tree)
    check_frame(R, p, w, R.Camera((305.0 * s, 305.0 * s, 900.0 * s), (0, 0, -1), 3000.0), False)      # the ghost is drawn ...
    assert ask(p, q)[0] == [(1, 7)]                                                                # ... and still not reported
    # a deleted entity is no longer reported; its id, created again, is reported at the new place
    q = np.array([cube(390, 420), [390 * s, 420 * s, 1390 * s, 1420 * s, 390 * s, 420 * s]], np.float32)
    assert ask(p, q)[0] == [(0, 8)]
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_DELETE, 8, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    assert ask(p, q)[0] == [] == box_hits(w, ids, q)
    add = ents[ents["id"] == 8].copy(); add["pos"][0] = (0.0, 1000.0 * s, 0.0)
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_ADD_ENTITY, 8, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT), added=to_oracle(add)); p.apply_changes(ch, added=add)
    assert ask(p, q)[0] == [(1, 8)] == box_hits(w, ids, q)
    # one box over all of them: everything the tree holds there, once
    q = np.array([[0, 1500 * s] * 3], np.float32)
    assert ask(p, q)[0] == box_hits(w, ids, q) == [(0, e) for e in (0, 1, 2, 4, 5, 6, 7, 8)]
    assert_clean_publication(p)
    p.close(); w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_staging_overflow(R, atomic):
    """more records in one workgroup than it stages (BOXQ_HITBUF = 1024; tests/test_box_query_rule.py holds the precondition): box 0 makes one wave walk
    1101 hit rows of one unique section (the overflow of the row walk), box 1 makes one lane emit the 1100 members of one shared section (the overflow of
    the shared part)"""
    ents = overflow_world(atomic)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = [int(i) for i in ents["id"]]
    boxes, _, _ = overflow_queries(atomic)
    want = box_hits(w, ids, boxes)
    assert len(want) == 2201
    for _ in range(2):                                                 # the same call again: the header was left zero
        got, n_total = ask(p, boxes)
        assert got == want and n_total == len(want)
    hits, n_total = p.find_entities_in_boxes(boxes, capacity=0)
    assert n_total == len(want) and len(hits) == 0
    hits, n_total = p.find_entities_in_boxes(boxes, capacity=1050)     # above the stage, below the total
    assert n_total == len(want) and len(hits) == 1050 and len(set(pairs_of(hits))) == 1050 and set(pairs_of(hits)) <= set(want)
    assert ask(p, boxes) == (want, len(want))
    assert_clean_publication(p)
    p.close(); w.close()


def test_boundaries_of_the_call(R):
    L = R._capi
    lib = L.load()
    n = C.c_uint32(77)
    one = np.array([[8100, 8300] * 3], np.float32)
    # before any upload
    p0 = R.Pipeline()
    assert lib.re_query_boxes(p0._h, one.ctypes.data, 1, None, None, 0, C.byref(n)) == RE_E_STATE
    p0.close()
    ents = query_world(600, 3, 120.0, 64)
    p, w = build_pair(R, ents)
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(3)
    boxes = draw_boxes(w, ids, rng, 16384, n=16)
    want = box_hits(w, ids, boxes)
    assert len(want) > 50
    # n == 0
    assert lib.re_query_boxes(p._h, None, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.re_query_boxes(p._h, boxes.ctypes.data, len(boxes), None, None, 0, None) == 0         # n_total is optional
    # capacity 0: the total is exact; capacity 7 of more: 7 distinct correct pairs, the total exact
    hits, n_total = p.find_entities_in_boxes(boxes, capacity=0)
    assert n_total == len(want) and len(hits) == 0
    hits, n_total = p.find_entities_in_boxes(boxes, capacity=7)
    assert n_total == len(want) and len(hits) == 7 and len(set(pairs_of(hits))) == 7 and set(pairs_of(hits)) <= set(want)
    assert ask(p, boxes)[0] == want
    # refused batches name the box and leave the world alone: the next correct call answers
    bad = boxes.copy(); bad[3, 2] = np.nan
    expect_error(R, RE_E_ARG, "box 3", p.find_entities_in_boxes, bad)
    bad = boxes.copy(); bad[5, 4], bad[5, 5] = bad[5, 5], bad[5, 4] - 1
    expect_error(R, RE_E_ARG, "box 5", p.find_entities_in_boxes, bad)
    bad = boxes.copy(); bad[9] = [7000, 10000] * 3
    expect_error(R, RE_E_ARG, "box 9", p.find_entities_in_boxes, bad)
    args = L.BoxQueryArgs(0, 0); args.reserved[1] = 1
    assert lib.re_query_boxes(p._h, boxes.ctypes.data, len(boxes), C.byref(args), None, 0, C.byref(n)) == RE_E_ARG
    assert b"reserved" in lib.re_last_error(p._h)
    assert lib.re_query_boxes(p._h, boxes.ctypes.data, len(boxes), None, None, 4, C.byref(n)) == RE_E_ARG          # capacity without a buffer
    assert lib.re_query_boxes(p._h, boxes.ctypes.data, L.BOX_QUERY_MAX_QUERIES + 1, None, None, 0, C.byref(n)) == RE_E_ARG
    assert ask(p, boxes)[0] == want
    # 4096 identical boxes: every query index appears, with the same set
    same = np.repeat(boxes[:1], 4096, axis=0)
    ent0 = sorted(e for i, e in want if i == 0)
    assert len(ent0) > 0
    hits, n_total = p.find_entities_in_boxes(same)
    assert n_total == 4096 * len(ent0) == len(hits)
    order = np.lexsort((hits["entity_id"], hits["query"]))
    np.testing.assert_array_equal(hits["query"][order], np.repeat(np.arange(4096, dtype=np.uint32), len(ent0)))
    np.testing.assert_array_equal(hits["entity_id"][order], np.tile(np.array(ent0, np.uint32), 4096))
    # a second context in the same process, unaffected and unaffecting
    ents2 = probe_world(64)
    p2, w2 = build_pair(R, ents2)
    q2, _ = probe_queries(64)
    assert ask(p2, q2)[0] == box_hits(w2, range(6), q2) == [(0, 0), (0, 1), (0, 2), (0, 4), (1, 1), (1, 2)]      # (entity 3 has not been pushed out here)
    assert ask(p, boxes)[0] == want
    assert ask(p2, q2)[1] == 6
    assert_clean_publication(p); assert_clean_publication(p2)
    p2.close(); w2.close(); p.close(); w.close()


def test_sample_scene_mine_producer(R):
    """the 45-entity sample scene: who is within a 200-unit box around the mine producer"""
    from test_sample_scene import scene
    ents, world, camd = scene()
    p, w = build_pair(R, ents, outline=world["outline_length"], atomic=world["atomic_length"])
    ids = [int(i) for i in ents["id"]]
    c = w.entity(44)["aabb"].reshape(3, 2).mean(axis=1)
    q = np.array([[c[0] - 100, c[0] + 100, c[1] - 100, c[1] + 100, c[2] - 100, c[2] + 100]], np.float32)
    want = box_hits(w, ids, q)
    assert (0, 44) in want
    assert ask(p, q)[0] == want
    p.cull_and_pack(R.Camera(camd["position"], camd["direction"], camd["far"]))
    assert ask(p, q)[0] == want
    assert_clean_publication(p)
    p.close(); w.close()


def test_cpp_mirror_find_entities_in_boxes():
    """include/render_engine_hip.hpp: Pipeline::find_entities_in_boxes -- before the first frame, filtered, with an instance registered after frames have
    run, a box that touches an instance on a section border (tests/cpp/box_query_shim_test.cpp)"""
    import os
    import subprocess
    from render_engine_amd import build as libbuild
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(here, "cpp", "_build", "box_query_shim_test")
    lib_dir = os.path.dirname(libbuild.build_library())
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(here), "include"),
                           os.path.join(here, "cpp", "box_query_shim_test.cpp"), "-o", exe, "-L", lib_dir, "-lrender_engine_hip", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "OK box queries" in out.stdout, out.stdout + out.stderr
