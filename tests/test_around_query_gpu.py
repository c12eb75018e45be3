"""re_query_boxes_around / re_query_spheres_around on the GPU: "who is within reach of me" for a batch of entity ids, the query records built on the device
from the askers' live StaticAABB / Position.  Against (a) the rule over the oracle (tests/around_rule.py) and (b) the sibling call (re_query_boxes,
re_query_spheres) on geometry built in numpy f32 from read_component values, with the asker removed: the sorted records equal, dist_sq bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from box_query_rule import N_BORDER, probe_world, query_world
from sphere_rule import NO_ENTITY, records_of
from around_rule import F32, OK, NOT_IN_TREE, TOO_LARGE, around_box_hits, around_sphere_hits, draw_asks
from test_around_rule import LONG, around_world, push_partly_out, known_asks
from test_gpu_parity import build_pair, check_frame, random_changes, assert_clean_publication
from test_logic_rule import camera_draw

pytestmark = pytest.mark.gpu

RE_E_ARG, RE_E_STATE = -1, -5


@pytest.fixture(scope="module")
def R():
    import render_engine_amd as R
    return R


def pairs_of(hits):
    return sorted(zip(hits["query"].tolist(), hits["entity_id"].tolist()))


def ask_boxes(p, askers, reach, keep=False, **k):
    """(sorted pairs, status) of one re_query_boxes_around; the pairs are distinct and as many as the total"""
    hits, n_total, status = p.find_entities_around(askers, reach, include_self=keep, **k)
    got = pairs_of(hits)
    assert len(got) == n_total == len(set(got)), (len(got), n_total)
    assert_clean_publication(p)
    return got, list(status)


def ask_spheres(p, askers, reach, keep=False, **k):
    hits, n_total, status = p.find_entities_within_reach(askers, reach, include_self=keep, **k)
    got = records_of(hits)
    assert len(got) == n_total == len({rec[:2] for rec in got}), (len(got), n_total)
    assert_clean_publication(p)
    return got, list(status)


def sibling_boxes(R, p, askers, reach, keep, status, **k):
    """what the caller did before: one read_component per asker, the boxes in numpy f32, re_query_boxes, the asker taken out on the host"""
    L = R._capi
    reach = np.broadcast_to(np.asarray(reach, F32), (len(askers),)); keep = np.broadcast_to(np.asarray(keep, bool), (len(askers),))
    live = [i for i in range(len(askers)) if status[i] == OK]
    boxes = np.zeros((len(live), 6), F32)
    for j, i in enumerate(live):
        ab = p.read_component(int(askers[i]), L.C_STATIC_AABB)
        boxes[j, 0::2] = ab[0::2] - reach[i]; boxes[j, 1::2] = ab[1::2] + reach[i]
    hits, _ = p.find_entities_in_boxes(boxes, **k)
    return sorted((live[q], e) for q, e in pairs_of(hits) if keep[live[q]] or e != int(askers[live[q]]))


def sibling_spheres(R, p, askers, reach, keep, status, **k):
    L = R._capi
    reach = np.broadcast_to(np.asarray(reach, F32), (len(askers),)); keep = np.broadcast_to(np.asarray(keep, bool), (len(askers),))
    live = [i for i in range(len(askers)) if status[i] == OK]
    sph = np.zeros((len(live), 4), F32)
    for j, i in enumerate(live):
        sph[j, 0:3] = p.read_component(int(askers[i]), L.C_POSITION); sph[j, 3] = reach[i]
    ex = np.array([NO_ENTITY if keep[i] else int(askers[i]) for i in live], np.uint32)
    hits, _ = p.find_entities_within_radius(sph, exclude=ex, **k)
    return sorted((live[rec[0]],) + rec[1:] for rec in records_of(hits))


def expect_error(R, code, text, fn, *a, **k):
    with pytest.raises(R.RenderEngineError) as e:
        fn(*a, **k)
    assert f"({code})" in str(e.value) and text in str(e.value), str(e.value)


def describe(got, want):
    return sorted(set(got) - set(want))[:6], sorted(set(want) - set(got))[:6]


@pytest.mark.parametrize("n,seed,spread,atomic", [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)])
def test_around_query_parity(R, n, seed, spread, atomic):
    """ten frames of cull, query, tick over the mixed world of test_sphere_query_parity with a change batch every third frame (add-entity among them):
    64 askers a frame among the live ids, reaches from 0 to three atomic lengths; both calls equal the rule over the oracle and the sibling call on geometry
    read back per asker; frames 4 and 7 with the filter, frame 5 behind an asynchronous cull and tick"""
    L = R._capi
    ents = query_world(n, seed, spread, atomic)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = [int(i) for i in ents["id"]]
    border_ids = sorted(ids)[-N_BORDER:]
    rng = np.random.default_rng(seed)
    pairs = records = filtered = left_out = 0
    next_id = max(ids) + 1000
    for f in range(10):
        cam = camera_draw(R, rng, spread)
        oc = oracle_camera(cam)
        if f == 5:                                                     # nothing awaited: the query finishes the frame itself
            assert p.cull_and_pack(cam, asynchronous=True, copy=False) is None
            p.tick(0.05, asynchronous=True)
            w.cull(oc); w.render(oc); w.tick(oc, 0.05)
        else:
            check_frame(R, p, w, cam, bool(f % 2))
        askers, reach, keep = draw_asks(w, ids, rng, atomic, border_ids=border_ids)
        flt = dict(need_flags=L.F_CAN_COLLIDE, forbid_flags=L.F_STATIC) if f in (4, 7) else {}
        oflt = dict(need=flt.get("need_flags", 0), forbid=flt.get("forbid_flags", 0))
        bwant, bst = around_box_hits(w, ids, askers, reach, keep, atomic=atomic, **oflt)
        bgot, bgot_st = ask_boxes(p, askers, reach, keep, **flt)
        assert bgot_st == list(bst), (f, bgot_st, list(bst))
        assert bgot == bwant, (f, len(bgot), len(bwant), describe(bgot, bwant))
        swant, sst = around_sphere_hits(w, ids, askers, reach, keep, atomic=atomic, **oflt)
        sgot, sgot_st = ask_spheres(p, askers, reach, keep, **flt)
        assert sgot_st == list(sst), (f, sgot_st, list(sst))
        assert sgot == swant, (f, len(sgot), len(swant), describe(sgot, swant))
        assert bgot == sibling_boxes(R, p, askers, reach, keep, bgot_st, **flt), f
        assert sgot == sibling_spheres(R, p, askers, reach, keep, sgot_st, **flt), f
        pairs += len(bgot); records += len(sgot); filtered += len(bgot) if flt else 0
        left_out += len(around_box_hits(w, ids, askers, reach, True, atomic=atomic, **oflt)[0]) - len(around_box_hits(w, ids, askers, reach, False, atomic=atomic, **oflt)[0])
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
    print(dict(pairs=pairs, records=records, filtered=filtered, left_out=left_out))
    # (floors well below what tests/test_around_rule.py finds in three draws over the same worlds)
    assert pairs > 20000 and records > 5000 and filtered > 100 and left_out > 60, (pairs, records, filtered, left_out)
    p.close(); w.close()


def test_a_mover_is_asked_about_where_the_tick_has_carried_it(R):
    """the point of the call: a mover that re_tick carries across the section border x = 64 is asked about right after the tick, with no read-back in between:
    the answer is the one for its new box.  Before: [58, 62] in x, 8 from the neighbour that ends at 50 and 18 from the one that starts at 80; after one tick of
    0.1 at velocity 100: [68, 72], 18 and 8 away.  Reach 10 (boxes) and 14 (spheres, from the Position in the middle)."""
    L = R._capi
    e = np.zeros(3, R.ENTITY_DT)
    e["id"] = (0, 1, 2); e["scale"] = 1.0; e["rot_axis"][:, 1] = 1.0; e["rotvel_axis"][:, 0] = 1.0; e["rotacc_axis"][:, 2] = 1.0
    e["original"][0] = [-2, 2, -2, 2, -2, 2]; e["pos"][0] = (60, 200, 200); e["vel"][0] = (100, 0, 0); e["flags"][0] = L.F_HAS_VEL | L.F_ALWAYS_EXEC
    e["original"][1] = [40, 50, 198, 202, 198, 202]
    e["original"][2] = [80, 90, 198, 202, 198, 202]
    p, w = build_pair(R, e)
    cam = R.Camera((65.0, 200.0, 400.0), (0, 0, -1), 1000.0)
    check_frame(R, p, w, cam, False)
    np.testing.assert_array_equal(w.entity(0)["aabb"], [58, 62, 198, 202, 198, 202])
    assert w.lookup(0) == (1, [ro.pack_key(0, 0, 3, 3)])
    assert ask_boxes(p, [0], 10.0) == ([(0, 1)], [OK]) and around_box_hits(w, range(3), [0], 10.0)[0] == [(0, 1)]
    assert [rec[:2] for rec in ask_spheres(p, [0], 14.0)[0]] == [(0, 1)]
    oc = oracle_camera(cam)
    n_o, _ = w.tick(oc, 0.1)
    t = p.tick(0.1)
    assert t["n_changed"] == n_o == 1 and t["n_rebucket"] == 1                 # carried into another section
    assert w.lookup(0) == (1, [ro.pack_key(0, 1, 3, 3)])
    np.testing.assert_array_equal(w.entity(0)["aabb"], [68, 72, 198, 202, 198, 202])
    # nothing is read back between the tick and the asks
    assert ask_boxes(p, [0], 10.0) == ([(0, 2)], [OK]) and around_box_hits(w, range(3), [0], 10.0)[0] == [(0, 2)]
    got, _ = ask_spheres(p, [0], 14.0)
    assert got == around_sphere_hits(w, range(3), [0], 14.0)[0] and [rec[:2] for rec in got] == [(0, 2)]
    assert got[0][2] == int(F32(100.0).view(np.uint32)) and got[0][3] == 1      # 10 below the minimum x face of 2, from (70, 200, 200)
    np.testing.assert_array_equal(p.read_component(0, L.C_STATIC_AABB), w.entity(0)["aabb"])
    p.close(); w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_known_answers_and_edges_on_the_device(R, atomic):
    """the hand-worked asks of tests/test_around_rule.py on both key encodings; then a query beyond the cap and an asker out of the tree among answered
    neighbours, the same asker twice, 257 asks, a small capacity, and a moved static entity of the frozen cache as asker"""
    L = R._capi
    s = F32(atomic) / F32(64.0)
    p, w = build_pair(R, around_world(atomic), atomic=atomic)
    ids = list(range(10))
    cam = R.Camera((305.0 * s, 305.0 * s, 900.0 * s), (0, 0, -1), 3000.0)
    check_frame(R, p, w, cam, False)                                       # (change requests belong to a frame; the static render cache freezes with 7 in it)
    ch = push_partly_out()
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    askers, reach, keep, bwant, swant = known_asks(atomic)
    assert ask_boxes(p, askers, reach, keep) == (bwant, [OK] * len(askers))
    assert ask_spheres(p, askers, reach, keep) == (swant, [OK] * len(askers))
    assert bwant == around_box_hits(w, ids, askers, reach, keep, atomic=atomic)[0] and swant == around_sphere_hits(w, ids, askers, reach, keep, atomic=atomic)[0]
    # the filter is the sibling's: static entities alone (7), and everything but them
    assert ask_boxes(p, askers, reach, keep, need_flags=L.F_STATIC)[0] == [(q, e) for q, e in bwant if e == 7] == around_box_hits(w, ids, askers, reach, keep, need=ro.F_STATIC, atomic=atomic)[0]
    assert ask_boxes(p, askers, reach, keep, forbid_flags=L.F_STATIC)[0] == [(q, e) for q, e in bwant if e != 7]
    assert ask_spheres(p, askers, reach, keep, forbid_flags=L.F_OOB_LOGIC)[0] == around_sphere_hits(w, ids, askers, reach, keep, forbid=ro.F_OOB_LOGIC, atomic=atomic)[0]
    # 8 with a reach of 40 atomic lengths is beyond the cap: it alone is refused, its neighbours in the batch are answered as before
    a4, r4 = np.array([0, 8, 1, 8], np.uint32), np.array([0, 40 * atomic, 0, 0], F32)
    want4 = [(0, 1), (0, 2), (0, 4), (2, 0), (2, 2), (2, 4)]
    assert ask_boxes(p, a4, r4) == (want4, [OK, TOO_LARGE, OK, OK]) and list(around_box_hits(w, ids, a4, r4, atomic=atomic)[1]) == [OK, TOO_LARGE, OK, OK]
    sgot, sst = ask_spheres(p, a4, r4)
    assert sst == [OK, TOO_LARGE, OK, OK] and [rec[:2] for rec in sgot] == [(0, 4), (2, 4), (3, 4)] and sgot == around_sphere_hits(w, ids, a4, r4, atomic=atomic)[0]
    # the same asker twice, once keeping itself
    assert ask_boxes(p, [0, 0], 0.0, [False, True])[0] == [(0, 1), (0, 2), (0, 4), (1, 0), (1, 1), (1, 2), (1, 4)]
    # 257 asks: one past a tile of the shared part and one past a 256-thread build block; the last is answered like the first of its kind
    many = np.tile(np.array([0, 1, 6, LONG], np.uint32), 65)[:257]
    bgot, bst = ask_boxes(p, many, F32(231.0) * s)
    bwant, bwant_st = around_box_hits(w, ids, many, F32(231.0) * s, atomic=atomic)
    assert bst == list(bwant_st) and bgot == bwant
    assert bst == [OK] * 257 if atomic == 64 else bst[:4] == [OK, OK, OK, TOO_LARGE]       # (626 x 9 x 9 sections of 16 around the long entity)
    assert [e for q, e in bgot if q == 256] == [e for q, e in bgot if q == 0] and len([1 for q, _ in bgot if q == 256]) >= 3
    sgot, sst = ask_spheres(p, many, F32(231.0) * s)
    assert sst == [OK] * 257 and sgot == around_sphere_hits(w, ids, many, F32(231.0) * s, atomic=atomic)[0]
    # capacity below the total: the total counts on, the first records are valid; capacity 0
    hits, n_total, status = p.find_entities_around(many, F32(231.0) * s, capacity=50)
    assert n_total == len(bgot) > 50 and len(hits) == 50 and len(set(pairs_of(hits))) == 50 and set(pairs_of(hits)) <= set(bgot) and list(status) == bst
    hits, n_total, status = p.find_entities_within_reach(many, F32(231.0) * s, capacity=0)
    assert n_total == len(sgot) and len(hits) == 0 and not status.any()
    # the static entity 7 ([300, 310]^3) of the frozen cache is moved by +500 s in x: its live box [800, 810] asks, the ghost never: LONG passes through both places
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_MODIFY, 7, L.C_POSITION, 0, (500.0 * s, 0.0, 0.0, 0.0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    far = np.array([[790 * s, 795 * s, 305 * s, 305 * s, 305 * s, 305 * s]], F32)
    assert pairs_of(p.find_entities_in_boxes(far)[0]) == [(0, LONG)]
    assert ask_boxes(p, [7, 7], [0.0, 0.0], [False, True]) == ([(0, LONG), (1, 7), (1, LONG)], [OK, OK])
    assert ask_boxes(p, [LONG], 0.0) == ([(0, 7)], [OK]) == (around_box_hits(w, ids, [LONG], 0.0, atomic=atomic)[0], [OK])
    check_frame(R, p, w, cam, False)                                       # the ghost is drawn ...
    assert ask_boxes(p, [7, LONG], 0.0)[0] == [(0, LONG), (1, 7)]          # ... and neither asks nor answers
    got, _ = ask_spheres(p, [7], F32(40.0) * s, True)                      # Position (500 s, 0, 0): nobody but, far off, nothing; its own box is 305 s away in y and z
    assert got == around_sphere_hits(w, ids, [7], F32(40.0) * s, True, atomic=atomic)[0]
    p.close(); w.close()


def test_an_asker_out_of_the_tree(R):
    """an entity that has no section: registered outside the world without out-of-bounds logic it is rejected from the tree, its row stays -- and an unknown id"""
    L = R._capi
    ents = probe_world(64)
    ents["original"][5] = [20000, 20010, 10, 20, 10, 20]                  # beyond the outline of 16384
    p = R.Pipeline(16384, 64)
    w = ro.World(16384, 64)
    rej = p.register_model_instances(ents)
    assert rej == w.register(to_oracle(ents)) == 1 and w.lookup(5)[0] == 0
    fl = int(p.read_component(5, L.C_FLAGS)[0])
    if fl & 0x80000000:                                                    # the rejected entity was removed altogether: the id is unknown
        expect_error(R, RE_E_ARG, "ask 1", p.find_entities_around, [0, 5], 0.0)
    else:
        assert ask_boxes(p, [0, 5, 1], 0.0) == ([(0, 1), (0, 2), (0, 4), (2, 0), (2, 2), (2, 4)], [OK, NOT_IN_TREE, OK])
        assert ask_spheres(p, [0, 5, 1], 0.0)[1] == [OK, NOT_IN_TREE, OK]
        assert list(around_box_hits(w, range(6), [0, 5, 1], 0.0)[1]) == [OK, NOT_IN_TREE, OK]
    assert_clean_publication(p)
    p.close(); w.close()


def test_boundaries_of_the_call(R):
    L = R._capi
    lib = L.load()
    n = C.c_uint32(77)
    one = np.zeros(1, L.AROUND_DT); one["entity_id"] = 0; one["reach"] = 5
    st = np.zeros(4, np.uint8)
    for fn in (lib.re_query_boxes_around, lib.re_query_spheres_around):
        pe = R.Pipeline()
        assert fn(pe._h, one.ctypes.data, 1, None, None, 0, C.byref(n), None) == RE_E_STATE           # before any upload
        pe.close()
    p, w = build_pair(R, around_world(64))
    asks = np.zeros(4, L.AROUND_DT); asks["entity_id"] = (0, 1, 4, 8); asks["reach"] = (0, 0, 17.5, 0)
    for fn, name, dt in ((lib.re_query_boxes_around, b"re_query_boxes_around", L.BOX_HIT_DT), (lib.re_query_spheres_around, b"re_query_spheres_around", L.SPHERE_HIT_DT)):
        assert fn(p._h, None, 0, None, None, 0, C.byref(n), None) == 0 and n.value == 0              # n == 0
        assert fn(p._h, asks.ctypes.data, 4, None, None, 0, None, st.ctypes.data) == 0 and not st.any()      # n_total is optional
        assert fn(p._h, asks.ctypes.data, 4, None, None, 0, C.byref(n), None) == 0 and n.value > 0  # status is optional
        total = n.value

        def refused(bad, text, code=RE_E_ARG, n_asks=4, args=None, cap=0):
            assert fn(p._h, None if bad is None else bad.ctypes.data, n_asks, args, None, cap, C.byref(n), None) == code
            err = lib.re_last_error(p._h)
            assert name in err and text in err, err

        bad = asks.copy(); bad["entity_id"][2] = 77
        refused(bad, b"ask 2: unknown entity 77")
        for k, v in enumerate((np.nan, np.inf, -1.0)):
            bad = asks.copy(); bad["reach"][k] = v
            refused(bad, b"ask %d" % k)
        bad = asks.copy(); bad["flags"][3] = 2
        refused(bad, b"ask 3 has unknown flag bits")
        bad = asks.copy(); bad["reserved"][1] = 1
        refused(bad, b"ask 1: reserved")
        refused(None, b"asks is NULL")
        refused(asks, b"capacity without a buffer", cap=4)
        refused(asks, b"at most", n_asks=L.BOX_QUERY_MAX_QUERIES + 1)
        args = L.BoxQueryArgs(0, 0); args.reserved[1] = 1
        refused(asks, b"reserved must be 0", args=C.byref(args))
        # a refused batch leaves the world alone: the next correct call answers
        rec = np.zeros(total, dt)
        assert fn(p._h, asks.ctypes.data, 4, None, rec.ctypes.data, total, C.byref(n), st.ctypes.data) == 0 and n.value == total and not st.any()
    # a removed entity is refused by name
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_DELETE, 8, 0, 0, (0, 0, 0, 0))
    check_frame(R, p, w, R.Camera((305.0, 305.0, 900.0), (0, 0, -1), 3000.0), False)
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    expect_error(R, RE_E_ARG, "ask 3: unknown entity 8", p.find_entities_around, asks["entity_id"], asks["reach"])
    expect_error(R, RE_E_ARG, "re_query_spheres_around: ask 3", p.find_entities_within_reach, asks["entity_id"], asks["reach"])
    assert ask_boxes(p, asks["entity_id"][:3], asks["reach"][:3])[0] == around_box_hits(w, range(10), asks["entity_id"][:3], asks["reach"][:3])[0]
    p.close(); w.close()


def test_contexts_give_their_memory_back(R):
    """re_debug_live_allocations is back at its starting value after contexts that have asked both questions, grown their buffers and been refused close"""
    live = R._capi.load().re_debug_live_allocations
    start = live()
    for atomic in (64, 16):
        p, w = build_pair(R, around_world(atomic), atomic=atomic)
        ask_boxes(p, [0, 1], 0.0); ask_spheres(p, [0, 1], 0.0)
        ask_boxes(p, np.tile(np.array([0, 1, 6], np.uint32), 200), 10.0); ask_spheres(p, np.tile(np.array([0, 1, 6], np.uint32), 200), 10.0)      # every buffer grows
        expect_error(R, RE_E_ARG, "ask 0", p.find_entities_around, [77], 0.0)
        assert live() > start
        p.close(); w.close()
    assert live() == start
