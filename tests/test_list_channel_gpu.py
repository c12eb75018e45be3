"""The record-list flows (re_logic_list, re_query_boxes, re_collide) at the edges of what they share: the 32-shard sign-off of k_logic_list and
k_box_query (list_sign_off, re_kernels.h) around 32 workgroups, the header it leaves zero for the next call, the two channels and the collision
header side by side on one context (ListChannel, re_api.hip), and their lifetime across uploads and re_destroy."""
import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from logic_rule import logic_call_counts, logic_records
from box_query_rule import box_hits, query_world, draw_boxes
from test_gpu_parity import build_pair, check_frame, sorted_pairs, assert_clean_publication
from test_logic_gpu import TYPE_A, TYPE_C, as_tuples, send_types, table_of, types_by_id
from test_box_query_gpu import ask
from test_segment_query_gpu import ask as ask_segments

pytestmark = pytest.mark.gpu

CAM_LATTICE = ((8160.0, 8160.0, 9300.0), (0, 0, -1), 2000.0)      # sees the whole 7 x 7 x 7 lattice (test_logic_gpu.test_compaction_edges)
CAM_MIXED = ((8192.0, 8192.0, 8300.0), (0, 0, -1), 1500.0)


@pytest.fixture(scope="module")
def R():
    import render_engine_amd as R
    return R


@pytest.fixture(scope="module")
def crowd(R):
    """48 non-static entities in each of the 343 sections of the lattice, one frame drawn with all of them in view: every typed row yields a record.
    (pipeline, ids in row order, the rule's calls)"""
    base = R.synthetic.lattice_world(cells_per_axis=7, first_cell=124, spinner_every=1)
    ents = np.concatenate([base] * 48)
    ents["id"] = np.arange(len(ents), dtype=np.uint32)
    assert len(ents) == 16464 and not np.any(ents["flags"] & R.F_STATIC)
    p, w = build_pair(R, ents)
    ids = np.ascontiguousarray(ents["id"], np.uint32)
    cam = R.Camera(*CAM_LATTICE)
    check_frame(R, p, w, cam, False)
    calls = logic_call_counts(w, oracle_camera(cam), [int(i) for i in ids])
    assert sorted(calls) == ids.tolist() and set(calls.values()) == {1}
    w.close()
    p.set_entity_logic([(TYPE_C, R._capi.LOGIC_ENTITY | R._capi.LOGIC_RANDOM)])
    yield p, ids, calls
    p.close()


@pytest.mark.parametrize("k,workgroups", [(1, 1), (7936, 31), (7937, 32), (8192, 32), (8193, 33), (16385, 65)])
def test_logic_list_sign_off_edges(R, crowd, k, workgroups):
    """k listed rows, every one of them a record: one workgroup, one short of the 32 shards, exactly 32 (the last of them with one lane, and full), one
    more than the shards, and two rounds of them plus one.  Twice in a row: the first call left the header zero."""
    p, ids, calls = crowd
    assert (k + 255) // 256 == workgroups
    table = [(TYPE_C, R._capi.LOGIC_ENTITY | R._capi.LOGIC_RANDOM)]
    p.set_entity_types(ids, None)
    pick = ids[(np.arange(k) * 5) % len(ids)]                         # 5 and 16464 are coprime: k distinct entities spread over the rows
    types = {int(i): TYPE_C for i in pick}
    assert len(types) == k
    send_types(p, types)
    want = logic_records(calls, types, table)
    assert len(want) == k
    for again in range(2):
        rec, n_total = p.logic_calls()
        assert n_total == k == len(rec), (again, n_total)
        assert as_tuples(rec) == want, again
    assert_clean_publication(p)


@pytest.fixture(scope="module")
def lattice(R):
    """the 343-entity lattice: no shared sections, so k_box_query's grid is the number of boxes"""
    ents = R.synthetic.lattice_world(cells_per_axis=7, first_cell=124, spinner_every=1)
    p, w = build_pair(R, ents)
    assert p.stats()["n_shared_sections"] == 0
    yield p, w, [int(i) for i in ents["id"]]
    p.close(); w.close()


@pytest.fixture(scope="module")
def mixed(R):
    """a mixed world whose shared sections fit one 256-entry chunk: k_box_query's grid is the number of boxes plus one (up to 256 boxes)"""
    ents = query_world(600, 3, 120.0, 64)
    p, w = build_pair(R, ents)
    assert 0 < p.stats()["n_shared_sections"] <= 256
    yield p, w, [int(i) for i in ents["id"]]
    p.close(); w.close()


def box_edge(p, w, ids, n, seed):
    boxes = draw_boxes(w, ids, np.random.default_rng(seed), 16384, n=n)
    want = box_hits(w, ids, boxes)
    assert len(want) > n // 2
    for again in range(2):                                             # the first call left the header zero
        got, n_total = ask(p, boxes)
        assert n_total == len(want) and got == want, (again, n_total, len(want))
    assert_clean_publication(p)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_box_query_sign_off_edges(R, lattice, n):
    """n boxes == n workgroups around the 32 shards of the sign-off"""
    box_edge(*lattice, n, 100 + n)


@pytest.mark.parametrize("n", [30, 31, 32])
def test_box_query_sign_off_edges_with_shared_sections(R, mixed, n):
    """n boxes and one workgroup of shared sections: 31, 32 and 33 workgroups"""
    box_edge(*mixed, n, 200 + n)


def typed_pipeline(R, ents, types, table, cam):
    """a fresh context with the world, the types and one frame drawn"""
    p = R.Pipeline(16384, 64)
    assert p.register_model_instances(ents) == 0
    send_types(p, types); p.set_entity_logic(table)
    p.cull_and_pack(cam)
    return p


def test_flows_interleaved_on_one_context(R):
    """logic list, box query, collision pass, another box query, logic list behind one cull_and_pack: every answer is the one the call gives alone on a
    fresh context (and the rule's) -- the two channels and the collision header share neither state nor sequence numbers"""
    ents = query_world(600, 3, 120.0, 64)
    ids = [int(i) for i in ents["id"]]
    types, table = types_by_id(ids), table_of(R)
    cam = R.Camera(*CAM_MIXED)
    w = ro.World(16384, 64)
    assert w.register(to_oracle(ents)) == 0
    oc = oracle_camera(cam)
    w.cull(oc)
    boxes_a = draw_boxes(w, ids, np.random.default_rng(7), 16384, n=33)
    boxes_b = draw_boxes(w, ids, np.random.default_rng(8), 16384, n=20)
    want_logic = logic_records(logic_call_counts(w, oc, ids), types, table)
    want_a, want_b = box_hits(w, ids, boxes_a), box_hits(w, ids, boxes_b)
    want_col = sorted_pairs(w.collide(oc))
    w.close()
    assert len(want_logic) > 50 and len(want_a) > 33 and len(want_b) > 20 and len(want_col) > 100

    def alone(call):
        q = typed_pipeline(R, ents, types, table, cam)
        out = call(q)
        assert_clean_publication(q)
        q.close()
        return out

    logic = lambda q: as_tuples(q.logic_calls()[0])
    collide = lambda q: sorted_pairs(q.collide()[0])
    steps = [(logic, want_logic), (lambda q: ask(q, boxes_a)[0], want_a), (collide, want_col), (lambda q: ask(q, boxes_b)[0], want_b), (logic, want_logic)]
    p = typed_pipeline(R, ents, types, table, cam)
    for i, (call, want) in enumerate(steps):
        got = call(p)
        np.testing.assert_array_equal(got, want, err_msg=f"step {i} against the rule")
        if i < 4:                                                      # (the last step is the first one again)
            np.testing.assert_array_equal(got, alone(call), err_msg=f"step {i} against the call alone")
    assert_clean_publication(p)
    p.close()


def test_flows_across_uploads_and_destroy(R):
    """create, all three flows, a world of another size, all three again, destroy -- twice in one process: the same answers both times, no error,
    and both publication counters 0"""
    worlds = [query_world(600, 3, 120.0, 64), query_world(1500, 13, 150.0, 64)]
    cam = R.Camera(*CAM_MIXED)
    boxes = np.array([[8100, 8300] * 3, [8000, 8192, 8150, 8400, 8192, 8250]], np.float32)
    seen = []
    for cycle in range(2):
        p = R.Pipeline(16384, 64)
        p.set_entity_logic([(TYPE_A, R._capi.LOGIC_ENTITY)])
        totals = []
        for ents in worlds:
            p.replace_world(ents)
            p.set_entity_types(np.ascontiguousarray(ents["id"], np.uint32), np.full(len(ents), TYPE_A, np.uint64))
            p.cull_and_pack(cam)
            n_logic, n_hits, n_pairs = p.logic_calls()[1], ask(p, boxes)[1], p.collide()[1]
            assert n_logic > 0 and n_hits > 0 and n_pairs > 0
            totals.append((n_logic, n_hits, n_pairs))
        assert totals[0] != totals[1]
        assert_clean_publication(p)
        p.close()
        seen.append(totals)
    assert seen[0] == seen[1]


def test_context_owns_its_memory(R):
    """one RE_CFG_PROBE context through everything that allocates lazily, three times over: the blocks of device and pinned memory the library holds
    (re_debug_live_allocations) are as many after every cycle -- nothing accumulates across uploads --, re_destroy gives back every one of them, the
    answers of the first cycle are those of the third, and both publication counters stay 0.  (A probe context re-buckets a tick's movers on the host
    path; the scratch of the device path is covered by the plain context at the end.)"""
    L, live = R._capi, R._capi.load().re_debug_live_allocations
    worlds = [query_world(600, 3, 120.0, 64), query_world(1500, 13, 150.0, 64)]
    static_world = R.synthetic.lattice_world(cells_per_axis=20, first_cell=118)
    assert not np.any(static_world["flags"] & (R.F_HAS_VEL | R.F_HAS_ROTVEL))
    cam = R.Camera(*CAM_MIXED)
    boxes = np.array([[8100, 8300] * 3, [8000, 8192, 8150, 8400, 8192, 8250]], np.float32)
    p0 = np.array([[8100, 8100, 8100], [8000, 8250, 8192]], np.float32); p1 = np.array([[8300, 8300, 8300], [8400, 8150, 8200]], np.float32)

    def flows(p, ents):
        """a synchronous frame and every flow behind it; what they answered"""
        ids = np.ascontiguousarray(ents["id"], np.uint32)
        p.set_entity_types(ids, np.full(len(ids), TYPE_A, np.uint64))
        vis = p.cull_and_pack(cam)
        out = [vis["total"], as_tuples(p.logic_calls()[0]), ask(p, boxes)[0], ask_segments(p, p0, p1)[0], sorted_pairs(p.collide()[0]),
               p.visible_lights(cam, R.F_LIGHT_SPOT).tolist(), p.get_indexes_for_components([L.C_POSITION, L.C_VELOCITY]).tolist(), p.export_entities(ids[:40]).tobytes()]
        assert out[0] > 0 and len(out[1]) > 0 and len(out[2]) > 0 and len(out[3]) > 0 and len(out[4]) > 0 and len(out[6]) > 0
        return out

    def cycle(p):
        answers = []
        ents = worlds[0]
        p.replace_world(ents)
        answers.append(flows(p, ents))
        still = int(ents["id"][-1])                                       # a border entity of query_world: no Velocity, so no slot of the dynamic table
        assert not ents["flags"][-1] & (R.F_HAS_VEL | R.F_HAS_ROTVEL)
        add = ents[:1].copy(); add["id"] = int(ents["id"].max()) + 1; add["pos"] += np.float32(7.5)
        ch = np.zeros(3, R.CHANGE_DT)
        ch[0] = (L.CHANGE_MODIFY, int(ents["id"][5]), L.C_POSITION, 0, (8200, 8190, 8210, 0))      # (the small-batch staging block)
        ch[1] = (L.CHANGE_ADD_ENTITY, int(add["id"][0]), 0, 0, (0, 0, 0, 0))                         # row_cap == n after an upload: every column grows
        ch[2] = (L.CHANGE_MODIFY, still, L.C_VELOCITY, 0, (3, 0, 0, 0))                             # the dynamic table grows
        answers.append(p.apply_changes(ch, added=add))
        t = p.tick(0.25)
        assert t["n_changed"] > 0 and t["n_rebucket"] > 0                  # movers: the re-bucket scratch exists
        answers.append(t)
        p.replace_world(worlds[1])
        answers.append(flows(p, worlds[1]))
        p.replace_world(static_world)
        switches = p.stats()["reserved"]
        p.cull_and_pack(cam); p.tick(0.016)                                # the static cache freezes here
        for i in range(12):
            c2 = R.Camera((8192 + 9.5 * i, 8192 - 4.25 * i, 8500 - 11.0 * i), (0.02 * i, 0.01 * i, -1), 900.0)
            p.cull_and_pack(c2, asynchronous=True, copy=False, defer_pack=True, two_lanes=True); p.tick(0.016, asynchronous=True)
        vis, _ = p.wait(copy=True)
        answers.append((vis["total"], vis["ids"].tobytes()))
        assert p.stats()["reserved"] - switches >= 12                      # lane switches: the second lane really existed
        p.replace_world(worlds[0])
        return answers

    base = live()
    p = R.Pipeline(16384, 64, flags=L.CFG_PROBE)
    p.set_entity_logic([(TYPE_A, L.LOGIC_ENTITY)])
    p.set_model_lod(int(worlds[0]["model_index"][0]), int(worlds[0]["render_system"][0]), [0, 150, 300], [150, 300, 450])
    seen, counts = [], []
    for _ in range(3):
        seen.append(cycle(p)); counts.append(live() - base)
    print("live blocks after each cycle:", counts)
    assert counts[0] > 0 and counts[0] == counts[1] == counts[2], counts
    assert_clean_publication(p)
    for a, b in zip(seen[0], seen[2]):
        np.testing.assert_equal(a, b)
    p.close()
    assert live() == base
    # the device re-bucket's scratch and pinned staging block (plain contexts only): allocated by a tick with movers, gone with the next upload
    q = R.Pipeline(16384, 64)
    counts = []
    for _ in range(3):
        q.replace_world(worlds[0]); q.cull_and_pack(cam)
        counts.append(live())
        assert q.tick(0.25)["n_rebucket"] > 0 and live() > counts[-1] + 30      # (more than 30 scratch buffers)
    assert q.stats()["n_device_rebuckets"] == 3 and counts[1] == counts[2], counts
    assert_clean_publication(q)
    q.close()
    assert live() == base
