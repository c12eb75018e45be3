"""re_query_segments_first and re_query_spheres_nearest on the GPU: what each segment of a batch hits first and who is nearest to each point, reduced on the
device, against first_hits / nearest_hits of the sibling's full answer on the same pipeline and against the CPU rule (tests/first_hit_rule.py, checked in
tests/test_first_hit_rule.py): the records equal byte for byte."""
import ctypes as C

import numpy as np
import pytest

import oracle as ro
from helpers import oracle_camera
from box_query_rule import probe_world, probe_push_out, query_world, overflow_world, overflow_queries, N_CROWD
import segment_rule as seg
import sphere_rule as sph
from first_hit_rule import NO_ENTITY, segments_first, spheres_nearest, staged_batches, push_further, known_cases
from test_segment_rule import known_world
from test_gpu_parity import build_pair, check_frame, assert_clean_publication

pytestmark = pytest.mark.gpu

RE_E_ARG, RE_E_STATE = -1, -5
F32 = np.float32


@pytest.fixture(scope="module")
def R():
    import render_engine_amd as R
    return R


def seg6(p0, p1):
    return np.concatenate([np.asarray(p0, F32).reshape(-1, 3), np.asarray(p1, F32).reshape(-1, 3)], axis=1)


def sph4(c, r):
    return np.concatenate([np.asarray(c, F32).reshape(-1, 3), np.asarray(r, F32).reshape(-1, 1)], axis=1)


def same(got, want):
    """(records, found) pairs equal on the raw bytes"""
    return got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


def first_both_ways(R, p, w, ids, p0, p1, exclude=None, need=0, forbid=0):
    """the device's reduction; it equals first_hits of the full answer of the same pipeline, and the CPU rule.  Returns (first, found)."""
    got = p.find_first_along_segments(seg6(p0, p1), exclude=exclude, need=need, forbid=forbid)
    hits, _ = p.find_entities_along_segments(seg6(p0, p1), exclude=exclude, need_flags=need, forbid_flags=forbid)
    host = R.first_hits(hits, len(p0))
    rule = segments_first(w, ids, p0, p1, exclude=exclude, need=need, forbid=forbid)
    assert same(got, host), [(i, got[0][i], host[0][i]) for i in np.nonzero(got[0] != host[0])[0][:4]]
    assert same(got, rule), [(i, got[0][i], rule[0][i]) for i in np.nonzero(got[0] != rule[0])[0][:4]]
    return got


def nearest_both_ways(R, p, w, ids, c, r, exclude=None, need=0, forbid=0):
    got = p.find_nearest_within_radius(sph4(c, r), exclude=exclude, need=need, forbid=forbid)
    hits, _ = p.find_entities_within_radius(sph4(c, r), exclude=exclude, need_flags=need, forbid_flags=forbid)
    host = R.nearest_hits(hits, len(c))
    rule = spheres_nearest(w, ids, c, r, exclude=exclude, need=need, forbid=forbid)
    assert same(got, host), [(i, got[0][i], host[0][i]) for i in np.nonzero(got[0] != host[0])[0][:4]]
    assert same(got, rule), [(i, got[0][i], rule[0][i]) for i in np.nonzero(got[0] != rule[0])[0][:4]]
    return got


def n_found_of(lib, fn, p, batch):
    """*n_found of the raw call, and its records"""
    n = C.c_uint32(12345)
    out = np.zeros((max(len(batch), 1), 4), np.uint32)
    assert fn(p._h, batch.ctypes.data, len(batch), None, out.ctypes.data, C.byref(n)) == 0, lib.re_last_error(p._h)
    return n.value, out[:len(batch)]


@pytest.mark.parametrize("n,seed,spread,atomic", [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)])
def test_parity(R, n, seed, spread, atomic):
    """the two worlds of the CPU test after 0, 3 and 6 ticks with its batches -- 64 drawn segments, 64 drawn spheres, 64 shell spheres --, for both calls: plain,
    with every query's unexcluded winner excluded, and with a need / forbid filter; n_found exact"""
    L = R._capi
    ents = query_world(n, seed, spread, atomic)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = [int(i) for i in ents["id"]]

    def tick(cam):
        oc = oracle_camera(cam)
        check_frame(R, p, w, cam, False)
        n_o, oob_o = w.tick(oc, 0.05); t = p.tick(0.05)
        assert t["n_changed"] == n_o and t["n_out_of_bounds"] == len(oob_o)

    check_frame(R, p, w, R.Camera((8192, 8192, 8300), (0, 0, -1), 1000.0), False)
    found_total = runner_up = filtered = 0
    for stage, (p0, p1), (c, r), (sc, sr) in staged_batches(w, ids, seed, spread, atomic, tick):
        flt = dict(need=L.F_CAN_COLLIDE, forbid=L.F_STATIC)
        first, found = first_both_ways(R, p, w, ids, p0, p1)
        found_total += int(found.sum())
        ex = np.where(found, first["entity_id"], np.uint32(NO_ENTITY)).astype(np.uint32)
        second, found2 = first_both_ways(R, p, w, ids, p0, p1, exclude=ex)
        assert not (found2 & (second["entity_id"] == ex)).any()
        runner_up += int(found2.sum())
        filtered += int(first_both_ways(R, p, w, ids, p0, p1, **flt)[1].sum())
        for cc, rr in ((c, r), (sc, sr)):
            near, found = nearest_both_ways(R, p, w, ids, cc, rr)
            found_total += int(found.sum())
            ex = np.where(found, near["entity_id"], np.uint32(NO_ENTITY)).astype(np.uint32)
            second, found2 = nearest_both_ways(R, p, w, ids, cc, rr, exclude=ex)
            assert not (found2 & (second["entity_id"] == ex)).any()
            runner_up += int(found2.sum())
            filtered += int(nearest_both_ways(R, p, w, ids, cc, rr, **flt)[1].sum())
        assert_clean_publication(p)
    print(dict(found=found_total, runner_up=runner_up, filtered=filtered))
    assert found_total > 300 and runner_up > 200 and filtered > 50, (found_total, runner_up, filtered)
    p.close(); w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_known_answers_on_the_device(R, atomic):
    """the hand-worked cases of tests/first_hit_rule.py on both key encodings: ties at a positive value that the lower id wins -- in a unique section, in
    the shared section of 8 links --, the winner excluded, filtered out, no hit, the out-of-bounds entity behind the boundary extension"""
    s = F32(atomic) / F32(64.0)
    p, w = build_pair(R, known_world(atomic), atomic=atomic)
    check_frame(R, p, w, R.Camera((305.0 * s, 305.0 * s, 900.0 * s), (0, 0, -1), 3000.0), False)      # change requests belong to a frame
    for ch in (probe_push_out(), push_further()):
        w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    for name, kind, query, exclude, need, forbid, want in known_cases(atomic, 16384, R.F_STATIC):
        ex = np.array([exclude], np.uint32)
        if kind == "sphere":
            rec, found = nearest_both_ways(R, p, w, range(9), query[0][None, :], np.array([query[1]], F32), exclude=ex, need=need, forbid=forbid)
        else:
            rec, found = first_both_ways(R, p, w, range(9), query[0][None, :], query[1][None, :], exclude=ex, need=need, forbid=forbid)
        got = tuple(int(x) for x in rec.view(np.uint32).reshape(-1, 4)[0][1:]) if found[0] else None
        assert got == want, (name, kind, got, want)
        if want is None:
            assert rec.tobytes() == np.zeros(4, np.uint32).tobytes()
    assert_clean_publication(p)
    p.close(); w.close()


def crowd_world(R, atomic, winner_unique, winner_shared):
    """overflow_world with one member of each crowd a unit (half a unit) nearer to the queries below than the rest: its box reaches 1 (0.5) further down in x"""
    s = F32(atomic) / F32(64.0)
    ents = overflow_world(atomic)
    if winner_unique is not None:
        ents["original"][ents["id"] == winner_unique, 0] = F32(99.0) * s
    if winner_shared is not None:
        ents["original"][ents["id"] == winner_shared, 0] = F32(638.5) * s
    return ents


@pytest.mark.parametrize("atomic", [64, 16])
@pytest.mark.parametrize("place", ["tie", "first", "middle", "last"])
def test_overflow_world(R, atomic, place):
    """query 0: the winner among the 1101 rows of ONE unique section, 18 iterations of one wave; query 1: the winner among the 1100 members of ONE shared
    section, one lane's walk.  All members tie (the lowest id wins), or one of them -- the first, the last or a middle one by id -- is nearer.  Each call
    twice: the header block was left zero."""
    s = F32(atomic) / F32(64.0)
    wu, ws = dict(tie=(None, None), first=(100, 5000), middle=(100 + N_CROWD // 2, 5000 + N_CROWD // 2), last=(100 + N_CROWD - 1, 5000 + N_CROWD - 1))[place]
    ents = crowd_world(R, atomic, wu, ws)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = [int(i) for i in ents["id"]]
    if ws is not None:
        assert w.lookup(ws) == w.lookup(5000 + 1) and w.lookup(ws)[0] == 2 and w.lookup(wu) == w.lookup(5)      # the nearer ones stay in their sections
    _, p0, p1 = overflow_queries(atomic)
    c, r = np.array([[90, 114, 114], [630, 640, 640]], F32) * s, np.array([20, 10], F32) * s
    for _ in range(2):
        first, found = first_both_ways(R, p, w, ids, p0, p1)
        near, found_n = nearest_both_ways(R, p, w, ids, c, r)
        assert found.all() and found_n.all()
        assert first["entity_id"].tolist() == near["entity_id"].tolist() == [5 if wu is None else wu, 5000 if ws is None else ws]
        assert first["t_enter"].tolist() == ([F32(10.0) / F32(40.0), F32(9.0) / F32(20.0)] if wu is None else [F32(9.0) / F32(40.0), F32(8.5) / F32(20.0)])
        assert near["dist_sq"].tolist() == ([100.0 * s * s, 81.0 * s * s] if wu is None else [81.0 * s * s, 72.25 * s * s])
    # the all-hits siblings behind them still count their 2201 records: nothing was left in any header
    assert p.find_entities_along_segments(seg6(p0, p1), capacity=0)[1] == 2 * N_CROWD + 1 == p.find_entities_within_radius(sph4(c, r), capacity=0)[1]
    assert_clean_publication(p)
    p.close(); w.close()


def test_boundaries_of_the_calls(R):
    L = R._capi
    lib = L.load()
    n = C.c_uint32(77)
    one_s = np.zeros(1, L.SPHERE_DT); one_s["centre"] = 8100; one_s["radius"] = 50; one_s["exclude_entity"] = NO_ENTITY
    one_g = np.zeros(1, L.SEGMENT_DT); one_g["p0"] = 8100; one_g["p1"] = 8150; one_g["exclude_entity"] = NO_ENTITY
    out = np.zeros((4, 4), np.uint32)
    # before any upload
    pe = R.Pipeline()
    assert lib.re_query_spheres_nearest(pe._h, one_s.ctypes.data, 1, None, out.ctypes.data, C.byref(n)) == RE_E_STATE
    assert lib.re_query_segments_first(pe._h, one_g.ctypes.data, 1, None, out.ctypes.data, C.byref(n)) == RE_E_STATE
    pe.close()
    ents = query_world(600, 3, 120.0, 64)
    p, w = build_pair(R, ents)
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(3)
    c, r = sph.draw_spheres(w, ids, rng, 16384, 64, n=16)
    p0, p1 = seg.draw_segments(w, ids, rng, 16384, 64, n=16)
    sp = np.zeros(16, L.SPHERE_DT); sp["centre"], sp["radius"], sp["exclude_entity"] = c, r, NO_ENTITY
    sg = np.zeros(16, L.SEGMENT_DT); sg["p0"], sg["p1"], sg["exclude_entity"] = p0, p1, NO_ENTITY
    want_n, want_f = spheres_nearest(w, ids, c, r), segments_first(w, ids, p0, p1)
    assert want_n[1].sum() >= 8 and want_f[1].sum() >= 8
    calls = ((lib.re_query_spheres_nearest, sp, want_n, p.find_nearest_within_radius, sph4(c, r), "sphere"),
             (lib.re_query_segments_first, sg, want_f, p.find_first_along_segments, seg6(p0, p1), "segment"))
    for fn, batch, want, method, plain, word in calls:
        # n == 0; n_found is optional; the output is not
        n.value = 77
        assert fn(p._h, None, 0, None, None, C.byref(n)) == 0 and n.value == 0
        out16 = np.zeros((16, 4), np.uint32)
        assert fn(p._h, batch.ctypes.data, 16, None, out16.ctypes.data, None) == 0
        assert fn(p._h, batch.ctypes.data, 16, None, None, C.byref(n)) == RE_E_ARG and b"NULL" in lib.re_last_error(p._h)
        # the raw records: a query without a hit carries its index, the sentinel and two zero words; n_found counts the others
        nf, raw = n_found_of(lib, fn, p, batch)
        assert nf == int(want[1].sum())
        np.testing.assert_array_equal(raw[:, 0], np.arange(16))
        np.testing.assert_array_equal(raw[~want[1]][:, 1:], np.tile(np.array([NO_ENTITY, 0, 0], np.uint32), (int((~want[1]).sum()), 1)))
        np.testing.assert_array_equal(raw[want[1]], want[0].view(np.uint32).reshape(-1, 4)[want[1]])
        np.testing.assert_array_equal(raw, out16)
        assert same(method(batch), want) and same(method(plain), want)
        # refused batches name the query as the sibling does and leave the world alone
        for col, value in ((1, np.nan), (0, np.inf)):
            bad = plain.copy(); bad[3, col] = value
            with pytest.raises(R.RenderEngineError) as e:
                method(bad)
            assert f"({RE_E_ARG})" in str(e.value) and f"{word} 3" in str(e.value) and fn.__name__ in str(e.value), str(e.value)
        bad = batch.copy(); bad["reserved"][11] = 1
        with pytest.raises(R.RenderEngineError) as e:
            method(bad)
        assert f"{word} 11" in str(e.value) and "reserved" in str(e.value)
        args = L.BoxQueryArgs(0, 0); args.reserved[1] = 1
        assert fn(p._h, batch.ctypes.data, 16, C.byref(args), out16.ctypes.data, C.byref(n)) == RE_E_ARG and b"reserved" in lib.re_last_error(p._h)
        assert fn(p._h, batch.ctypes.data, L.BOX_QUERY_MAX_QUERIES + 1, None, out16.ctypes.data, C.byref(n)) == RE_E_ARG
        assert same(method(batch), want)
    bad = sph4(c, r); bad[6, 3] = -1.0
    with pytest.raises(R.RenderEngineError) as e:
        p.find_nearest_within_radius(bad)
    assert "sphere 6" in str(e.value) and "negative radius" in str(e.value)
    bad = sph4(c, r); bad[9] = [8000, 8000, 8000, 15 * 64]                                          # the cap: 15 atomic lengths
    with pytest.raises(R.RenderEngineError) as e:
        p.find_nearest_within_radius(bad)
    assert "sphere 9" in str(e.value) and "candidate cells" in str(e.value)
    bad = seg6(p0, p1); bad[5] = [1000, 1000, 1000, 1000 + 34 * 64, 1000 + 34 * 64, 1000 + 34 * 64]   # the cap: a diagonal of 34 atomic lengths
    with pytest.raises(R.RenderEngineError) as e:
        p.find_first_along_segments(bad)
    assert "segment 5" in str(e.value) and "candidate cells" in str(e.value)
    assert same(p.find_nearest_within_radius(sp), want_n) and same(p.find_first_along_segments(sg), want_f)
    # an all-miss batch
    far_c = np.tile(np.array([[300.0, 300.0, 300.0]], F32), (5, 1)); far_r = np.full(5, 10.0, F32)
    near, found = nearest_both_ways(R, p, w, ids, far_c, far_r)
    first, found_f = first_both_ways(R, p, w, ids, far_c, far_c + F32(20.0))
    assert not found.any() and not found_f.any() and near["entity_id"].sum() == 0 == first["entity_id"].sum()
    # n = 257 with one hit, in the last query: two tiles of the shared part
    qh = int(np.nonzero(want_n[1])[0][0]); gh = int(np.nonzero(want_f[1])[0][0])
    c257 = np.concatenate([np.tile(far_c[:1], (256, 1)), c[qh:qh + 1]]); r257 = np.concatenate([np.full(256, 10.0, F32), r[qh:qh + 1]])
    near, found = nearest_both_ways(R, p, w, ids, c257, r257)
    assert found.tolist() == [False] * 256 + [True] and near[256]["entity_id"] == want_n[0][qh]["entity_id"]
    a257 = np.concatenate([np.tile(far_c[:1], (256, 1)), p0[gh:gh + 1]]); b257 = np.concatenate([np.tile(far_c[:1] + F32(20.0), (256, 1)), p1[gh:gh + 1]])
    first, found = first_both_ways(R, p, w, ids, a257, b257)
    assert found.tolist() == [False] * 256 + [True] and first[256]["entity_id"] == want_f[0][gh]["entity_id"]
    # 4096 identical queries, all with the same winner
    near, found = p.find_nearest_within_radius(np.repeat(sph4(c, r)[qh:qh + 1], 4096, axis=0))
    assert found.all() and (near["query"] == np.arange(4096)).all()
    np.testing.assert_array_equal(near.view(np.uint32).reshape(-1, 4)[:, 1:], np.tile(want_n[0].view(np.uint32).reshape(-1, 4)[qh, 1:], (4096, 1)))
    first, found = p.find_first_along_segments(np.repeat(seg6(p0, p1)[gh:gh + 1], 4096, axis=0))
    assert found.all() and (first["query"] == np.arange(4096)).all()
    np.testing.assert_array_equal(first.view(np.uint32).reshape(-1, 4)[:, 1:], np.tile(want_f[0].view(np.uint32).reshape(-1, 4)[gh, 1:], (4096, 1)))
    # interleaved with the siblings, a frame and a tick
    cam = R.Camera((8192, 8192, 8300), (0, 0, -1), 1000.0)
    all_s = sph.sphere_hits(w, ids, c, r); all_g = seg.segment_hits(w, ids, p0, p1)
    for _ in range(2):
        assert same(p.find_nearest_within_radius(sp), want_n)
        assert sph.records_of(p.find_entities_within_radius(sp)[0]) == all_s
        assert same(p.find_first_along_segments(sg), want_f)
        assert seg.records_of(p.find_entities_along_segments(sg)[0]) == all_g
        check_frame(R, p, w, cam, False)
        assert same(p.find_first_along_segments(sg), want_f) and same(p.find_nearest_within_radius(sp), want_n)
    n_o, _ = w.tick(oracle_camera(cam), 0.05); t = p.tick(0.05)
    assert t["n_changed"] == n_o
    nearest_both_ways(R, p, w, ids, c, r); first_both_ways(R, p, w, ids, p0, p1)                     # the moved world, against the rule
    assert p.cull_and_pack(cam, asynchronous=True, copy=False) is None                               # nothing awaited: the query finishes the frame itself
    w.cull(oracle_camera(cam)); w.render(oracle_camera(cam))
    nearest_both_ways(R, p, w, ids, c, r); first_both_ways(R, p, w, ids, p0, p1)
    check_frame(R, p, w, cam, False)
    # a second context in the same process, unaffected and unaffecting
    p2, w2 = build_pair(R, probe_world(64))
    a, ra = np.array([[32, 15, 15]], F32), np.array([40], F32)
    near2, found2 = nearest_both_ways(R, p2, w2, range(6), a, ra)
    assert found2[0] and near2["entity_id"][0] == 0
    first2, found2 = first_both_ways(R, p2, w2, range(6), np.array([[0, 15, 15]], F32), np.array([[128, 15, 15]], F32))
    assert found2[0] and first2["entity_id"][0] == 4 and first2["t_enter"][0] == 0.0
    nearest_both_ways(R, p, w, ids, c, r)
    assert_clean_publication(p); assert_clean_publication(p2)
    p2.close(); w2.close(); p.close(); w.close()


def test_sample_scene_shot_and_reach(R):
    """the 45-entity sample scene through the new calls: the shot from the user entity (excluded) towards the mine producer, and the user entity's reach"""
    from test_sample_scene import scene
    ents, world, camd = scene()
    p, w = build_pair(R, ents, outline=world["outline_length"], atomic=world["atomic_length"])
    ids = [int(i) for i in ents["id"]]
    a = w.entity(0)["aabb"].reshape(3, 2).mean(axis=1)[None, :].astype(F32)
    b = w.entity(44)["aabb"].reshape(3, 2).mean(axis=1)[None, :].astype(F32)
    ra = np.array([146.0], F32)                                                   # the mine producer's box is sqrt(21250) = 145.8 away
    ex = np.array([0], np.uint32)
    for _ in range(2):
        first, found = first_both_ways(R, p, w, ids, a, b, exclude=ex)
        assert found[0] and first["entity_id"][0] == seg.first_hits_brute(seg.segment_hits(w, ids, a, b, exclude=ex), 1)[0][1]
        assert first_both_ways(R, p, w, ids, a, b)[0]["entity_id"][0] == 0       # (unexcluded, the shooter is its own first hit)
        near, found = nearest_both_ways(R, p, w, ids, a, ra, exclude=ex)
        assert found[0] and near["entity_id"][0] == sph.nearest_brute(sph.sphere_hits(w, ids, a, ra, exclude=ex), 1)[0][1]
        assert nearest_both_ways(R, p, w, ids, a, ra)[0]["entity_id"][0] == 0
        p.cull_and_pack(R.Camera(camd["position"], camd["direction"], camd["far"]))
    assert_clean_publication(p)
    p.close(); w.close()


def test_cpp_mirror_first_hit_and_nearest():
    """include/render_engine_hip.hpp: Pipeline::find_first_along_segments and find_nearest_within_radius -- before the first frame, with the asking entity
    excluded, filtered, with an instance registered after frames have run, ties (tests/cpp/first_hit_shim_test.cpp)"""
    import os
    import subprocess
    from render_engine_amd import build as libbuild
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(here, "cpp", "_build", "first_hit_shim_test")
    lib_dir = os.path.dirname(libbuild.build_library())
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(here), "include"),
                           os.path.join(here, "cpp", "first_hit_shim_test.cpp"), "-o", exe, "-L", lib_dir, "-lrender_engine_hip", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "OK first hits" in out.stdout, out.stdout + out.stderr
