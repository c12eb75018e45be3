"""re_query_spheres on the GPU: the entities within a radius of each point of a batch (an explosion, a proximity trigger, a producer looking for
asteroids) through the C ABI against its CPU restatement over the oracle (tests/sphere_rule.py, itself checked against the oracle's section decisions in
tests/test_sphere_rule.py): the pairs equal, dist_sq bit for bit, side equal."""
import ctypes as C

import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from box_query_rule import probe_world, probe_push_out, query_world, overflow_world
from sphere_rule import NO_ENTITY, sphere_hits, records_of, nearest_brute, draw_spheres
from test_segment_rule import known_world
from test_sphere_rule import known_spheres, overflow_spheres
from test_gpu_parity import build_pair, check_frame, random_changes, assert_clean_publication
from test_logic_rule import camera_draw

pytestmark = pytest.mark.gpu

RE_E_ARG, RE_E_STATE = -1, -5
F32 = np.float32


@pytest.fixture(scope="module")
def R():
    import render_engine_amd as R
    return R


def ask(p, c, r, exclude=None, **k):
    """(sorted records (query, entity, bits of dist_sq, side), total) of one call; the pairs are distinct and as many as the total"""
    hits, n_total = p.find_entities_within_radius(np.concatenate([np.asarray(c, F32).reshape(-1, 3), np.asarray(r, F32).reshape(-1, 1)], axis=1), exclude=exclude, **k)
    got = records_of(hits)
    assert len(got) == n_total == len({rec[:2] for rec in got}), (len(got), n_total)
    return got, n_total


def expect_error(R, code, text, fn, *a, **k):
    with pytest.raises(R.RenderEngineError) as e:
        fn(*a, **k)
    assert f"({code})" in str(e.value) and text in str(e.value), str(e.value)


def describe(got, want):
    return sorted(set(got) - set(want))[:6], sorted(set(want) - set(got))[:6]


@pytest.mark.parametrize("n,seed,spread,atomic", [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)])
def test_sphere_query_parity(R, n, seed, spread, atomic):
    """ten frames of cull, query, tick over the mixed world of test_box_query_parity with a change batch every third frame (add-entity among them):
    64 spheres a frame, every second with its nearest entity excluded; the sorted records equal the rule's, dist_sq bit for bit; frames 4 and 7 with the
    filter, frame 5 behind an asynchronous cull and tick"""
    L = R._capi
    ents = query_world(n, seed, spread, atomic)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(seed)
    total = filtered = excluded = 0
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
        c, r = draw_spheres(w, ids, rng, 16384, atomic)
        flt = dict(need_flags=L.F_CAN_COLLIDE, forbid_flags=L.F_STATIC) if f in (4, 7) else {}
        # every second sphere excludes the nearest entity it would otherwise report
        free = sphere_hits(w, ids, c, r, need=flt.get("need_flags", 0), forbid=flt.get("forbid_flags", 0))
        ex = np.full(len(c), NO_ENTITY, np.uint32)
        for i, rec in enumerate(nearest_brute(free, len(c))):
            if i % 2 and rec is not None:
                ex[i] = rec[1]
        want = sphere_hits(w, ids, c, r, exclude=ex, need=flt.get("need_flags", 0), forbid=flt.get("forbid_flags", 0))
        excluded += len(free) - len(want)
        got, n_total = ask(p, c, r, exclude=ex, **flt)
        assert got == want, (f, n_total, len(want), describe(got, want))
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
    print(dict(total=total, filtered=filtered, excluded=excluded))
    assert total > 5000 and filtered > 100 and excluded > 20, (total, filtered, excluded)
    p.close(); w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_known_answers_on_the_device(R, atomic):
    """the hand-worked spheres of tests/test_sphere_rule.py on both key encodings (256 sections per axis: compact 32-bit stream keys; 1024: the full
    keys), then a static entity of the frozen cache that is moved -- reported once, at its live box, the ghost never -- and a deleted and re-created id"""
    L = R._capi
    s = F32(atomic) / F32(64.0)
    ents = known_world(atomic)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = list(range(9))
    # change requests belong to a frame: one is drawn first (and the static render cache freezes with entity 7 in it)
    cam = R.Camera((305.0 * s, 305.0 * s, 900.0 * s), (0, 0, -1), 3000.0)
    check_frame(R, p, w, cam, False)
    ch = probe_push_out()
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    c, r, ex, want = known_spheres(atomic)
    got, _ = ask(p, c, r, exclude=ex)
    assert got == want == sphere_hits(w, ids, c, r, exclude=ex), describe(got, want)
    assert [rec[:2] for rec in ask(p, c, r, exclude=ex, need_flags=L.F_OOB_LOGIC)[0]] == [(9, 3)]
    # the static entity 7 ([300, 310]^3) is moved by +500 in x: 10 below its old minimum face nothing is left, 10 below the new one ([800, 810]) it is met once
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_MODIFY, 7, L.C_POSITION, 0, (500.0 * s, 0.0, 0.0, 0.0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    a = np.array([[290, 305, 305], [790, 305, 305], [305, 305, 305]], F32) * s; ra = np.array([10, 10, 0], F32) * s
    want7 = [(1, 7, int((F32(100.0) * s * s).view(np.uint32)), 1)]
    assert ask(p, a, ra)[0] == want7 == sphere_hits(w, ids, a, ra)
    assert ask(p, a, ra, need_flags=L.F_STATIC)[0] == [] == sphere_hits(w, ids, a, ra, need=L.F_STATIC)      # (a moved entity is re-added as not static: the flag follows the tree)
    check_frame(R, p, w, cam, False)                                                                      # the ghost is drawn ...
    assert ask(p, a, ra)[0] == want7                                                                      # ... and still not reported
    # a deleted entity is no longer reported; its id, created again, is reported at the new place
    a = np.array([[405, 405, 405], [405, 1405, 405]], F32) * s; ra = np.array([0, 2], F32) * s
    assert ask(p, a, ra)[0] == [(0, 8, 0, 0)] == sphere_hits(w, ids, a, ra)
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_DELETE, 8, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    assert ask(p, a, ra)[0] == [] == sphere_hits(w, ids, a, ra)
    add = ents[ents["id"] == 8].copy(); add["pos"][0] = (0.0, 1000.0 * s, 0.0)
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (L.CHANGE_ADD_ENTITY, 8, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT), added=to_oracle(add)); p.apply_changes(ch, added=add)
    assert ask(p, a, ra)[0] == [(1, 8, 0, 0)] == sphere_hits(w, ids, a, ra)
    assert_clean_publication(p)
    p.close(); w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_staging_overflow(R, atomic):
    """more records in one workgroup than it stages (BOXQ_HITBUF = 1024; tests/test_sphere_rule.py holds the precondition): sphere 0 makes one wave walk
    1101 hit rows of one unique section (the overflow of the row walk), sphere 1 makes one lane emit the 1100 members of one shared section (the
    overflow of the shared part); dist_sq bit for bit"""
    ents = overflow_world(atomic)
    p, w = build_pair(R, ents, atomic=atomic)
    ids = [int(i) for i in ents["id"]]
    c, r = overflow_spheres(atomic)
    both = np.concatenate([c, r[:, None]], axis=1)
    want = sphere_hits(w, ids, c, r)
    assert len(want) == 2201
    for _ in range(2):                                                 # the same call again: the header was left zero
        got, n_total = ask(p, c, r)
        assert got == want and n_total == len(want), describe(got, want)
    hits, n_total = p.find_entities_within_radius(both, capacity=0)
    assert n_total == len(want) and len(hits) == 0
    hits, n_total = p.find_entities_within_radius(both, capacity=1050)       # above the stage, below the total
    assert n_total == len(want) and len(hits) == 1050 and len(set(records_of(hits))) == 1050 and set(records_of(hits)) <= set(want)
    assert ask(p, c, r) == (want, len(want))
    assert_clean_publication(p)
    p.close(); w.close()


def test_boundaries_of_the_call(R):
    L = R._capi
    lib = L.load()
    n = C.c_uint32(77)
    one = np.zeros(1, L.SPHERE_DT); one["centre"] = 8100; one["radius"] = 50; one["exclude_entity"] = NO_ENTITY
    # before any upload
    pe = R.Pipeline()
    assert lib.re_query_spheres(pe._h, one.ctypes.data, 1, None, None, 0, C.byref(n)) == RE_E_STATE
    pe.close()
    ents = query_world(600, 3, 120.0, 64)
    p, w = build_pair(R, ents)
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(3)
    c, r = draw_spheres(w, ids, rng, 16384, 64, n=16)
    sph = np.zeros(16, L.SPHERE_DT); sph["centre"], sph["radius"], sph["exclude_entity"] = c, r, NO_ENTITY
    both = np.concatenate([c, r[:, None]], axis=1)
    want = sphere_hits(w, ids, c, r)
    assert len(want) > 50
    # n == 0
    assert lib.re_query_spheres(p._h, None, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.re_query_spheres(p._h, sph.ctypes.data, len(sph), None, None, 0, None) == 0           # n_total is optional
    # capacity 0: the total is exact; capacity 7 of more: 7 distinct correct records, the total exact
    hits, n_total = p.find_entities_within_radius(sph, capacity=0)
    assert n_total == len(want) and len(hits) == 0
    hits, n_total = p.find_entities_within_radius(sph, capacity=7)
    assert n_total == len(want) and len(hits) == 7 and len(set(records_of(hits))) == 7 and set(records_of(hits)) <= set(want)
    assert ask(p, c, r)[0] == want
    # refused batches name the sphere and leave the world alone: the next correct call answers
    bad = both.copy(); bad[3, 1] = np.nan
    expect_error(R, RE_E_ARG, "sphere 3", p.find_entities_within_radius, bad)
    bad = both.copy(); bad[5, 0] = np.inf
    expect_error(R, RE_E_ARG, "sphere 5", p.find_entities_within_radius, bad)
    bad = both.copy(); bad[4, 3] = np.inf
    expect_error(R, RE_E_ARG, "sphere 4", p.find_entities_within_radius, bad)
    bad = both.copy(); bad[6, 3] = -1.0
    expect_error(R, RE_E_ARG, "sphere 6", p.find_entities_within_radius, bad)
    bad = both.copy(); bad[7, 2] = np.nextafter(F32(-64.0 * 16384.0), F32(-np.inf))                  # the magnitude limit: 64 outline lengths, on a centre and on the radius
    expect_error(R, RE_E_ARG, "sphere 7", p.find_entities_within_radius, bad)
    bad = both.copy(); bad[8, 3] = np.nextafter(F32(64.0 * 16384.0), F32(np.inf))
    expect_error(R, RE_E_ARG, "sphere 8", p.find_entities_within_radius, bad)
    bad = both.copy(); bad[9] = [8000, 8000, 8000, 15 * 64]                                          # the cap: 15 atomic lengths (14 pass, below)
    expect_error(R, RE_E_ARG, "sphere 9", p.find_entities_within_radius, bad)
    bad = sph.copy(); bad["reserved"][11] = 1
    expect_error(R, RE_E_ARG, "sphere 11", p.find_entities_within_radius, bad)
    args = L.BoxQueryArgs(0, 0); args.reserved[1] = 1
    assert lib.re_query_spheres(p._h, sph.ctypes.data, len(sph), C.byref(args), None, 0, C.byref(n)) == RE_E_ARG
    assert b"reserved" in lib.re_last_error(p._h)
    assert lib.re_query_spheres(p._h, sph.ctypes.data, len(sph), None, None, 4, C.byref(n)) == RE_E_ARG           # capacity without a buffer
    assert lib.re_query_spheres(p._h, sph.ctypes.data, L.BOX_QUERY_MAX_QUERIES + 1, None, None, 0, C.byref(n)) == RE_E_ARG
    assert ask(p, c, r)[0] == want
    # the largest radius the header promises, and a centre at the magnitude limit, far outside the world: answered
    big_c, big_r = np.array([[8000, 8000, 8000], [64.0 * 16384.0, 8192, 8192]], F32), np.array([14 * 64, 100], F32)
    assert ask(p, big_c, big_r)[0] == sphere_hits(w, ids, big_c, big_r)
    # 4096 identical spheres: every query index appears, with the same set (the staging overflow path; more than one tile of the shared part)
    q0 = min(range(16), key=lambda i: abs(sum(1 for rec in want if rec[0] == i) - 40))       # (a sphere of about 40 hits: 160 K records)
    rec0 = sorted(rec[1:] for rec in want if rec[0] == q0)
    assert len(rec0) >= 20
    hits, n_total = p.find_entities_within_radius(np.repeat(both[q0:q0 + 1], 4096, axis=0))
    assert n_total == 4096 * len(rec0) == len(hits)
    order = np.lexsort((hits["entity_id"], hits["query"]))
    np.testing.assert_array_equal(hits["query"][order], np.repeat(np.arange(4096, dtype=np.uint32), len(rec0)))
    np.testing.assert_array_equal(hits["entity_id"][order], np.tile(np.array([rec[0] for rec in rec0], np.uint32), 4096))
    np.testing.assert_array_equal(hits["dist_sq"][order].view(np.uint32), np.tile(np.array([rec[1] for rec in rec0], np.uint32), 4096))
    np.testing.assert_array_equal(hits["side"][order], np.tile(np.array([rec[2] for rec in rec0], np.uint32), 4096))
    # a second context in the same process, unaffected and unaffecting
    p2, w2 = build_pair(R, probe_world(64))
    a, ra = np.array([[32, 15, 15]], F32), np.array([40], F32)
    assert [rec[:2] for rec in ask(p2, a, ra)[0]] == [(0, 0), (0, 1), (0, 2), (0, 4)] == [rec[:2] for rec in sphere_hits(w2, range(6), a, ra)]
    assert ask(p, c, r)[0] == want
    assert ask(p2, a, ra)[1] == 4
    assert_clean_publication(p); assert_clean_publication(p2)
    p2.close(); w2.close(); p.close(); w.close()


def test_sample_scene_reach_of_the_user_entity(R):
    """the 45-entity sample scene: a sphere around the user entity (excluded) that reaches the mine producer; the nearest hit is the rule's"""
    from test_sample_scene import scene
    ents, world, camd = scene()
    p, w = build_pair(R, ents, outline=world["outline_length"], atomic=world["atomic_length"])
    ids = [int(i) for i in ents["id"]]
    a = w.entity(0)["aabb"].reshape(3, 2).mean(axis=1)[None, :].astype(F32)
    ra = np.array([146.0], F32)                                                   # the mine producer's box is sqrt(21250) = 145.8 away
    ex = np.array([0], np.uint32)
    want = sphere_hits(w, ids, a, ra, exclude=ex)
    assert (0, 44) in [rec[:2] for rec in want] and (0, 0) not in [rec[:2] for rec in want]
    assert nearest_brute(sphere_hits(w, ids, a, ra), 1)[0][:2] == (0, 0)           # (unexcluded, the asking entity is its own nearest: dist_sq 0, side 0)
    for _ in range(2):
        hits, n_total = p.find_entities_within_radius(np.concatenate([a, ra[:, None]], axis=1), exclude=ex)
        assert records_of(hits) == want and n_total == len(want)
        nearest, found = R.nearest_hits(hits, 1)
        assert found[0] and records_of(nearest) == [nearest_brute(want, 1)[0]]
        p.cull_and_pack(R.Camera(camd["position"], camd["direction"], camd["far"]))
    assert_clean_publication(p)
    p.close(); w.close()


def test_cpp_mirror_find_entities_within_radius():
    """include/render_engine_hip.hpp: Pipeline::find_entities_within_radius and nearest_hits -- before the first frame, with the asking entity excluded,
    filtered, with an instance registered after frames have run, spheres that touch a face and an edge (tests/cpp/sphere_query_shim_test.cpp)"""
    import os
    import subprocess
    from render_engine_amd import build as libbuild
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(here, "cpp", "_build", "sphere_query_shim_test")
    lib_dir = os.path.dirname(libbuild.build_library())
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(here), "include"),
                           os.path.join(here, "cpp", "sphere_query_shim_test.cpp"), "-o", exe, "-L", lib_dir, "-lrender_engine_hip", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "OK sphere queries" in out.stdout, out.stdout + out.stderr
