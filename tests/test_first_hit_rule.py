"""The rule of re_query_segments_first / re_query_spheres_nearest (tests/first_hit_rule.py) on the CPU: the 64-bit key orders hits as (value, entity id)
does, the draws the GPU tests use hold ties, positive values and queries without a hit, hand-worked known answers, the second pass of the device reaches
the winner and everything tied with it through its shrunk prunes, and the call exists in every layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from box_query_rule import MAX_CELLS, query_cell_ranges, probe_push_out, query_world
import segment_rule as seg
import sphere_rule as sph
from first_hit_rule import (F32, NO_ENTITY, KEY_NONE, pack_keys, as_arrays, winners_by_key, reduced_records, segments_first, spheres_nearest,
                            shrunk_prune_passes_segment, shrunk_prune_passes_sphere, pick_reaches, draw_shell_spheres, staged_batches, push_further, known_cases)
from test_segment_rule import known_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)]      # n, seed, spread, atomic: the worlds of test_box_query_rule.py
OUTLINE = 16384


def staged_world(n, seed, spread, atomic):
    """query_world on the oracle with the batches of first_hit_rule.staged_batches: yields (stage, w, ids, segments, spheres, shell spheres)"""
    ents = query_world(n, seed, spread, atomic)
    w = ro.World(OUTLINE, atomic)
    assert w.register(to_oracle(ents)) == 0
    ids = [int(i) for i in ents["id"]]
    for stage, segments, spheres, shell in staged_batches(w, ids, seed, spread, atomic, lambda cam: w.tick(oracle_camera(cam), 0.05)):
        yield stage, w, ids, segments, spheres, shell
    w.close()


def check_key_order(recs, n, brute):
    """every record's value is a non-negative number; the packed key sorts as (query, value, id) does; the argmin by key is the host rule's pick"""
    q, e, v, _ = as_arrays(recs)
    val = v.view(F32)
    assert not (v >> 31).any() and not np.isnan(val).any()
    assert e.max() < NO_ENTITY
    key = pack_keys(v, e)
    assert (key != KEY_NONE).all()
    by_key = np.lexsort((key, q))
    by_value = np.lexsort((e, val, q))
    np.testing.assert_array_equal(by_key, by_value)
    assert winners_by_key(recs, n) == brute(recs, n)


@pytest.mark.parametrize("n,seed,spread,atomic", WORLDS)
def test_key_order_draws_and_the_second_pass(n, seed, spread, atomic):
    """tests 1, 2 and 4 of the rule over one set of worlds and batches:
    the key order on every record; the classes of winners the draws hold (printed; each asserted to be there, no fraction); and for every query with a
    winner, that the winner and every entity tied with it in value has a key inside the query's cell range whose cell box passes the SHRUNK prune of the
    second pass (0 exceptions)."""
    cls = dict(seg_hit=0, seg_none=0, seg_tied=0, seg_tied_across=0, seg_positive=0, sph_hit=0, sph_none=0, sph_tied=0, sph_tied_across=0, sph_at_zero=0,
               shell_hit=0, shell_none=0, shell_positive=0, records=0, reached=0, reached_tied=0, reached_shared=0)
    for stage, w, ids, (p0, p1), (c, r), (sc, sr) in staged_world(n, seed, spread, atomic):
        lookups = {}

        def lookup(e):
            if e not in lookups:
                lookups[e] = w.lookup(e)
            return lookups[e]

        def classify(recs, nq, name, ranges, passes):
            cls["records"] += len(recs)
            winners = winners_by_key(recs, nq)
            by_query = {}
            for rec in recs:
                by_query.setdefault(rec[0], []).append(rec)
            for i, win in enumerate(winners):
                if win is None:
                    cls[name + "_none"] += 1
                    continue
                cls[name + "_hit"] += 1
                tied = [rec for rec in by_query[i] if rec[2] == win[2]]
                assert win in tied and win[1] == min(rec[1] for rec in tied)
                if name != "shell":
                    cls[name + "_tied"] += len(tied) > 1
                    cls[name + "_tied_across"] += len({lookup(rec[1])[0] for rec in tied}) > 1
                if win[2] != 0:
                    cls[name + "_positive"] = cls.get(name + "_positive", 0) + 1
                elif name == "sph":
                    cls["sph_at_zero"] += 1
                # the second pass: the winner and everything tied with it
                for rec in tied:
                    assert pick_reaches(lookup(rec[1]), ranges[i], lambda cells: passes(i, cells, win[2])), (stage, name, i, rec, win)
                    cls["reached"] += 1; cls["reached_tied"] += rec != win; cls["reached_shared"] += lookup(rec[1])[0] == 2

        # segments
        recs = seg.segment_hits(w, ids, p0, p1)
        check_key_order(recs, len(p0), seg.first_hits_brute)
        d = [seg.direction(p0[i], p1[i]) for i in range(len(p0))]
        ranges = [query_cell_ranges(seg.bounding_box(p0[i], p1[i], OUTLINE), OUTLINE, atomic) for i in range(len(p0))]
        classify(recs, len(p0), "seg", ranges, lambda i, cells, best: shrunk_prune_passes_segment(p0[i], d[i], cells, best, OUTLINE, atomic))
        # the siblings' spheres, then the shell
        for name, cc, rr in (("sph", c, r), ("shell", sc, sr)):
            recs = sph.sphere_hits(w, ids, cc, rr)
            check_key_order(recs, len(cc), sph.nearest_brute)
            assert all(sph.sphere_cell_count(cc[i], rr[i], OUTLINE, atomic) <= MAX_CELLS for i in range(len(cc)))
            ranges = [query_cell_ranges(sph.bounding_box(cc[i], rr[i], OUTLINE), OUTLINE, atomic) for i in range(len(cc))]
            classify(recs, len(cc), name, ranges, lambda i, cells, best, cc=cc: shrunk_prune_passes_sphere(cc[i], cells, best, OUTLINE, atomic))
    print(cls)
    assert cls["shell_positive"] == cls["shell_hit"]                    # no shell centre lies inside an entity
    for k, v in cls.items():
        assert v > 0, (k, cls)


def test_key_of_special_values():
    """+0.0 is the smallest key value, ties fall to the id, and the sentinel is above every key an entity can have"""
    v = np.array([0.0, 1e-45, 0.25, 1.0, 3e38, np.inf], F32).view(np.uint32)
    keys = pack_keys(v, np.full(len(v), 0xFFFFFFFE, np.uint32))
    assert (np.diff(keys.astype(object)) > 0).all() and keys.max() < KEY_NONE
    assert pack_keys([v[2]], [7])[0] < pack_keys([v[2]], [8])[0] < pack_keys([v[3]], [0])[0]
    recs = [(0, 9, int(v[2]), 1), (0, 4, int(v[2]), 2), (0, 2, int(v[3]), 3), (2, 5, 0, 0)]
    assert winners_by_key(recs, 3) == [(0, 4, int(v[2]), 2), None, (2, 5, 0, 0)] == seg.first_hits_brute(sorted(recs), 3)
    rec, found = reduced_records(winners_by_key(recs, 3), seg.SEGMENT_HIT_DT)
    assert found.tolist() == [True, False, True] and rec["query"].tolist() == [0, 1, 2] and rec["entity_id"].tolist() == [4, 0, 5]
    assert rec[1].tobytes() == np.array([1, 0, 0, 0], np.uint32).tobytes()


@pytest.mark.parametrize("atomic", [64, 16])
def test_hand_worked_known_answers(atomic):
    import render_engine_amd as R
    w = ro.World(OUTLINE, atomic)
    assert w.register(to_oracle(known_world(atomic))) == 0
    w.apply_changes(probe_push_out().view(ro.CHANGE_DT))
    w.apply_changes(push_further().view(ro.CHANGE_DT))
    last = OUTLINE // atomic
    assert w.lookup(3) == (1, [ro.pack_key(0, last, 0, 0)])                                      # kept in the cell one past the grid, clipped
    assert w.lookup(6)[0] == 2 and len(w.lookup(6)[1]) == 8 and w.lookup(2)[0] == 2 and w.lookup(5)[0] == 1 and w.lookup(8)[0] == 1 and w.lookup(0)[0] == 1
    names = set()
    for name, kind, query, exclude, need, forbid, want in known_cases(atomic, OUTLINE, R.F_STATIC):
        names.add(name)
        ex = np.array([exclude], np.uint32)
        if kind == "sphere":
            c, r = query
            rec, found = spheres_nearest(w, range(9), c[None, :], np.array([r], F32), exclude=ex, need=need, forbid=forbid)
            all_recs = sph.sphere_hits(w, range(9), c[None, :], np.array([r], F32), exclude=ex, need=need, forbid=forbid)
        else:
            p0, p1 = query
            rec, found = segments_first(w, range(9), p0[None, :], p1[None, :], exclude=ex, need=need, forbid=forbid)
            all_recs = seg.segment_hits(w, range(9), p0[None, :], p1[None, :], exclude=ex, need=need, forbid=forbid)
        got = tuple(int(x) for x in rec.view(np.uint32).reshape(-1, 4)[0][1:]) if found[0] else None
        assert got == want, (name, kind, got, want, all_recs)
        tied = [h for h in all_recs if want is not None and h[2] == want[1]]
        if name.startswith("tie"):
            assert len(tied) >= 2 and want[1] != 0 and want[0] == min(h[1] for h in tied), (name, tied)
        if "shared section" in name:
            assert w.lookup(want[0])[0] == 2 and len(w.lookup(want[0])[1]) == 8 and {w.lookup(h[1])[0] for h in tied} == {1, 2}
        if "unique section" in name:
            assert w.lookup(want[0])[0] == 1 and {w.lookup(h[1])[0] for h in tied} == {1, 2}
        if name == "out of bounds":                                                                # only the boundary extension of the prune reaches it
            if kind == "sphere":
                assert sph.prune_passes(query[0], query[1], [(0, last, 0, 0)], OUTLINE, atomic) and not sph.prune_passes(query[0], query[1], [(0, last, 0, 0)], OUTLINE, atomic, extend=False)
                assert shrunk_prune_passes_sphere(query[0], [(0, last, 0, 0)], want[1], OUTLINE, atomic)
            else:
                d = seg.direction(*query)
                assert seg.prune_passes(query[0], d, [(0, last, 0, 0)], OUTLINE, atomic) and not seg.prune_passes(query[0], d, [(0, last, 0, 0)], OUTLINE, atomic, extend=False)
                assert shrunk_prune_passes_segment(query[0], d, [(0, last, 0, 0)], want[1], OUTLINE, atomic)
    assert len(names) >= 12
    w.close()


# ---- ABI and mirrors --------------------------------------------------------------------------------------------------------------------------------

def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_are_exported_and_declared():
    from render_engine_amd import _capi
    L = _capi.load()
    header = re.sub(r"/\*.*?\*/", "", read("include", "re_hip.h"), flags=re.S)
    for name, batch, q, hit, out in (("re_query_segments_first", "re_segment", "segments", "re_segment_hit", "first"),
                                     ("re_query_spheres_nearest", "re_sphere", "spheres", "re_sphere_hit", "nearest")):
        assert hasattr(L, name) and name in _capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(\s*re_ctx\s*\*ctx,\s*const\s+%s\s*\*%s,\s*uint32_t\s+n,\s*const\s+re_box_query_args\s*\*args,\s*%s\s*\*%s\s*,\s*uint32_t\s*\*n_found\s*\)\s*;"
                         % (name, batch, q, hit, out), header), name
        fn = getattr(L, name)
        assert fn.restype == C.c_int and len(fn.argtypes) == 6 and fn.argtypes[2] == C.c_uint32 and fn.argtypes[5] == C.POINTER(C.c_uint32)
    assert L.re_abi_version() == 3                                   # additions only
    tq = read("render_engine_amd", "csrc", "re_treequery.hip")
    for k in ("k_segment_first_reduce", "k_segment_first_pick", "k_sphere_nearest_reduce", "k_sphere_nearest_pick"):
        assert k in tq and k in read("render_engine_amd", "csrc", "re_kernels.h") and k in read("render_engine_amd", "csrc", "re_api.hip")


def test_rust_binding_cpp_mirror_and_python_carry_them():
    ffi = read("integration", "rust", "src", "gpu_visible_set", "ffi.rs")
    assert "pub fn re_query_segments_first(" in ffi and "pub fn re_query_spheres_nearest(" in ffi
    mod = read("integration", "rust", "src", "gpu_visible_set", "mod.rs")
    assert "pub fn first_along_segments" in mod and "ffi::re_query_segments_first" in mod and "pub fn nearest_within_radius" in mod and "ffi::re_query_spheres_nearest" in mod
    hpp = read("include", "render_engine_hip.hpp")
    assert "find_first_along_segments(" in hpp and "re_query_segments_first(" in hpp and "find_nearest_within_radius(" in hpp and "re_query_spheres_nearest(" in hpp
    assert ffi.rstrip() in read("INTEGRATION.md")                    # the block of INTEGRATION.md is the file, verbatim
    import inspect
    import render_engine_amd as R
    for fn in (R.Pipeline.find_first_along_segments, R.Pipeline.find_nearest_within_radius):
        assert callable(fn)
        names = list(inspect.signature(fn).parameters)
        assert names[2:] == ["exclude", "need", "forbid"], names
