"""The rule of re_query_spheres and the pruning of its walk (tests/sphere_rule.py) against the oracle's own section decisions: hand-worked known answers
with their exact dist_sq and side, the property the walk rests on -- every pair of the rule has a section key inside the inflated bounding cube's cell
range of its level whose inflated, boundary-extended cell box lies within the radius --, and nearest_hits against a brute-force argmin."""
import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from box_query_rule import MAX_CELLS, query_cell_ranges, key_in_ranges, probe_push_out, query_world, N_CROWD, overflow_world, assert_overflow_placement
from sphere_rule import (F32, NO_ENTITY, SPHERE_HIT_DT, dist_sq, sphere_hits, nearest_brute, bounding_box, sphere_cell_count, key_cells, prune_passes,
                         pruned_fraction, draw_spheres, margin)
from test_segment_rule import known_world, bits
from test_logic_rule import camera_draw

WORLDS = [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)]      # n, seed, spread, atomic: the worlds of test_box_query_rule.py


def known_spheres(atomic=64, outline=16384):
    """(c [n, 3], r [n], exclude [n], expected [(query, entity, bits of dist_sq, side)]) on known_world after probe_push_out: coordinates in units of
    s = atomic / 64 (a power of two: every product below is exact in f32), so both encodings see the same cases"""
    s = F32(atomic) / F32(64.0)
    far = F32(outline)
    Cs, Rs, EX, want = [], [], [], []

    def sph(c, r, hits, exclude=NO_ENTITY):
        i = len(Cs)
        Cs.append(np.asarray(c, F32)); Rs.append(F32(r)); EX.append(exclude)
        want.extend((i, e, bits(F32(d) * s * s), side) for e, d, side in hits)

    at = lambda *p: np.asarray(p, F32) * s
    # 0: touching the minimum x face of 7 ([300, 310]^3) from 10 away; 1: one float less of a radius: nothing
    sph(at(290, 305, 305), F32(10.0) * s, [(7, 100.0, 1)])
    sph(at(290, 305, 305), np.nextafter(F32(10.0) * s, F32(0.0)), [])
    # 2: a 3-4-5 touch over the edge x = 300, y = 300; 3: over the corner (300, 300, 300): 1 + 4 + 4 = 9
    sph(at(297, 296, 305), F32(5.0) * s, [(7, 25.0, 3)])
    sph(at(299, 298, 298), F32(3.0) * s, [(7, 9.0, 7)])
    # 4, 5: a point query inside 8 ([400, 410]^3) and one outside everything
    sph(at(405, 405, 405), 0.0, [(8, 0.0, 0)])
    sph(at(420, 405, 405), 0.0, [])
    # 6: a point in the shared section of 8 links (6: [639, 641]^3): once
    sph(at(640, 640, 640), 0.0, [(6, 0.0, 0)])
    # 7, 8: inside 0 (x in [10, 64]) and 4 ([0, 64]^3), 32 below 1 (x from 64) and 31.5 below 2 (x from 63.5); then with 2 excluded
    near = [(0, 0.0, 0), (1, 1024.0, 1), (2, 992.25, 1), (4, 0.0, 0)]
    sph(at(32, 15, 15), F32(40.0) * s, near)
    sph(at(32, 15, 15), F32(40.0) * s, [h for h in near if h[0] != 2], exclude=2)
    # 9: the out-of-bounds entity 3 ([outline + 6, outline + 16] in x, pushed out by probe_push_out; y, z in [10, 20] * s), one cell past the grid, from 14
    #    beyond its maximum face; x and the radius are not scaled
    i = len(Cs)
    Cs.append(np.array([far + F32(30.0), F32(15.0) * s, F32(15.0) * s], F32)); Rs.append(F32(14.0)); EX.append(NO_ENTITY)
    want.append((i, 3, bits(196.0), 16))
    return np.array(Cs, F32), np.array(Rs, F32), np.array(EX, np.uint32), sorted(want)


def walk_reaches(w, e, c, r, outline, atomic, lookup=None, ranges=None, **k):
    kind, keys = lookup if lookup is not None else w.lookup(e)
    if ranges is None:
        ranges = query_cell_ranges(bounding_box(c, r, outline), outline, atomic)
    if kind == 2:      # a shared section: any linked key in the range of its level, then the bounding cell box of its keys
        return any(key_in_ranges(key, ranges) for key in keys) and prune_passes(c, r, key_cells(keys), outline, atomic, **k)
    return any(key_in_ranges(key, ranges) and prune_passes(c, r, key_cells([key]), outline, atomic, **k) for key in keys)


@pytest.mark.parametrize("atomic", [64, 16])
def test_hand_worked_known_answers(atomic):
    w = ro.World(16384, atomic)
    assert w.register(to_oracle(known_world(atomic))) == 0
    w.apply_changes(probe_push_out().view(ro.CHANGE_DT))
    c, r, ex, want = known_spheres(atomic)
    got = sphere_hits(w, range(9), c, r, exclude=ex)
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert len([h for h in want if h[0] == 6]) == 1                                # the shared section of 8 links: once
    assert w.lookup(6)[0] == 2 and len(w.lookup(6)[1]) == 8
    # the filter follows the boxes': the out-of-bounds entity alone, and everything but it
    assert [h[:2] for h in sphere_hits(w, range(9), c, r, exclude=ex, need=ro.F_OOB_LOGIC)] == [(9, 3)]
    assert (9, 3) not in [h[:2] for h in sphere_hits(w, range(9), c, r, exclude=ex, forbid=ro.F_OOB_LOGIC)]
    # ... and the walk reaches every one of them: a key in the range of its level whose cell box passes the prune
    for i, e, _, _ in want:
        assert walk_reaches(w, e, c[i], r[i], 16384, atomic), (i, e)
    # entity 3 sits one cell past the grid, clipped to the outline.  Sphere 9 (x = outline + 30, r = 14) is still within 14 of that cell's own inflated box
    # [outline - 4, outline + atomic + 4] at both atomic lengths, so it does not need the extension; a sphere around an entity pushed out further than the
    # cell reaches (by more than a section length and the radius) lies beyond the cell's own box and meets it only as extended -- with extend=False it is lost
    last = 16384 // atomic
    assert w.lookup(3) == (1, [ro.pack_key(0, last, 0, 0)])
    a = np.array([16384 + 300, 5, 5], F32)
    assert prune_passes(a, 14.0, [(0, last, 0, 0)], 16384, atomic) and not prune_passes(a, 14.0, [(0, last, 0, 0)], 16384, atomic, extend=False)
    assert not prune_passes(a, 14.0, [(0, last - 2, 0, 0)], 16384, atomic)          # (cell last - 1 ends on the face of the world: extended too)
    w.close()


@pytest.mark.parametrize("n,seed,spread,atomic", WORLDS)
def test_every_hit_is_reached_by_the_walk(n, seed, spread, atomic):
    """the superset property, after 0, 3 and 6 ticks of the oracle, over 64 drawn spheres each; and that the draw is not hollow"""
    import render_engine_amd as R
    outline = 16384
    ents = query_world(n, seed, spread, atomic)
    w = ro.World(outline, atomic)
    assert w.register(to_oracle(ents)) == 0
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(seed)
    pairs = through_shared = touch = inside = special = cells = kept = 0
    for stage in range(3):
        c, r = draw_spheres(w, ids, rng, outline, atomic)
        ranges, plain = [], []
        for j in range(len(c)):
            assert sphere_cell_count(c[j], r[j], outline, atomic) <= MAX_CELLS
            tot, k = pruned_fraction(c[j], r[j], outline, atomic)
            cells += tot; kept += k
            ranges.append(query_cell_ranges(bounding_box(c[j], r[j], outline), outline, atomic))
            # the plain range of the raw bounding cube: no minus-one step (the inflation subsumes it), no inflation
            plain.append(query_cell_ranges(bounding_box(c[j], r[j], outline, inflate=False), outline, atomic, minus_one=False))
        lookups = {}
        for i, e, d2, side in sphere_hits(w, ids, c, r):
            if e not in lookups:
                lookups[e] = w.lookup(e)
            kind, keys = lookups[e]
            assert walk_reaches(w, e, c[i], r[i], outline, atomic, lookup=lookups[e], ranges=ranges[i]), \
                (stage, i, e, c[i], r[i], w.entity(e)["aabb"], [ro.unpack_key(k) for k in keys])
            pairs += 1; through_shared += kind == 2
            touch += r[i] > 0 and d2 == bits(F32(r[i]) * F32(r[i]))
            inside += side == 0
            if side == 0:                                                              # the centre is inside the box
                assert d2 == 0
            # what only the minus-one step of the cell range or the boundary extension of the prune reaches
            special += not any(key_in_ranges(key, plain[i]) for key in keys) or not walk_reaches(w, e, c[i], r[i], outline, atomic, lookup=lookups[e], ranges=ranges[i], extend=False)
        for _ in range(3):
            w.tick(oracle_camera(camera_draw(R, rng, spread)), 0.05)
    print(dict(pairs=pairs, through_shared=through_shared, touch=touch, inside=inside, special=special, cells=cells, kept=kept))
    assert pairs >= 5000 and through_shared >= 1000 and touch >= 20 and inside >= 100 and special >= 5, (pairs, through_shared, touch, inside, special)
    assert kept < cells, (kept, cells)
    w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_the_margin_the_cap_and_the_limits(atomic):
    """outline * 2^-12; a radius of 14 atomic lengths passes the cap and one of 15 does not, at both atomic lengths; the magnitude limit of the call,
    64 outline lengths, keeps one ulp of c +- r (outline * 2^-16 at outline * 2^7) below the margin"""
    assert margin(16384) == F32(4.0)
    a = np.array([8000, 8000, 8000], F32)
    assert sphere_cell_count(a, F32(14 * atomic), 16384, atomic) <= MAX_CELLS < sphere_cell_count(a, F32(15 * atomic), 16384, atomic)
    big = F32(64.0) * F32(16384.0)
    assert np.spacing(big + big) <= F32(16384.0) / F32(65536.0) < margin(16384)
    # an overflowing product gives inf, which misses (r2 is finite: the radius is at most 64 outline lengths); infinite bounds give e = 0
    d2, side = dist_sq(np.array([3e38, 0, 0], F32), np.array([[-3e38, -2e38, -1, 1, -1, 1], [-np.inf, np.inf, -1, 1, -np.inf, np.inf]], F32))
    assert np.isinf(d2[0]) and not d2[0] <= big * big and np.isfinite(big * big) and side[0] == 16 and d2[1] == 0 and side[1] == 0


@pytest.mark.parametrize("atomic", [64, 16])
def test_overflow_world_exceeds_the_staging_buffer(atomic):
    """the precondition of the GPU test of the overflow paths (test_sphere_query_gpu.py): the placement of overflow_world, and both spheres return more
    records than a workgroup stages"""
    ents = overflow_world(atomic)
    w = ro.World(16384, atomic)
    assert w.register(to_oracle(ents)) == 0
    assert_overflow_placement(w)
    c, r = overflow_spheres(atomic)
    got = sphere_hits(w, [int(i) for i in ents["id"]], c, r)
    per_query = [sum(1 for rec in got if rec[0] == q) for q in range(2)]
    assert per_query == [N_CROWD + 1, N_CROWD] == [1101, 1100]
    assert min(per_query) > 1024                                                 # BOXQ_HITBUF (re_kernels.h)
    assert sorted(rec[1] for rec in got if rec[0] == 0) == [5] + list(range(100, 100 + N_CROWD)) and sorted(rec[1] for rec in got if rec[0] == 1) == list(range(5000, 5000 + N_CROWD))
    w.close()


def overflow_spheres(atomic=64):
    """(c [2, 3], r [2]): sphere 0 over the first crowd of overflow_world (and entity 5: N_CROWD + 1 hits), sphere 1 over the second (N_CROWD hits)"""
    s = F32(atomic) / F32(64.0)
    return np.array([[114, 114, 114], [640, 640, 640]], F32) * s, np.array([20, 10], F32) * s


def test_nearest_hits_against_brute_force():
    """render_engine_amd.nearest_hits: per query the record with the smallest (dist_sq, entity_id), ties by entity id, none for a query without hits"""
    import render_engine_amd as R
    rng = np.random.default_rng(11)
    n = 40
    hits = np.zeros(600, SPHERE_HIT_DT)
    hits["query"] = rng.integers(0, n - 3, len(hits))                              # (the last three queries hit nothing)
    hits["entity_id"] = rng.permutation(len(hits)).astype(np.uint32)
    hits["dist_sq"] = rng.integers(0, 6, len(hits)).astype(F32) * F32(0.25)        # few values: ties abound
    hits["side"] = rng.integers(0, 128, len(hits))
    recs = sorted(zip(hits["query"].tolist(), hits["entity_id"].tolist(), hits["dist_sq"].view(np.uint32).tolist(), hits["side"].tolist()))
    want = nearest_brute(recs, n)
    nearest, found = R.nearest_hits(hits, n)
    assert nearest.dtype == R._capi.SPHERE_HIT_DT == SPHERE_HIT_DT and len(nearest) == n == len(found)
    ties = 0
    for i in range(n):
        assert found[i] == (want[i] is not None)
        assert int(nearest["query"][i]) == i
        if want[i] is not None:
            assert (i, int(nearest["entity_id"][i]), bits(nearest["dist_sq"][i]), int(nearest["side"][i])) == want[i]
            ties += sum(1 for rec in recs if rec[0] == i and rec[2] == want[i][2]) > 1
    assert ties >= 5 and not found[n - 3:].any()
    nearest, found = R.nearest_hits(hits[:0], 4)
    assert len(nearest) == 4 and not found.any()
