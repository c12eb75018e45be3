"""The rule of re_query_segments_first and re_query_spheres_nearest restated on the CPU, plain numpy over the rules of their siblings (tests/segment_rule.py,
tests/sphere_rule.py; no GPU, no product code): record i is the record of query i that the sibling reports with the smallest (t_enter, entity_id) /
(dist_sq, entity_id), or the no-hit record.

The device finds it by a 64-bit key, bits(value) << 32 | entity_id, reduced with an unsigned minimum.  That is the lexicographic (value, id) order because
both values are non-negative and never NaN: the slab test's lo starts at +0.0 and is replaced only by something greater, dist_sq is a sum of squares of 0.0
or positive differences, and the bit patterns of non-negative floats order as the floats do.  All ones is "no hit": 0xFFFFFFFF is no entity's id.

The second pass walks again with every query shrunk to its best value: a sphere with r2 := best dist_sq, a segment whose cell prune also misses a cell whose
slab lo exceeds the best t_enter.  shrunk_prune_passes_* are those prunes; tests/test_first_hit_rule.py shows that the winner and everything tied with it
stay inside them."""
import numpy as np

import segment_rule as seg
import sphere_rule as sph
from box_query_rule import MAX_CELLS, tree_entities, key_in_ranges

F32 = np.float32
NO_ENTITY = 0xFFFFFFFF
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def pack_keys(value_bits, ids):
    """bits(value) << 32 | entity id, as u64"""
    return (np.asarray(value_bits, np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


def as_arrays(recs):
    """(query, id, value bits, second word) u32 arrays of records as segment_hits / sphere_hits return them"""
    a = np.array(recs, np.uint64).reshape(-1, 4)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32), a[:, 3].astype(np.uint32)


def winners_by_key(recs, n):
    """per query the record with the smallest key, or None: the device's reduction, on the records of the sibling's rule"""
    out = [None] * n
    if not len(recs):
        return out
    q, e, v, x = as_arrays(recs)
    key = pack_keys(v, e)
    best = np.full(n, KEY_NONE, np.uint64)
    np.minimum.at(best, q, key)
    for i in np.nonzero(key == best[q])[0]:
        assert out[int(q[i])] is None                               # entity ids are unique: one record per query carries the minimum
        out[int(q[i])] = (int(q[i]), int(e[i]), int(v[i]), int(x[i]))
    return out


def reduced_records(winners, dtype):
    """(records, found) in the format of render_engine_amd.first_hits / nearest_hits: winners as first_hits_brute / nearest_brute / winners_by_key give them;
    a query without a hit is zero but for its query index"""
    n = len(winners)
    rec = np.zeros(n, dtype)
    rec["query"] = np.arange(n, dtype=np.uint32)
    found = np.zeros(n, bool)
    words = rec.view(np.uint32).reshape(n, 4)
    for i, w in enumerate(winners):
        if w is not None:
            assert w[0] == i
            words[i] = w
            found[i] = True
    return rec, found


def segments_first(w, ids, p0, p1, exclude=None, need=0, forbid=0):
    """(first, found): the rule of re_query_segments_first in the format of first_hits"""
    recs = seg.segment_hits(w, ids, p0, p1, exclude=exclude, need=need, forbid=forbid)
    return reduced_records(seg.first_hits_brute(recs, len(np.asarray(p0).reshape(-1, 3))), seg.SEGMENT_HIT_DT)


def spheres_nearest(w, ids, c, r, exclude=None, need=0, forbid=0):
    """(nearest, found): the rule of re_query_spheres_nearest in the format of nearest_hits"""
    recs = sph.sphere_hits(w, ids, c, r, exclude=exclude, need=need, forbid=forbid)
    return reduced_records(sph.nearest_brute(recs, len(np.asarray(c).reshape(-1, 3))), sph.SPHERE_HIT_DT)


# ---- the prunes of the second pass ----------------------------------------------------------------------------------------------------------------

def shrunk_prune_passes_segment(p0, d, cells, best_bits, outline, atomic):
    """the segment meets the cell box (inflated, boundary-extended) and enters it no later than the best t_enter"""
    hit, lo, _ = seg.slab(p0, d, seg.cell_box(cells, outline, atomic))
    return bool(hit[0]) and bool(lo[0] <= np.array([best_bits], np.uint32).view(F32)[0])


def shrunk_prune_passes_sphere(c, cells, best_bits, outline, atomic):
    """the cell box lies no further from the centre than the best dist_sq (the sibling's prune with r2 := best)"""
    return bool(sph.dist_sq(c, seg.cell_box(cells, outline, atomic))[0][0] <= np.array([best_bits], np.uint32).view(F32)[0])


def pick_reaches(lookup, ranges, passes):
    """does the second pass reach an entity: a key inside the query's cell range of its level whose cell box passes the shrunk prune `passes(cells)`;
    for a shared section any linked key in the range, then the bounding cell box of its keys"""
    kind, keys = lookup
    if kind == 2:
        return any(key_in_ranges(key, ranges) for key in keys) and passes(seg.key_cells(keys))
    return any(key_in_ranges(key, ranges) and passes(seg.key_cells([key])) for key in keys)


# ---- the shell draw: winners at a positive distance ---------------------------------------------------------------------------------------------------

def draw_shell_spheres(w, ids, rng, outline, atomic, n=64):
    """(c [n, 3], r [n]): centres uniform inside the bounding box of the tree's entities, then moved 5 to 60 units beyond one of its faces; radius 30 to 200,
    capped at 14 atomic lengths (which passes the cap on candidate cells).  No centre lies inside an entity: every hit has dist_sq > 0."""
    _, ab, _ = tree_entities(w, ids)
    lo, hi = ab[:, 0::2].min(axis=0), ab[:, 1::2].max(axis=0)
    cs, rs = np.zeros((n, 3), F32), np.zeros(n, F32)
    for j in range(n):
        c = rng.uniform(lo, hi).astype(F32)
        a, up = int(rng.integers(3)), int(rng.integers(2))
        off = F32(rng.uniform(5, 60))
        c[a] = hi[a] + off if up else lo[a] - off
        r = min(F32(rng.uniform(30, 200)), F32(14 * atomic))
        assert sph.sphere_cell_count(c, r, outline, atomic) <= MAX_CELLS
        cs[j], rs[j] = c, r
    return cs, rs


def staged_batches(w, ids, seed, spread, atomic, tick, outline=16384):
    """the batches of the tests at three stages of one world, 0, 3 and 6 ticks old: yields (stage, (p0, p1), (c, r), (shell c, shell r)).  The segments and the
    spheres are the siblings' draws (draw_segments / draw_spheres from a generator seeded as in their tests; the cameras of the ticks come from the
    spheres' generator, as in test_sphere_rule.py); the shell spheres have a generator of their own.  tick(camera) advances the world(s) by one tick."""
    import render_engine_amd as R
    from test_logic_rule import camera_draw
    rng_seg, rng_sph, rng_shell = np.random.default_rng(seed), np.random.default_rng(seed), np.random.default_rng(seed + 1000)
    for stage in range(3):
        yield stage, seg.draw_segments(w, ids, rng_seg, outline, atomic), sph.draw_spheres(w, ids, rng_sph, outline, atomic), draw_shell_spheres(w, ids, rng_shell, outline, atomic)
        if stage < 2:
            for _ in range(3):
                tick(camera_draw(R, rng_sph, spread))


# ---- hand-worked known answers on known_world (tests/test_segment_rule.py) ------------------------------------------------------------------------------

def push_further():
    """a second change request for entity 3 of probe_world, behind probe_push_out: its position set to 300, x in [outline + 216, outline + 226] -- more than a
    section length beyond the cell it is kept in (one past the grid, clipped), so a query out there meets that cell's box only as extended"""
    import render_engine_amd as R
    ch = np.zeros(1, R.CHANGE_DT)
    ch[0] = (R._capi.CHANGE_MODIFY, 3, R._capi.C_POSITION, 0, (300.0, 0.0, 0.0, 0.0))
    return ch


def bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def known_cases(atomic=64, outline=16384, F_STATIC=1):
    """[(name, kind, query, exclude, need, forbid, expected)] on known_world after probe_push_out and push_further.  kind "sphere": query = (c [3], r);
    kind "segment": query = (p0 [3], p1 [3]).  expected = (entity, value bits, second word) or None.  Coordinates in units of s = atomic / 64, a power of two:
    every sum of squares below is exact in f32, every t a correctly rounded quotient of exact values.
    The boxes (units of s): 0: x [10, 64]  1: x [64, 100]  2: x [63.5, 64.5] (a shared section of 2 links), y and z of the three [10, 20];  4: [0, 64]^3
    5: [100, 128]^3   6: [639, 641]^3 (a shared section of 8 links)   7: [300, 310]^3, static   8: [400, 410]^3   3: out of bounds (x and its query unscaled)."""
    s = F32(atomic) / F32(64.0)
    far = F32(outline)
    at = lambda *p: np.asarray(p, F32) * s
    d2 = lambda v: bits(F32(v) * s * s)
    t = lambda a, b: bits(F32(a) / F32(b))
    low, high = 1 | 2 | 4, 16 | 32 | 64                                 # side: the centre below the minimum corner, above the maximum corner
    mid78, mid86, mid56 = at(355, 355, 355), at(524.5, 524.5, 524.5), at(383.5, 383.5, 383.5)
    down = (at(64, 84, 15), at(64, 4, 15))                              # along -y in the plane x = 64, where 0, 1, 2 and 4 meet
    out = [
        # 45 from the maximum corner of 7 and from the minimum corner of 8 on every axis: 3 * 45^2 = 6075 twice, the lower id wins
        ("tie at a positive distance", "sphere", (mid78, F32(80.0) * s), NO_ENTITY, 0, 0, (7, d2(6075.0), high)),
        # ... with 7 filtered out the other one of the tie
        ("the winner filtered out", "sphere", (mid78, F32(80.0) * s), NO_ENTITY, 0, F_STATIC, (8, d2(6075.0), low)),
        # 114.5 from 8 and from 6 on every axis: 3 * 114.5^2 = 39330.75; the lower id, 6, sits in the shared section of 8 links, 8 in a unique one
        ("tie, the lower id in the shared section", "sphere", (mid86, F32(200.0) * s), NO_ENTITY, 0, 0, (6, d2(39330.75), low)),
        # 16.5 below 8: 816.75; with 8 excluded 7, 73.5 away: 16206.75; with 7 filtered out too 5 and 6, both 255.5 away: 195840.75 -- the lower id, 5, in a
        # unique section, 6 in the shared one
        ("the nearest of four", "sphere", (mid56, F32(450.0) * s), NO_ENTITY, 0, 0, (8, d2(816.75), low)),
        ("the winner excluded", "sphere", (mid56, F32(450.0) * s), 8, 0, 0, (7, d2(16206.75), high)),
        ("tie, the lower id in the unique section", "sphere", (mid56, F32(450.0) * s), 8, 0, F_STATIC, (5, d2(195840.75), high)),
        ("no hit", "sphere", (at(420, 405, 405), F32(0.0)), NO_ENTITY, 0, 0, None),
        # the out-of-bounds entity, 14 beyond its maximum face; its cell ends at outline + atomic: reached through the boundary extension alone
        ("out of bounds", "sphere", (np.array([far + F32(240.0), F32(15.0) * s, F32(15.0) * s], F32), F32(14.0)), NO_ENTITY, 0, 0, (3, bits(196.0), 16)),
        # from y = 84 down to y = 4: 4 ([0, 64]^3) is entered at 20 / 80; with 4 excluded 0, 1 and 2 (y up to 20) all at 64 / 80 -- x = 64 is the maximum of
        # 0, the minimum of 1 and inside 2 --, left at 74 / 80: the lowest id wins, 0 and 1 in unique sections, 2 in a shared one
        ("the first of four", "segment", down, NO_ENTITY, 0, 0, (4, t(20, 80), bits(1.0))),
        ("tie at a positive t, the winner excluded", "segment", down, 4, 0, 0, (0, t(64, 80), t(74, 80))),
        # through the corner (300, 300, 300) of the static 7 at 2 / 4; filtered out: nothing
        ("through a corner", "segment", (at(298, 298, 298), at(302, 302, 302)), NO_ENTITY, 0, 0, (7, t(2, 4), bits(1.0))),
        ("the winner filtered out, no hit", "segment", (at(298, 298, 298), at(302, 302, 302)), NO_ENTITY, 0, F_STATIC, None),
        ("no hit", "segment", (at(420, 405, 405), at(420, 405, 405)), NO_ENTITY, 0, 0, None),
        # the out-of-bounds entity ([outline + 216, outline + 226]) from outline + 250 down to outline + 210: in at 24 / 40, out at 34 / 40
        ("out of bounds", "segment", (np.array([far + F32(250.0), F32(15.0) * s, F32(15.0) * s], F32), np.array([far + F32(210.0), F32(15.0) * s, F32(15.0) * s], F32)),
         NO_ENTITY, 0, 0, (3, t(24, 40), t(34, 40))),
    ]
    return out
