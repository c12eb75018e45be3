"""The rule of re_query_segments and the pruning of its walk (tests/segment_rule.py) against the oracle's own section decisions: hand-worked known
answers with their exact t values, the property the walk rests on -- every pair of the rule has a section key inside the bounding box's cell range of
its level whose inflated, boundary-extended cell box the segment meets --, and first_hits against a brute-force argmin."""
import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from box_query_rule import MAX_CELLS, query_cell_ranges, key_in_ranges, probe_world, probe_push_out, query_world, N_CROWD, overflow_world, overflow_queries, assert_overflow_placement
from segment_rule import (F32, NO_ENTITY, SEGMENT_HIT_DT, segment_hits, first_hits_brute, direction, bounding_box, segment_cell_count, key_cells, prune_passes,
                          pruned_fraction, draw_segments, margin)
from test_logic_rule import camera_draw

WORLDS = [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)]      # n, seed, spread, atomic: the worlds of test_box_query_rule.py


def bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def known_world(atomic=64):
    """probe_world (box_query_rule.py; coordinates in units of s = atomic / 64) and three boxes more:
    6: [639, 641]^3     straddles a section corner: a shared section linked from 8 sections
    7: [300, 310]^3     static
    8: [400, 410]^3"""
    import render_engine_amd as R
    s = F32(atomic) / F32(64.0)
    ents = probe_world(atomic)
    extra = np.zeros(3, R.ENTITY_DT)
    extra[:] = ents[0]
    extra["id"] = (6, 7, 8); extra["flags"] = (0, R.F_STATIC, 0)
    extra["original"][0] = np.array([639, 641] * 3, F32) * s
    extra["original"][1] = np.array([300, 310] * 3, F32) * s
    extra["original"][2] = np.array([400, 410] * 3, F32) * s
    return np.concatenate([ents, extra])


def known_segments(atomic=64, outline=16384):
    """(p0 [n, 3], p1 [n, 3], exclude [n], expected [(query, entity, t_enter, t_exit)]) on known_world after probe_push_out: every t is a ratio of small
    integers times s that f32 division gives exactly, or a power of two; coordinates in units of s = atomic / 64, so both encodings see the same cases"""
    s = F32(atomic) / F32(64.0)
    far = F32(outline)
    one_up = lambda x: np.nextafter(F32(x), F32(np.inf))
    P0, P1, EX, want = [], [], [], []

    def seg(p0, p1, hits, exclude=NO_ENTITY, scaled=True):
        i = len(P0)
        P0.append(np.asarray(p0, F32) * (s if scaled else F32(1.0))); P1.append(np.asarray(p1, F32) * (s if scaled else F32(1.0))); EX.append(exclude)
        want.extend((i, e, bits(a), bits(b)) for e, a, b in hits)

    # 0: touching a face at one endpoint: from x = 290 to x = 300, the minimum face of 7 ([300, 310]^3)
    seg((290, 305, 305), (300, 305, 305), [(7, 1.0, 1.0)])
    # 1: through a corner of 7: from (298, 298, 298) along the diagonal to (302, 302, 302): enters at the corner (300, 300, 300), t = 2 / 4
    seg((298, 298, 298), (302, 302, 302), [(7, 0.5, 1.0)])
    # 2: only the corner: (296, 304, 300) -> (304, 296, 300), z on the face: x enters at t = 0.5, y leaves at t = 0.5
    seg((296, 304, 300), (304, 296, 300), [(7, 0.5, 0.5)])
    # 3: lying in a face plane: d[y] == 0 with y == the maximum of 7; x from 295 to 315: enters at 5 / 20, leaves at 15 / 20
    seg((295, 310, 305), (315, 310, 305), [(7, 0.25, 0.75)])
    # 4: a single float outside that plane: miss
    P0.append(np.array([295 * s, one_up(310 * s), 305 * s], F32)); P1.append(np.array([315 * s, one_up(310 * s), 305 * s], F32)); EX.append(NO_ENTITY)
    # 5, 6: a point query inside 8 and one outside everything
    seg((405, 405, 405), (405, 405, 405), [(8, 0.0, 1.0)])
    seg((420, 405, 405), (420, 405, 405), [])
    # 7: p0 inside 8, leaving through its x maximum: (405 -> 425): leaves at 5 / 20
    seg((405, 405, 405), (425, 405, 405), [(8, 0.0, 0.25)])
    # 8: from outside the world through the out-of-bounds entity 3 ([outline + 6, outline + 16] in x, pushed out by probe_push_out; y, z in [10, 20] * s),
    #    one cell past the grid: x from outline + 27 down to outline - 5: 32 units, enters at 11 / 32, leaves at 21 / 32
    P0.append(np.array([far + F32(27.0), 15 * s, 15 * s], F32)); P1.append(np.array([far - F32(5.0), 15 * s, 15 * s], F32)); EX.append(NO_ENTITY)
    want.extend([(8, 3, bits(F32(11.0) / F32(32.0)), bits(F32(21.0) / F32(32.0)))])
    # 9: a subnormal d component (y moves by the smallest subnormal: treated as 0, a containment test on y): through 8 along x as segment 7, from outside
    tiny = np.nextafter(F32(0.0), F32(1.0))
    P0.append(np.array([395 * s, 0.0, 405 * s], F32)); P1.append(np.array([415 * s, tiny, 405 * s], F32)); EX.append(NO_ENTITY)      # y = 0: outside [400, 410]: miss
    P0.append(np.array([0.0, 0.0, 32 * s], F32)); P1.append(np.array([tiny, 32 * s, 32 * s], F32)); EX.append(NO_ENTITY)                # 10: x subnormal -> 0 == the minimum face of 4 ([0, 64]^3)
    want.extend([(10, 4, bits(0.0), bits(1.0))])
    # 11, 12: the exclude: along x through 0 ([10, 64]), 2 ([63.5, 64.5]), 1 ([64, 100]) and 4 ([0, 64]^3) at y = z = 15, from x = 0 to x = 128
    along = [(0, 10.0 / 128.0, 0.5), (1, 0.5, 100.0 / 128.0), (2, 63.5 / 128.0, 64.5 / 128.0), (4, 0.0, 0.5)]
    seg((0, 15, 15), (128, 15, 15), along)
    seg((0, 15, 15), (128, 15, 15), [h for h in along if h[0] != 2], exclude=2)
    # 13: through the shared section of 8 links (6: [639, 641]^3) along the diagonal from 638 to 642: 1 / 4 .. 3 / 4 -- reported once
    seg((638, 638, 638), (642, 642, 642), [(6, 0.25, 0.75)])
    return np.array(P0, F32), np.array(P1, F32), np.array(EX, np.uint32), sorted(want)


@pytest.mark.parametrize("atomic", [64, 16])
def test_hand_worked_known_answers(atomic):
    w = ro.World(16384, atomic)
    assert w.register(to_oracle(known_world(atomic))) == 0
    w.apply_changes(probe_push_out().view(ro.CHANGE_DT))
    p0, p1, ex, want = known_segments(atomic)
    got = segment_hits(w, range(9), p0, p1, exclude=ex)
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert direction(p0[9], p1[9])[1] == 0 and p1[9][1] != 0                       # the subnormal component is gone
    # the filter follows the boxes': the out-of-bounds entity alone, and everything but it
    assert [h[:2] for h in segment_hits(w, range(9), p0, p1, exclude=ex, need=ro.F_OOB_LOGIC)] == [(8, 3)]
    assert (8, 3) not in [h[:2] for h in segment_hits(w, range(9), p0, p1, exclude=ex, forbid=ro.F_OOB_LOGIC)]
    # ... and the walk reaches every one of them: a key in the range of its level whose cell box passes the prune; entity 3, one cell past the grid, only
    # through the boundary extension
    for i, e, _, _ in want:
        assert walk_reaches(w, e, p0[i], p1[i], 16384, atomic), (i, e)
    # an entity pushed out further than a section length is still kept in that cell, clipped: a segment out there meets the cell's box only as extended
    last = 16384 // atomic
    assert w.lookup(3) == (1, [ro.pack_key(0, last, 0, 0)])
    a, b = np.array([16384 + 200, 5, 5], F32), np.array([16384 + 300, 5, 5], F32)
    assert prune_passes(a, direction(a, b), [(0, last, 0, 0)], 16384, atomic) and not prune_passes(a, direction(a, b), [(0, last, 0, 0)], 16384, atomic, extend=False)
    assert not prune_passes(a, direction(a, b), [(0, last - 2, 0, 0)], 16384, atomic)       # (cell last - 1 ends on the face of the world: extended too)
    w.close()


def walk_reaches(w, e, p0, p1, outline, atomic, **k):
    kind, keys = w.lookup(e)
    ranges = query_cell_ranges(bounding_box(p0, p1, outline), outline, atomic)
    d = direction(p0, p1)
    if kind == 2:      # a shared section: any linked key in the range of its level, then the bounding cell box of its keys
        return any(key_in_ranges(key, ranges) for key in keys) and prune_passes(p0, d, key_cells(keys), outline, atomic, **k)
    return any(key_in_ranges(key, ranges) and prune_passes(p0, d, key_cells([key]), outline, atomic, **k) for key in keys)


@pytest.mark.parametrize("n,seed,spread,atomic", WORLDS)
def test_every_hit_is_reached_by_the_walk(n, seed, spread, atomic):
    """the superset property, after 0, 3 and 6 ticks of the oracle, over 64 drawn segments each; and that the draw is not hollow"""
    import render_engine_amd as R
    outline = 16384
    ents = query_world(n, seed, spread, atomic)
    w = ro.World(outline, atomic)
    assert w.register(to_oracle(ents)) == 0
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(seed)
    pairs = through_shared = touch = special = cells = kept = 0
    for stage in range(3):
        p0, p1 = draw_segments(w, ids, rng, outline, atomic)
        for j in range(len(p0)):
            assert segment_cell_count(p0[j], p1[j], outline, atomic) <= MAX_CELLS
            c, k = pruned_fraction(p0[j], p1[j], outline, atomic)
            cells += c; kept += k
        for i, e, t0, t1 in segment_hits(w, ids, p0, p1):
            kind, keys = w.lookup(e)
            assert walk_reaches(w, e, p0[i], p1[i], outline, atomic), (stage, i, e, p0[i], p1[i], w.entity(e)["aabb"], [ro.unpack_key(k) for k in keys])
            pairs += 1; through_shared += kind == 2
            d, box = direction(p0[i], p1[i]), w.entity(e)["aabb"]
            touch += t0 == t1 or any(d[a] == 0 and p0[i][a] in (box[2 * a], box[2 * a + 1]) for a in range(3))
            # what only the minus-one step of the cell range or the boundary extension of the prune reaches: the plain range of the raw bounding box
            # (no step; the inflation of the bounding box subsumes the step) or the unextended prune misses it
            plain = query_cell_ranges(bounding_box(p0[i], p1[i], outline, inflate=False), outline, atomic, minus_one=False)
            special += not any(key_in_ranges(key, plain) for key in keys) or not walk_reaches(w, e, p0[i], p1[i], outline, atomic, extend=False)
        for _ in range(3):
            w.tick(oracle_camera(camera_draw(R, rng, spread)), 0.05)
    print(dict(pairs=pairs, through_shared=through_shared, touch=touch, special=special, cells=cells, kept=kept))
    assert pairs >= 500 and through_shared >= 100 and touch >= 10 and special >= 5, (pairs, through_shared, touch, special)
    assert 2 * kept <= cells, (kept, cells)
    w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_overflow_world_exceeds_the_staging_buffer(atomic):
    """the precondition of the GPU test of the overflow paths (test_segment_query_gpu.py): the placement of overflow_world, and both segments return more
    records than a workgroup stages"""
    ents = overflow_world(atomic)
    w = ro.World(16384, atomic)
    assert w.register(to_oracle(ents)) == 0
    assert_overflow_placement(w)
    _, p0, p1 = overflow_queries(atomic)
    got = segment_hits(w, [int(i) for i in ents["id"]], p0, p1)
    per_query = [sum(1 for r in got if r[0] == q) for q in range(2)]
    assert per_query == [N_CROWD + 1, N_CROWD] == [1101, 1100]
    assert min(per_query) > 1024                                                 # BOXQ_HITBUF (re_kernels.h)
    assert sorted(r[1] for r in got if r[0] == 0) == [5] + list(range(100, 100 + N_CROWD)) and sorted(r[1] for r in got if r[0] == 1) == list(range(5000, 5000 + N_CROWD))
    w.close()


def test_the_margin_and_the_cap():
    """outline * 2^-12; a diagonal of 28 atomic lengths per axis passes the cap, one of 34 does not; an axis-aligned segment passes at 100 times that"""
    assert margin(16384) == F32(4.0)
    a = np.array([8000, 8000, 8000], F32)
    assert segment_cell_count(a, a + F32(28 * 64), 16384, 64) <= MAX_CELLS < segment_cell_count(a, a + F32(34 * 64), 16384, 64)
    assert segment_cell_count(np.array([100, 8000, 8000], F32), np.array([16000, 8000, 8000], F32), 16384, 64) <= MAX_CELLS


def test_first_hits_against_brute_force():
    """render_engine_amd.first_hits: per query the record with the smallest (t_enter, entity_id), ties by entity id, none for a query without hits"""
    import render_engine_amd as R
    rng = np.random.default_rng(11)
    n = 40
    hits = np.zeros(600, SEGMENT_HIT_DT)
    hits["query"] = rng.integers(0, n - 3, len(hits))                              # (the last three queries hit nothing)
    hits["entity_id"] = rng.permutation(len(hits)).astype(np.uint32)
    hits["t_enter"] = rng.integers(0, 6, len(hits)).astype(F32) / F32(8.0)         # few values: ties abound
    hits["t_exit"] = hits["t_enter"] + F32(0.125)
    recs = sorted(zip(hits["query"].tolist(), hits["entity_id"].tolist(), hits["t_enter"].view(np.uint32).tolist(), hits["t_exit"].view(np.uint32).tolist()))
    want = first_hits_brute(recs, n)
    first, found = R.first_hits(hits, n)
    assert first.dtype == R._capi.SEGMENT_HIT_DT and len(first) == n == len(found)
    ties = 0
    for i in range(n):
        assert found[i] == (want[i] is not None)
        assert int(first["query"][i]) == i
        if want[i] is not None:
            assert (i, int(first["entity_id"][i]), bits(first["t_enter"][i]), bits(first["t_exit"][i])) == want[i]
            ties += sum(1 for r in recs if r[0] == i and r[2] == want[i][2]) > 1
    assert ties >= 5 and not found[n - 3:].any()
    first, found = R.first_hits(hits[:0], 4)
    assert len(first) == 4 and not found.any()
