"""The rule of re_query_boxes and the cell ranges of its walk (tests/box_query_rule.py) against the oracle's own section decisions: the hand-worked
boundary cases, and the property the walk rests on -- every entity whose stored AABB intersects a box has at least one of its section keys inside the
box's cell range of that key's level."""
import numpy as np
import pytest

import oracle as ro
from helpers import to_oracle, oracle_camera
from box_query_rule import (MAX_CELLS, box_hits, query_cell_ranges, candidate_cell_count, key_in_ranges, probe_world, probe_push_out, probe_queries,
                            query_world, draw_boxes, N_CROWD, overflow_world, overflow_queries, assert_overflow_placement)
from test_logic_rule import camera_draw

WORLDS = [(2500, 5, 160.0, 64), (1500, 13, 150.0, 16)]      # n, seed, spread, atomic: the worlds of test_logic_gpu.py


@pytest.mark.parametrize("atomic", [64, 16])
def test_hand_worked_boundaries(atomic):
    """the section decisions the walk has to follow, written out (outline 16384; coordinates in units of atomic / 64)"""
    w = ro.World(16384, atomic)
    assert w.register(to_oracle(probe_world(atomic))) == 0
    w.apply_changes(probe_push_out().view(ro.CHANGE_DT))
    last = 16384 // atomic
    K = ro.pack_key
    assert w.lookup(0) == (1, [K(0, 0, 0, 0)])                                   # x in [10, 64]: the lower section only
    assert w.lookup(1) == (1, [K(0, 1, 0, 0)])                                   # x in [64, 100]
    assert w.lookup(2)[0] == 2 and sorted(w.lookup(2)[1]) == [K(0, 0, 0, 0), K(0, 1, 0, 0)]      # x in [63.5, 64.5]: shared over both
    assert w.lookup(3) == (1, [K(0, last, 0, 0)])                                # out of bounds, kept: one past the grid
    assert w.lookup(4) == (1, [K(0, 0, 0, 0)]) and w.lookup(5) == (1, [K(0, 1, 1, 1)])
    assert w.entity(3)["flags"] & ro.F_OOB_LOGIC
    q, want = probe_queries(atomic)
    got = box_hits(w, range(6), q)
    assert got == want
    assert (0, 0) in got and (0, 1) in got and (0, 2) in got                     # x in [64, 70] meets [10, 64] at x = 64
    assert (1, 0) not in got and (1, 4) not in got                               # one float above: no longer
    assert (2, 3) in got                                                         # beyond the world: the clipped entity
    # ... and the ranges find them: [10, 64] sits in cell 0, which only the minus-one step reaches from a minimum of exactly 64
    r0 = query_cell_ranges(q[0], 16384, atomic)
    assert r0[0][0] == (0, 1) and query_cell_ranges(q[0], 16384, atomic, minus_one=False)[0][0] == (1, 1)
    assert query_cell_ranges(q[1], 16384, atomic)[0][0] == (1, 1)
    assert query_cell_ranges(q[2], 16384, atomic)[0][0] == (last - 1, last)      # hi is not clamped to the grid
    for i, e in want:
        assert any(key_in_ranges(k, query_cell_ranges(q[i], 16384, atomic)) for k in w.lookup(e)[1]), (i, e)
    # the filter
    assert box_hits(w, range(6), q, need=ro.F_OOB_LOGIC) == [(2, 3)] and (2, 3) not in box_hits(w, range(6), q, forbid=ro.F_OOB_LOGIC)
    w.close()


@pytest.mark.parametrize("n,seed,spread,atomic", WORLDS)
def test_every_hit_has_a_key_in_the_cell_ranges(n, seed, spread, atomic):
    """the superset property, after 0, 3 and 6 ticks of the oracle, over 64 boxes each: random sizes, snapped faces, boxes partly outside the world"""
    import render_engine_amd as R
    ents = query_world(n, seed, spread, atomic)
    w = ro.World(16384, atomic)
    assert w.register(to_oracle(ents)) == 0
    ids = [int(i) for i in ents["id"]]
    rng = np.random.default_rng(seed)
    pairs = through_shared = minus_one_only = 0
    for stage in range(3):
        boxes = draw_boxes(w, ids, rng, 16384)
        ranges = [query_cell_ranges(b, 16384, atomic) for b in boxes]
        plain = [query_cell_ranges(b, 16384, atomic, minus_one=False) for b in boxes]
        for b in boxes:
            assert candidate_cell_count(b, 16384, atomic) <= MAX_CELLS
        for i, e in box_hits(w, ids, boxes):
            kind, keys = w.lookup(e)
            assert any(key_in_ranges(k, ranges[i]) for k in keys), (stage, i, e, boxes[i], w.entity(e)["aabb"], [ro.unpack_key(k) for k in keys])
            pairs += 1; through_shared += kind == 2
            minus_one_only += not any(key_in_ranges(k, plain[i]) for k in keys)
        for _ in range(3):
            w.tick(oracle_camera(camera_draw(R, rng, spread)), 0.05)
    assert pairs >= 200 and through_shared >= 20 and minus_one_only >= 5, (pairs, through_shared, minus_one_only)
    w.close()


@pytest.mark.parametrize("atomic", [64, 16])
def test_overflow_world_exceeds_the_staging_buffer(atomic):
    """the precondition of the GPU test of the overflow paths (test_box_query_gpu.py): the placement of overflow_world, and both boxes return more
    records than a workgroup stages"""
    ents = overflow_world(atomic)
    w = ro.World(16384, atomic)
    assert w.register(to_oracle(ents)) == 0
    assert_overflow_placement(w)
    boxes, _, _ = overflow_queries(atomic)
    got = box_hits(w, [int(i) for i in ents["id"]], boxes)
    per_query = [sum(1 for i, _ in got if i == q) for q in range(2)]
    assert per_query == [N_CROWD + 1, N_CROWD] == [1101, 1100]
    assert min(per_query) > 1024                                                 # BOXQ_HITBUF (re_kernels.h)
    assert sorted(e for i, e in got if i == 0) == [5] + list(range(100, 100 + N_CROWD)) and sorted(e for i, e in got if i == 1) == list(range(5000, 5000 + N_CROWD))
    w.close()


def test_the_cap_on_candidate_cells():
    """a 200-unit box is a few hundred cells; a 3000-unit box exceeds the cap (about 30 atomic lengths a side)"""
    assert candidate_cell_count([8100, 8300] * 3, 16384, 64) < 400
    assert candidate_cell_count([7000, 10000] * 3, 16384, 64) > MAX_CELLS
    assert candidate_cell_count([8000, 8000 + 28 * 64] * 3, 16384, 64) <= MAX_CELLS < candidate_cell_count([8000, 8000 + 32 * 64] * 3, 16384, 64)
