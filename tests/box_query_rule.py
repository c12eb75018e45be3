"""The rule of re_query_boxes restated on the CPU, plain numpy over the oracle (no GPU, no product code): which (query, entity) pairs a batch of
boxes returns, and the per-level cell ranges the walk probes, exactly as the host code of the library computes them (make_box_query in re_api.hip,
box_level_range in re_kernels.h).  tests/test_box_query_rule.py checks the ranges against the oracle's own section decisions; the GPU tests compare
the library with box_hits."""
import numpy as np

import oracle as ro

MAX_CELLS = 32768                # RE_BOX_QUERY_MAX_CELLS


def tree_static_ids(w):
    """the entities in the static sets of the tree's sections (BoundingBoxTree::is_entity_static).  The public RE_F_STATIC bit follows the tree: an entity that
    a change request moves is re-added with is_static = false (entity_change_helpers.rs:330) whatever it was registered as, so the oracle's flag word, which
    keeps the registration's bit, is not asked"""
    out = set()
    for key in w.cells()["keys"]:
        out.update(int(e) for e in w.cell_entities(int(key))[1])
    for sh in w.shared_sections():
        out.update(int(e) for e in sh["static"])
    return out


def tree_entities(w, ids):
    """(ids, f32 AABBs [n, 6], flags) of the entities the oracle's tree holds: w.lookup(e) places them in a unique or a shared section"""
    keep, boxes, flags = [], [], []
    static = tree_static_ids(w)
    for e in ids:
        kind, keys = w.lookup(int(e))
        if kind == 0 or not keys:
            continue
        st = w.entity(int(e))
        if st is None:
            continue
        keep.append(int(e)); boxes.append(st["aabb"]); flags.append((st["flags"] & ~ro.F_STATIC) | (ro.F_STATIC if int(e) in static else 0))
    return np.array(keep, np.uint32), np.array(boxes, np.float32).reshape(-1, 6), np.array(flags, np.uint32)


def box_hits(w, ids, boxes, need=0, forbid=0):
    """sorted [(query, entity_id)]: brute force, StaticAABB::intersect (aabb.rs:68-73: a.min <= b.max && a.max >= b.min per axis, closed, f32) of the
    stored AABB of every entity in the tree with every box, filtered by (flags & need) == need and (flags & forbid) == 0"""
    eid, ab, fl = tree_entities(w, ids)
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    ok = ((fl & np.uint32(need)) == np.uint32(need)) & ((fl & np.uint32(forbid)) == 0)
    out = []
    for i, q in enumerate(boxes):
        hit = ok.copy()
        for a in range(3):
            hit &= (ab[:, 2 * a] <= q[2 * a + 1]) & (ab[:, 2 * a + 1] >= q[2 * a])
        out += [(i, int(e)) for e in eid[hit]]
    return sorted(out)


def max_level(outline, atomic):
    return int(ro.lib().ro_max_level(outline, atomic))


def query_cell_ranges(box, outline, atomic, minus_one=True):
    """per level 0 .. max_level (inclusive: an entity longer than half the outline sits there) the cell range [(lo, hi)] * 3 (x, y, z) of the box:
    clip as normalize_aabb does, truncate, integer-divide by the level's section length; hi is not clamped to the grid; lo steps down by one (not
    below 0) when the clipped minimum is an exact multiple of the section length.  minus_one=False leaves that step out (for the test that it matters)."""
    q = np.asarray(box, np.float32)
    L = np.float32(outline)
    out = []
    clip = [np.minimum(np.maximum(v, np.float32(0.0)), L) for v in q]
    for level in range(max_level(outline, atomic) + 1):
        ln = atomic << level
        axes = []
        for a in range(3):
            cmin, cmax = clip[2 * a], clip[2 * a + 1]
            umin, umax = int(cmin), int(cmax)                      # f32 -> u32 truncation (both are >= 0)
            lo, hi = umin // ln, umax // ln
            if minus_one and np.float32(umin) == cmin and lo > 0 and lo * ln == umin:
                lo -= 1
            axes.append((lo, hi))
        out.append(axes)
    return out


def candidate_cell_count(box, outline, atomic):
    n = 0
    for axes in query_cell_ranges(box, outline, atomic):
        p = 1
        for lo, hi in axes:
            p *= hi - lo + 1
        n += p
    return n


def key_in_ranges(key, ranges):
    level, x, z, y = ro.unpack_key(key)
    if level >= len(ranges):
        return False
    (xl, xh), (yl, yh), (zl, zh) = ranges[level]
    return xl <= x <= xh and yl <= y <= yh and zl <= z <= zh


def probe_world(atomic=64, outline=16384):
    """the hand-worked world (coordinates in units of atomic / 64): ids 0..5 are
    0: x in [10, 64]        -> Unique (0, 0, 0, 0): its maximum lies on a section border, it sits in the lower section only
    1: x in [64, 100]       -> Unique (0, 1, 0, 0)
    2: x in [63.5, 64.5]    -> shared over both
    3: x in [outline - 84, outline - 74], RE_F_OOB_LOGIC: probe_push_out moves it by +90 to [outline + 6, outline + 16]; it is kept (add_if_out_bounds),
       clipped to the outline: cell outline / atomic, one past the grid
    4: [0, 64]^3            -> cell (0, 0, 0)
    5: [100, 128]^3         -> cell (1, 1, 1)
    y and z of 0..3 are [10, 20]."""
    import render_engine_amd as R
    s = np.float32(atomic) / np.float32(64.0)
    far = np.float32(outline)
    boxes = np.array([[10, 64, 10, 20, 10, 20], [64, 100, 10, 20, 10, 20], [63.5, 64.5, 10, 20, 10, 20], [0, 0, 10, 20, 10, 20],
                      [0, 64, 0, 64, 0, 64], [100, 128, 100, 128, 100, 128]], np.float32) * s
    boxes[3, 0:2] = (far - np.float32(84.0), far - np.float32(74.0))
    e = np.zeros(len(boxes), R.ENTITY_DT)
    e["id"] = np.arange(len(boxes)); e["original"] = boxes
    e["flags"][3] |= R.F_OOB_LOGIC
    e["scale"] = 1.0; e["rot_axis"][:, 1] = 1.0; e["rotvel_axis"][:, 0] = 1.0; e["rotacc_axis"][:, 2] = 1.0
    return e


def probe_push_out():
    """the change request that moves entity 3 of probe_world out of the world (Modify Position)"""
    import render_engine_amd as R
    ch = np.zeros(1, R.CHANGE_DT)
    ch[0] = (R._capi.CHANGE_MODIFY, 3, R._capi.C_POSITION, 0, (90.0, 0.0, 0.0, 0.0))
    return ch


def probe_queries(atomic=64, outline=16384):
    """[x in [64, 70], x from one float above 64, x beyond the world] (y and z covering [0, 30]) and the pairs they return"""
    s = np.float32(atomic) / np.float32(64.0)
    b = np.float32(64.0) * s
    yz = [np.float32(0.0), np.float32(30.0) * s] * 2
    q = np.array([[b, np.float32(70.0) * s] + yz, [np.nextafter(b, np.float32(np.inf)), np.float32(70.0) * s] + yz,
                  [np.float32(outline) + np.float32(11.0), np.float32(outline) + np.float32(116.0)] + yz], np.float32)
    return q, [(0, 0), (0, 1), (0, 2), (0, 4), (1, 1), (1, 2), (2, 3)]


N_CROWD = 1100                   # more than the 1024 records a query workgroup stages between two flushes (BOXQ_HITBUF)


def overflow_world(atomic=64):
    """probe_world and two crowds of N_CROWD entities each (coordinates in units of atomic / 64):
    ids 100 .. 1199:  copies of entity 5, [100, 128]^3  -> all in the unique section (1, 1, 1) with it: ONE WAVE walks more rows that hit than the
                      workgroup stages (the overflow of the row walk)
    ids 5000 .. 6099: [639, 641]^3, straddling a section corner -> all in one shared section of 8 links: ONE LANE emits more records than the workgroup
                      stages (the overflow of the shared part)"""
    import render_engine_amd as R
    s = np.float32(atomic) / np.float32(64.0)
    base = probe_world(atomic)
    crowd = np.zeros(2 * N_CROWD, R.ENTITY_DT)
    crowd[:] = base[5]
    crowd["id"] = np.concatenate([100 + np.arange(N_CROWD), 5000 + np.arange(N_CROWD)])
    crowd["original"][N_CROWD:] = np.array([639, 641] * 3, np.float32) * s
    return np.concatenate([base, crowd])


def assert_overflow_placement(w):
    """the oracle's placement of overflow_world that the GPU tests of the overflow paths rest on: one key set for the first crowd, one shared section of
    8 links with N_CROWD members for the second"""
    kind5, keys5 = w.lookup(5)
    assert kind5 == 1 and keys5 == [ro.pack_key(0, 1, 1, 1)]
    assert {(w.lookup(e)[0], tuple(w.lookup(e)[1])) for e in range(100, 100 + N_CROWD)} == {(1, tuple(keys5))}
    kind, keys = w.lookup(5000)
    assert kind == 2 and len(keys) == 8
    assert all(w.lookup(e) == (kind, keys) for e in range(5000, 5000 + N_CROWD))
    mine = [sh for sh in w.shared_sections() if sorted(sh["keys"]) == sorted(keys)]
    assert len(mine) == 1 and len(mine[0]["active"]) + len(mine[0]["static"]) == N_CROWD
    assert sorted(int(e) for e in np.concatenate([mine[0]["active"], mine[0]["static"]])) == list(range(5000, 5000 + N_CROWD))


def overflow_queries(atomic=64):
    """(boxes [2, 6], p0 [2, 3], p1 [2, 3]): query 0 over the first crowd of overflow_world (and entity 5: N_CROWD + 1 hits), query 1 over the second
    (N_CROWD hits), as boxes and as segments along x through the middle of each crowd"""
    s = np.float32(atomic) / np.float32(64.0)
    boxes = np.array([[90, 130] * 3, [630, 650] * 3], np.float32) * s
    p0 = np.array([[90, 114, 114], [630, 640, 640]], np.float32) * s
    p1 = np.array([[130, 114, 114], [650, 640, 640]], np.float32) * s
    return boxes, p0, p1


N_BORDER = 12


def query_world(n, seed, spread, atomic):
    """mixed_world(n, seed, spread, atomic) -- unique sections of several levels, shared sections, movers -- with RE_F_CAN_COLLIDE on every third entity
    (the filter of the parity test) and N_BORDER more entities whose maximum on one axis lies exactly on a section border of every level they can
    have (8064, 8192, 8320, 8448: multiples of 128): a random float AABB never does, and those are the entities only the minus-one step of the
    cell range reaches"""
    import render_engine_amd as R
    ents = R.synthetic.mixed_world(n, seed=seed, spread=spread, atomic=atomic)
    ents["flags"][::3] |= R.F_CAN_COLLIDE
    b = np.zeros(N_BORDER, R.ENTITY_DT)
    b["id"] = int(ents["id"].max()) + 100 + np.arange(N_BORDER)
    b["scale"] = 1.0; b["rot_axis"][:, 1] = 1.0; b["rotvel_axis"][:, 0] = 1.0; b["rotacc_axis"][:, 2] = 1.0
    for k in range(N_BORDER):
        a, border = k % 3, np.float32(8064.0 + 128.0 * (k // 3))
        box = np.zeros(6, np.float32)
        for ax in range(3):
            c = np.float32(8192.0 + 25.0 * ((k + ax) % 5 - 2))
            box[2 * ax], box[2 * ax + 1] = c - np.float32(5.0), c + np.float32(5.0)
        box[2 * a], box[2 * a + 1] = border - np.float32(5.0 + 3.0 * k), border
        b["original"][k] = box
        b["flags"][k] = (R.F_STATIC if k % 2 else 0) | (R.F_CAN_COLLIDE if k % 4 == 0 else 0)
    return np.concatenate([ents, b])


def draw_boxes(w, ids, rng, outline, n=64):
    """n query boxes around random entities of the tree, sides 1 to 300 units; every fourth (j % 4 == 1) around one of the border entities with its faces
    snapped to multiples of 64 or 128; four of them (j % 16 == 3) pushed over a face of the world, partly outside"""
    eid, ab, _ = tree_entities(w, ids)
    border = np.nonzero(np.isin(eid, sorted(ids)[-N_BORDER:]))[0]
    out = np.zeros((n, 6), np.float32)
    for j in range(n):
        i = int(rng.choice(border)) if j % 4 == 1 and len(border) else int(rng.integers(len(eid)))
        for a in range(3):
            c = (ab[i, 2 * a] + ab[i, 2 * a + 1]) * np.float32(0.5) + np.float32(rng.uniform(-20, 20))
            h = np.float32(rng.uniform(1, 300)) * np.float32(0.5)
            lo, hi = c - h, c + h
            if j % 4 == 1:
                step = np.float32(64.0 if j % 8 == 1 else 128.0)
                lo, hi = np.round(lo / step) * step, np.round(hi / step) * step
                if hi <= lo:
                    hi = lo + step
            out[j, 2 * a], out[j, 2 * a + 1] = lo, hi
        if j % 16 == 3:
            a = (j // 16) % 3
            side = out[j, 2 * a + 1] - out[j, 2 * a]
            if (j // 16) % 2:
                out[j, 2 * a], out[j, 2 * a + 1] = np.float32(outline) - side / 2, np.float32(outline) + side / 2
            else:
                out[j, 2 * a], out[j, 2 * a + 1] = -side / 2, side / 2
    return out
