"""The rule of re_query_segments restated on the CPU, plain numpy over the oracle (no GPU, no product code): which (query, entity, t_enter, t_exit)
records a batch of segments returns, and what the walk of k_segment_query may leave out -- the per-level cell ranges of the segment's bounding box
(box_query_rule.query_cell_ranges) and the prune of a candidate cell against the segment itself.  tests/test_segment_rule.py checks both against the
oracle's own section decisions; the GPU tests compare the library with segment_hits.

The slab test, in plain f32 (numpy float32 scalars and arrays: every operation rounds once, IEEE division), in this order:
    lo = 0, hi = 1
    for a in x, y, z:   (mn, mx = the box's bounds on a)
        if d[a] == 0:  if !(p0[a] >= mn && p0[a] <= mx) -> miss
        else:          u = (mn - p0[a]) / d[a];  v = (mx - p0[a]) / d[a];  if u > v swap
                       if u > lo: lo = u;   if v < hi: hi = v
    hit iff lo <= hi;   t_enter = lo, t_exit = hi
d = p1 - p0 (one f32 subtraction per axis), a subnormal component replaced by 0."""
import numpy as np

import oracle as ro
from box_query_rule import MAX_CELLS, N_BORDER, tree_entities, query_cell_ranges, candidate_cell_count

F32 = np.float32
NO_ENTITY = 0xFFFFFFFF           # RE_SEGMENT_NO_ENTITY
TINY = np.finfo(np.float32).tiny
SEGMENT_HIT_DT = np.dtype([("query", "u4"), ("entity_id", "u4"), ("t_enter", "f4"), ("t_exit", "f4")])


def direction(p0, p1):
    """d = p1 - p0 in f32, subnormal components replaced by 0 (the host does it once and carries d in the record)"""
    d = np.asarray(p1, F32) - np.asarray(p0, F32)
    return np.where(np.abs(d) < TINY, F32(0.0), d).astype(F32)


def slab(p0, d, boxes):
    """(hit, t_enter, t_exit) of one segment against boxes [n, 6] (xmin xmax ymin ymax zmin zmax; bounds may be infinite)"""
    boxes = np.asarray(boxes, F32).reshape(-1, 6)
    n = len(boxes)
    lo, hi, ok = np.zeros(n, F32), np.ones(n, F32), np.ones(n, bool)
    with np.errstate(over="ignore"):
        for a in range(3):
            mn, mx = boxes[:, 2 * a], boxes[:, 2 * a + 1]
            if d[a] == 0:
                ok &= (p0[a] >= mn) & (p0[a] <= mx)
                continue
            u, v = (mn - p0[a]) / d[a], (mx - p0[a]) / d[a]
            swap = u > v
            u, v = np.where(swap, v, u), np.where(swap, u, v)
            lo = np.where(u > lo, u, lo); hi = np.where(v < hi, v, hi)
    return ok & (lo <= hi), lo, hi


def segment_hits(w, ids, p0, p1, exclude=None, need=0, forbid=0):
    """sorted [(query, entity_id, bits of t_enter, bits of t_exit)]: brute force, the slab test of every segment with the stored AABB of every entity in
    the tree, filtered by (flags & need) == need and (flags & forbid) == 0 and by the segment's excluded entity"""
    eid, ab, fl = tree_entities(w, ids)
    p0 = np.asarray(p0, F32).reshape(-1, 3); p1 = np.asarray(p1, F32).reshape(-1, 3)
    ok = ((fl & np.uint32(need)) == np.uint32(need)) & ((fl & np.uint32(forbid)) == 0)
    out = []
    for i in range(len(p0)):
        hit, lo, hi = slab(p0[i], direction(p0[i], p1[i]), ab)
        hit &= ok
        if exclude is not None and int(exclude[i]) != NO_ENTITY:
            hit &= eid != np.uint32(exclude[i])
        out += [(i, int(e), int(a), int(b)) for e, a, b in zip(eid[hit], lo[hit].view(np.uint32), hi[hit].view(np.uint32))]
    return sorted(out)


def records_of(hits):
    """a SEGMENT_HIT_DT array in the form segment_hits returns"""
    return sorted(zip(hits["query"].tolist(), hits["entity_id"].tolist(), hits["t_enter"].view(np.uint32).tolist(), hits["t_exit"].view(np.uint32).tolist()))


def first_hits_brute(recs, n):
    """per query the record with the smallest (t_enter, entity_id), or None: recs as segment_hits returns them"""
    out = [None] * n
    for r in recs:
        t = np.array([r[2]], np.uint32).view(F32)[0]
        if out[r[0]] is None or (t, r[1]) < (out[r[0]][0], out[r[0]][1][1]):
            out[r[0]] = (t, r)
    return [None if o is None else o[1] for o in out]


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------------

def margin(outline):
    """the inflation of the cell boxes the prune tests and of the segment's bounding box: outline * 2^-12.  The slab test's rounding error in world units is
    bounded by about outline * 2^-21 (three rounded operations on t <= 1 times |d| <= sqrt(3) * outline, plus the ulp of the coordinates)."""
    return F32(outline) * F32(1.0 / 4096.0)


def bounding_box(p0, p1, outline, inflate=True):
    """the box whose per-level cell ranges hold the candidate cells: min / max of the endpoints per axis, inflated by the margin -- the slab test accepts
    t = 1 after rounding for a face a few ulps beyond p1, which the raw bounding box no longer meets"""
    p0, p1 = np.asarray(p0, F32), np.asarray(p1, F32)
    m = margin(outline) if inflate else F32(0.0)
    out = np.zeros(6, F32)
    out[0::2] = np.minimum(p0, p1) - m; out[1::2] = np.maximum(p0, p1) + m
    return out


def segment_cell_count(p0, p1, outline, atomic):
    return candidate_cell_count(bounding_box(p0, p1, outline), outline, atomic)


def cell_box(cells, outline, atomic, inflate=True, extend=True):
    """the closed box of the cells [(level, x0, y0, z0, x1, y1, z1)] (a unique section: one cell; a shared section: the bounding cell box of its keys) in
    world units, inflated by the margin; minus infinity on an axis where the lower bound is 0, plus infinity where the upper bound reaches the outline:
    entities clipped to the world sit in those cells, and the exact test runs on their unclipped boxes"""
    lo = np.full(3, np.inf); hi = np.zeros(3)
    for level, x, y, z in cells:
        ln = atomic << level
        c = np.array([x, y, z], np.int64) * ln
        lo = np.minimum(lo, c); hi = np.maximum(hi, c + ln)
    m = margin(outline) if inflate else F32(0.0)
    out = np.zeros(6, F32)
    for a in range(3):
        out[2 * a] = F32(-np.inf) if extend and lo[a] == 0 else F32(lo[a]) - m
        out[2 * a + 1] = F32(np.inf) if extend and hi[a] >= outline else F32(hi[a]) + m
    return out


def key_cells(keys):
    out = []
    for k in keys:
        level, x, z, y = ro.unpack_key(k)
        out.append((level, x, y, z))
    return out


def prune_passes(p0, d, cells, outline, atomic, **k):
    return bool(slab(p0, d, cell_box(cells, outline, atomic, **k))[0][0])


def pruned_fraction(p0, p1, outline, atomic):
    """(candidate cells of the bounding box's ranges over all levels, those of them the prune lets through to the probe)"""
    d = direction(p0, p1)
    total = kept = 0
    m = margin(outline)
    for level, axes in enumerate(query_cell_ranges(bounding_box(p0, p1, outline), outline, atomic)):
        ln = atomic << level
        grids = np.meshgrid(*[np.arange(lo, hi + 1, dtype=np.int64) for lo, hi in axes], indexing="ij")
        c = np.stack([g.ravel() for g in grids], axis=1) * ln                  # [cells, 3] lower corners
        boxes = np.zeros((len(c), 6), F32)
        for a in range(3):
            boxes[:, 2 * a] = np.where(c[:, a] == 0, F32(-np.inf), c[:, a].astype(F32) - m)
            boxes[:, 2 * a + 1] = np.where(c[:, a] + ln >= outline, F32(np.inf), (c[:, a] + ln).astype(F32) + m)
        total += len(c); kept += int(slab(np.asarray(p0, F32), d, boxes)[0].sum())
    return total, kept


# ---- the draw -------------------------------------------------------------------------------------------------------------------------------------

def draw_segments(w, ids, rng, outline, atomic, n=64):
    """(p0, p1) [n, 3] each: p0 near a random entity of the tree, length 1 to 1500 units, in a random direction through the neighbourhood of the entity;
    every fourth (j % 4 == 1) axis-aligned along one of the border entities of query_world, its coordinates on that axis snapped to multiples of 64 or
    128 and the other two either through the entity or (every second of them) in the plane of one of its faces; j % 16 == 3 crossing a face of the
    world; j % 16 == 7 a point (p0 == p1), inside an entity for every second of them; j % 16 == 11 ending exactly on a face of an entity.  A segment
    whose bounding box exceeds the cap on candidate cells is halved until it passes."""
    eid, ab, _ = tree_entities(w, ids)
    border = np.nonzero(np.isin(eid, sorted(ids)[-N_BORDER:]))[0]
    p0, p1 = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    for j in range(n):
        i = int(rng.choice(border)) if j % 4 == 1 and len(border) else int(rng.integers(len(eid)))
        box = ab[i].reshape(3, 2)
        c = (box[:, 0] + box[:, 1]) * F32(0.5)
        length = F32(rng.uniform(1, 1500))
        dirn = rng.normal(size=3); dirn = (dirn / np.linalg.norm(dirn)).astype(F32)
        if j % 4 == 1:
            a = int(rng.integers(3))
            step = F32(64.0 if j % 8 == 1 else 128.0)
            a0 = np.round((c[a] - length * F32(rng.uniform(0, 1))) / step) * step
            a1 = np.round((a0 + length) / step) * step
            if a1 <= a0:
                a1 = a0 + step
            s, e = c.copy(), c.copy()
            if j % 8 == 5:                                         # in the plane of a face of the entity: a touch-only hit
                b = (a + 1) % 3
                s[b] = e[b] = box[b, (j // 8) % 2]
            s[a], e[a] = (a0, a1) if (j // 16) % 2 else (a1, a0)
        elif j % 16 == 7:
            s = c + (F32(0.0) if (j // 16) % 2 else (box[:, 1] - box[:, 0]) * F32(0.5) + F32(rng.uniform(0.5, 5)))
            e = s.copy()
        elif j % 16 == 11:                                         # from outside onto the middle of a face: t_enter == t_exit == 1
            a, side = int(rng.integers(3)), int(rng.integers(2))
            e = c.copy(); e[a] = box[a, side]
            dirn[a] = abs(dirn[a]) + F32(0.2) if side else -abs(dirn[a]) - F32(0.2)
            s = e + dirn * length
        else:
            s = c + rng.uniform(-20, 20, 3).astype(F32) - dirn * length * F32(rng.uniform(0, 1))
            e = s + dirn * length
            if j % 16 == 3:
                a = (j // 16) % 3
                shift = (F32(outline) if (j // 16) % 2 else F32(0.0)) - (s[a] + e[a]) * F32(0.5)
                s[a] += shift; e[a] += shift
        s, e = np.asarray(s, F32), np.asarray(e, F32)
        while segment_cell_count(s, e, outline, atomic) > MAX_CELLS:
            if j % 16 == 11:
                s = e + (s - e) * F32(0.5)                         # (the end stays on the face)
            else:
                e = s + (e - s) * F32(0.5)
        p0[j], p1[j] = s, e
    return p0, p1
