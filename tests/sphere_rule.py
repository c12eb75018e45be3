"""The rule of re_query_spheres restated on the CPU, plain numpy over the oracle (no GPU, no product code): which (query, entity, dist_sq, side) records
a batch of spheres returns, and what the walk of k_sphere_query may leave out -- the per-level cell ranges of the sphere's bounding cube
(box_query_rule.query_cell_ranges) and the prune of a candidate cell against the sphere itself.  tests/test_sphere_rule.py checks both against the
oracle's own section decisions; the GPU tests compare the library with sphere_hits.

Sphere i has a centre c and a radius r; r2 = r * r is one f32 multiplication.  One record for every entity that re_query_boxes would consider (live,
row_cell set, not F_PHANTOM, no ghost instance; the same need / forbid filter, RE_F_STATIC follows the tree), that is not the sphere's exclude_entity
and whose stored, unclipped StaticAABB passes this test, in plain f32 (numpy float32 scalars and arrays: every operation rounds once, no contraction,
compares written as compares, not fmin / fmax):
    side = 0
    for a in x, y, z:   (mn, mx = the box's bounds on a)
        if      c[a] < mn:  e[a] = mn - c[a];  side |= 1 << a
        else if c[a] > mx:  e[a] = c[a] - mx;  side |= 16 << a
        else:               e[a] = 0
    dist_sq = (e[x]*e[x] + e[y]*e[y]) + e[z]*e[z]
    hit iff dist_sq <= r2
The test is closed: a sphere that only touches a face, an edge or a corner hits.  r == 0 is a point query.  side == 0 exactly when the centre is inside
the box; then dist_sq == 0.  An overflowing product gives inf, which misses.  Each pair once, in no particular order.  The nearest entity of a query is
the record with the smallest (dist_sq, entity_id)."""
import numpy as np

from box_query_rule import MAX_CELLS, N_BORDER, tree_entities, query_cell_ranges, candidate_cell_count
from segment_rule import margin, cell_box, key_cells  # noqa: F401  (key_cells: for the callers)

F32 = np.float32
NO_ENTITY = 0xFFFFFFFF           # RE_SPHERE_NO_ENTITY
SPHERE_HIT_DT = np.dtype([("query", "u4"), ("entity_id", "u4"), ("dist_sq", "f4"), ("side", "u4")])


def dist_sq(c, boxes):
    """(dist_sq f32 [n], side u32 [n]) of the point c against boxes [n, 6] (xmin xmax ymin ymax zmin zmax; bounds may be infinite: both compares are
    false then and e = 0)"""
    boxes = np.asarray(boxes, F32).reshape(-1, 6)
    c = np.asarray(c, F32)
    side = np.zeros(len(boxes), np.uint32)
    e = []
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            mn, mx = boxes[:, 2 * a], boxes[:, 2 * a + 1]
            below, above = c[a] < mn, ~(c[a] < mn) & (c[a] > mx)
            e.append(np.where(below, mn - c[a], np.where(above, c[a] - mx, F32(0.0))).astype(F32))
            side |= np.where(below, np.uint32(1 << a), np.where(above, np.uint32(16 << a), np.uint32(0))).astype(np.uint32)
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    return d2.astype(F32), side


def radius_sq(r):
    with np.errstate(over="ignore"):
        return F32(r) * F32(r)


def sphere_hits(w, ids, c, r, exclude=None, need=0, forbid=0):
    """sorted [(query, entity_id, bits of dist_sq, side)]: brute force, the test of every sphere with the stored AABB of every entity in the tree,
    filtered by (flags & need) == need and (flags & forbid) == 0 and by the sphere's excluded entity"""
    eid, ab, fl = tree_entities(w, ids)
    c = np.asarray(c, F32).reshape(-1, 3); r = np.asarray(r, F32).reshape(-1)
    ok = ((fl & np.uint32(need)) == np.uint32(need)) & ((fl & np.uint32(forbid)) == 0)
    out = []
    for i in range(len(c)):
        d2, side = dist_sq(c[i], ab)
        hit = ok & (d2 <= radius_sq(r[i]))
        if exclude is not None and int(exclude[i]) != NO_ENTITY:
            hit &= eid != np.uint32(exclude[i])
        out += [(i, int(e), int(a), int(b)) for e, a, b in zip(eid[hit], d2[hit].view(np.uint32), side[hit])]
    return sorted(out)


def records_of(hits):
    """a SPHERE_HIT_DT array in the form sphere_hits returns"""
    return sorted(zip(hits["query"].tolist(), hits["entity_id"].tolist(), hits["dist_sq"].view(np.uint32).tolist(), hits["side"].tolist()))


def nearest_brute(recs, n):
    """per query the record with the smallest (dist_sq, entity_id), or None: recs as sphere_hits returns them"""
    out = [None] * n
    for rec in recs:
        d = np.array([rec[2]], np.uint32).view(F32)[0]
        if out[rec[0]] is None or (d, rec[1]) < (out[rec[0]][0], out[rec[0]][1][1]):
            out[rec[0]] = (d, rec)
    return [None if o is None else o[1] for o in out]


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------------

def bounding_box(c, r, outline, inflate=True):
    """the box whose per-level cell ranges hold the candidate cells: [(c - r) - m, (c + r) + m] per axis, m = margin(outline): the rounding of c +- r
    and of the test stays below the margin (magnitudes of at most outline * 2^7: one ulp is outline * 2^-16, the margin outline * 2^-12)"""
    c, r = np.asarray(c, F32), F32(r)
    m = margin(outline) if inflate else F32(0.0)
    out = np.zeros(6, F32)
    out[0::2] = (c - r) - m; out[1::2] = (c + r) + m
    return out


def sphere_cell_count(c, r, outline, atomic):
    return candidate_cell_count(bounding_box(c, r, outline), outline, atomic)


def prune_passes(c, r, cells, outline, atomic, **k):
    """the prune by the exact test's own function on the segments' cell box (inflated by the margin, open-ended on a face of the world): conservative
    because a cell box contains the clipped AABB of its members, is open-ended where they were clipped, and f32 subtract, multiply and add are monotone"""
    return bool(dist_sq(c, cell_box(cells, outline, atomic, **k))[0][0] <= radius_sq(r))


def pruned_fraction(c, r, outline, atomic):
    """(candidate cells of the bounding cube's ranges over all levels, those of them the prune lets through to the probe)"""
    total = kept = 0
    m = margin(outline)
    for level, axes in enumerate(query_cell_ranges(bounding_box(c, r, outline), outline, atomic)):
        ln = atomic << level
        grids = np.meshgrid(*[np.arange(lo, hi + 1, dtype=np.int64) for lo, hi in axes], indexing="ij")
        lc = np.stack([g.ravel() for g in grids], axis=1) * ln                 # [cells, 3] lower corners
        boxes = np.zeros((len(lc), 6), F32)
        for a in range(3):
            boxes[:, 2 * a] = np.where(lc[:, a] == 0, F32(-np.inf), lc[:, a].astype(F32) - m)
            boxes[:, 2 * a + 1] = np.where(lc[:, a] + ln >= outline, F32(np.inf), (lc[:, a] + ln).astype(F32) + m)
        total += len(lc); kept += int((dist_sq(c, boxes)[0] <= radius_sq(r)).sum())
    return total, kept


# ---- the draw -------------------------------------------------------------------------------------------------------------------------------------

def draw_spheres(w, ids, rng, outline, atomic, n=64):
    """(c [n, 3], r [n]): the centre near a random entity of the tree, radius 1 to 120 units;
    j % 4 == 1 around one of the border entities of query_world, on the axis whose maximum is a multiple of 64, with a whole-number radius:
        j % 8 == 1 the sphere touches that face: the centre at face + r over the middle of the face (j % 32 == 9: the minimum face, centre at face - r),
        j % 8 == 5 a 3-4-5 touch over an edge of that face: 3k beyond it, 4k beyond a face of the next axis, radius 5k;
    j % 16 == 3 the centre on a face of the world; j % 16 == 7 r = 0, inside an entity for every second of them; j % 16 == 11 a power-of-two radius with
    the centre at a face +- r.  A sphere whose bounding cube exceeds the cap on candidate cells has its radius halved until it passes."""
    eid, ab, _ = tree_entities(w, ids)
    border = np.nonzero(np.isin(eid, sorted(ids)[-N_BORDER:]))[0]
    cs, rs = np.zeros((n, 3), F32), np.zeros(n, F32)
    for j in range(n):
        i = int(rng.choice(border)) if j % 4 == 1 and len(border) else int(rng.integers(len(eid)))
        box = ab[i].reshape(3, 2)
        mid = (box[:, 0] + box[:, 1]) * F32(0.5)
        c = (mid + rng.uniform(-20, 20, 3).astype(F32)).astype(F32)
        r = F32(rng.uniform(1, 120))
        if j % 4 == 1:
            on = [a for a in range(3) if box[a, 1] % F32(64.0) == 0]
            a = on[0] if on else 0
            c = mid.copy()
            if j % 8 == 1:
                r = F32(rng.integers(1, 100))
                c[a] = box[a, 0] - r if j % 32 == 9 else box[a, 1] + r
            else:
                k = F32(rng.integers(1, 20))
                b = (a + 1) % 3
                c[a] = box[a, 1] + F32(3.0) * k
                c[b] = box[b, 1] + F32(4.0) * k if (j // 8) % 2 else box[b, 0] - F32(4.0) * k
                r = F32(5.0) * k
        elif j % 16 == 3:
            a = (j // 16) % 3
            c[a] = F32(outline) if (j // 16) % 2 else F32(0.0)
        elif j % 16 == 7:
            r = F32(0.0)
            c = mid.copy() if (j // 16) % 2 else (mid + (box[:, 1] - box[:, 0]) * F32(0.5) + F32(rng.uniform(0.5, 5))).astype(F32)
        elif j % 16 == 11:
            a, side = int(rng.integers(3)), int(rng.integers(2))
            r = F32(2.0) ** F32(rng.integers(0, 7))
            c = mid.copy(); c[a] = box[a, 1] + r if side else box[a, 0] - r
        c = np.asarray(c, F32)
        while sphere_cell_count(c, r, outline, atomic) > MAX_CELLS:        # (radii up to 120 pass at atomic lengths of 16 and more: 14 atomic lengths do)
            r = r * F32(0.5)
        cs[j], rs[j] = c, r
    return cs, rs
