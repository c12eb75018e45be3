"""The rule of re_query_boxes_around / re_query_spheres_around restated on the CPU, plain numpy over the oracle (no GPU, no product code): the tree
queries asked by entity.  Ask i names an entity and a reach; the query is formed from the entity's state in the oracle world as it is now --

    boxes:    (min - reach, max + reach) per axis of the asker's stored StaticAABB, one f32 subtraction / addition a bound;
    spheres:  centre = the asker's Position, radius = reach

-- and answered by the siblings' rules (box_query_rule.box_hits, sphere_rule.sphere_hits), minus the asker itself unless the ask says include-self.
An asker that is not in the tree gets NOT_IN_TREE and no hits, a query whose candidate cells (box_query_rule.candidate_cell_count: the box's, or the
inflated bounding cube's) exceed MAX_CELLS gets TOO_LARGE and no hits; the other asks of the batch are answered."""
import numpy as np

from box_query_rule import MAX_CELLS, box_hits, candidate_cell_count, tree_entities
from sphere_rule import NO_ENTITY, sphere_hits, sphere_cell_count

F32 = np.float32
OK, NOT_IN_TREE, TOO_LARGE = 0, 1, 2         # RE_AROUND_OK, RE_AROUND_NOT_IN_TREE, RE_AROUND_TOO_LARGE


def _batch(askers, reach, include_self):
    askers = [int(e) for e in np.asarray(askers).reshape(-1)]
    reach = np.broadcast_to(np.asarray(reach, F32), (len(askers),))
    keep = np.broadcast_to(np.asarray(False if include_self is None else include_self, bool), (len(askers),))
    return askers, reach, keep


def asker_state(w, e):
    """(StaticAABB f32 [6], Position f32 [3]) of an entity of the tree, or None when the oracle's tree does not hold it"""
    kind, keys = w.lookup(int(e))
    st = w.entity(int(e)) if kind != 0 and keys else None
    return None if st is None else (np.asarray(st["aabb"], F32), np.asarray(st["pos"], F32))


def around_boxes(w, askers, reach):
    """(boxes f32 [n, 6], status [n]): xmin - reach, xmax + reach, ... in f32; a refused ask keeps a zero box"""
    askers, reach, _ = _batch(askers, reach, None)
    boxes, status = np.zeros((len(askers), 6), F32), np.zeros(len(askers), np.uint8)
    for i, e in enumerate(askers):
        st = asker_state(w, e)
        if st is None:
            status[i] = NOT_IN_TREE
            continue
        boxes[i, 0::2] = st[0][0::2] - reach[i]; boxes[i, 1::2] = st[0][1::2] + reach[i]
    return boxes, status


def around_box_hits(w, ids, askers, reach, include_self=None, need=0, forbid=0, outline=16384, atomic=64):
    """(sorted [(query, entity_id)], status [n])"""
    askers, reach, keep = _batch(askers, reach, include_self)
    boxes, status = around_boxes(w, askers, reach)
    for i in range(len(askers)):
        if status[i] == OK and candidate_cell_count(boxes[i], outline, atomic) > MAX_CELLS:
            status[i] = TOO_LARGE
    hits = box_hits(w, ids, boxes, need=need, forbid=forbid)
    return [(q, e) for q, e in hits if status[q] == OK and (keep[q] or e != askers[q])], status


def around_spheres(w, askers, reach, include_self=None, outline=16384, atomic=64):
    """(centres f32 [n, 3], radii f32 [n], exclude u32 [n], status [n]): what re_query_spheres would be asked"""
    askers, reach, keep = _batch(askers, reach, include_self)
    c, status = np.zeros((len(askers), 3), F32), np.zeros(len(askers), np.uint8)
    ex = np.array([NO_ENTITY if k else e for e, k in zip(askers, keep)], np.uint32)
    for i, e in enumerate(askers):
        st = asker_state(w, e)
        if st is None:
            status[i] = NOT_IN_TREE
            continue
        c[i] = st[1]
        if sphere_cell_count(c[i], reach[i], outline, atomic) > MAX_CELLS:
            status[i] = TOO_LARGE
    return c, np.array(reach, F32), ex, status


def around_sphere_hits(w, ids, askers, reach, include_self=None, need=0, forbid=0, outline=16384, atomic=64):
    """(sorted [(query, entity_id, bits of dist_sq, side)], status [n])"""
    c, r, ex, status = around_spheres(w, askers, reach, include_self, outline, atomic)
    hits = sphere_hits(w, ids, c, r, exclude=ex, need=need, forbid=forbid)
    return [h for h in hits if status[h[0]] == OK], status


def draw_asks(w, ids, rng, atomic, n=64, border_ids=None):
    """(askers [n], reach f32 [n], include_self [n]): askers drawn among the entities of the tree (every fourth a border entity of query_world), reaches
    from 0 (every eighth) to a few atomic lengths, whole numbers for every fourth; every fifth ask keeps the asker.  Every eighth ask (j % 8 == 5) is a
    border entity k >= 3 -- its maximum on one axis lies on the border 8064 + 128 (k // 3), its minimum 5 + 3 k below -- with the reach that puts its grown
    minimum exactly on the border 128 lower, where border entity k - 3 ends: the hit only the minus-one step of the cell range reaches."""
    from box_query_rule import N_BORDER
    eid, _, _ = tree_entities(w, ids)
    last = sorted(ids)[-N_BORDER:] if border_ids is None else list(border_ids)      # (border_ids: for a caller whose world has grown since)
    border = eid[np.isin(eid, last)]
    askers = np.array([int(rng.choice(border)) if j % 4 == 1 and len(border) else int(rng.choice(eid)) for j in range(n)], np.uint32)
    reach = rng.uniform(0.0, 3.0 * atomic, n).astype(F32)
    reach[0::8] = 0.0
    reach[1::4] = np.floor(reach[1::4])
    for j in range(5, n, 8):
        k = int(rng.integers(3, N_BORDER))
        if last[k] in border:
            askers[j], reach[j] = last[k], F32(128.0 - (5.0 + 3.0 * k))
    return askers, reach, (np.arange(n) % 5 == 4)
