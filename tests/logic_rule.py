"""CPU restatement of LogicFlow::update_logic (flows/logic_flow.rs:245, body :662-734, find_always_execute_entities :801-837) for the tests of
re_logic_list, over the oracle World's introspection and the oracle's two culler predicates: which entities apply_entity_logic is called for in a
frame, and how often."""
import ctypes as C
from collections import Counter

import numpy as np

import oracle as ro

BRANCHES = ("unique", "twice", "shared_in_view", "shared_out_of_view", "always_unique", "always_shared")


def logic_call_counts(w, oc, ids, stats=None):
    """Counter {entity id: calls of apply_entity_logic} of the frame whose camera is `oc` on the tree as it stands (before the tick).  `ids`: every
    entity id of the world (for the always-execute walk).  `stats` (a dict) receives how often each branch was taken (BRANCHES)."""
    L = ro.lib()
    calls, seen = Counter(), set()
    st = Counter()
    vis = w.cull(oc)                                                  # visible_sections_vec sorted, duplicates included
    cells = w.cells()
    is_static_section = {int(k): bool(s) for k, s in zip(cells["keys"], cells["is_static_section"])}
    shared = w.shared_sections()
    linking = {}
    for si, sh in enumerate(shared):
        for k in sh["keys"]:
            linking.setdefault(k, []).append(si)
    planes = np.ascontiguousarray(ro.make_planes(np.array(list(oc.pv), np.float32)).reshape(24))
    cam = np.array(list(oc.pos), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for key in (int(k) for k in vis):                                 # active_world_sections: the listed sections that are not static sections
        if key not in is_static_section or is_static_section[key]:
            continue
        for e in w.cell_entities(key)[0]:                             # local_entities: once per listing
            calls[int(e)] += 1; st["unique"] += 1
        for si in linking.get(key, ()):
            if si in seen:
                continue
            seen.add(si)
            box = ro.aabb(shared[si]["aabb"])
            if L.ro_logic_aabb_in_view(np.float32(w.atomic), fp(cam), box) or L.ro_frustum_aabb_visible(fp(planes), box):
                for e in shared[si]["active"]:
                    calls[int(e)] += 1; st["shared_in_view"] += 1
            else:
                st["shared_out_of_view"] += 1
    vis_map = {int(k) for k in vis}
    for e in ids:                                                     # find_always_execute_entities: none of the entity's sections is visible
        o = w.entity(int(e))
        if o is None or not (o["flags"] & ro.F_ALWAYS_EXEC):
            continue
        kind, keys = w.lookup(int(e))
        if not keys:
            continue
        if not any(k in vis_map for k in keys):
            calls[int(e)] += 1; st["always_unique" if len(keys) == 1 else "always_shared"] += 1
    st["twice"] = sum(1 for v in calls.values() if v == 2)
    assert all(v in (1, 2) for v in calls.values())
    if stats is not None:
        stats.update(st)
    return calls


def logic_records(calls, types, table):
    """the call list: sorted (entity_id, logic_index, which, times) for the entities with calls whose type is in the table.
    types: {entity id: type identifier}; table: [(type identifier, which)]"""
    index = {t: (i, which) for i, (t, which) in enumerate(table)}
    out = []
    for e, times in calls.items():
        t = types.get(e)
        if t is not None and t in index:
            out.append((e, index[t][0], index[t][1], times))
    return sorted(out)
