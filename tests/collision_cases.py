"""Known answers of the collision pass (LogicFlow::handle_collisions, flows/logic_flow.rs:452-651), shared by the CPU tests of
the oracle (test_oracle_flows.py, test_collision_cases.py) and the device tests (test_collision_gpu.py).  Every scenario carries
its entity records, its cameras as (position, direction, far draw distance) and the expected (this, other) pairs written out by
hand; the worlds derived from the reference's find_related_entities known answer carry the rule that derives theirs."""
import json
import os

import numpy as np

import oracle as ro

MV = ro.F_HAS_VEL | ro.F_CAN_COLLIDE


def ent(i, pos, half, flags, vel=(0, 0, 0)):
    e = np.zeros(1, ro.ENTITY_DT)[0]
    e["id"] = i; e["flags"] = flags
    e["original"] = (-half, half, -half, half, -half, half)
    e["pos"] = pos; e["scale"] = (1, 1, 1); e["rot_axis"] = (1, 0, 0); e["vel"] = vel
    return e


def box_ent(i, box, flags, vel=(0, 0, 0)):
    """an entity at the origin with the identity transform: its StaticAABB is `box` (xmin, xmax, ymin, ymax, zmin, zmax)"""
    e = np.zeros(1, ro.ENTITY_DT)[0]
    e["id"] = i; e["flags"] = flags
    e["original"] = tuple(box)
    e["pos"] = (0, 0, 0); e["scale"] = (1, 1, 1); e["rot_axis"] = (1, 0, 0); e["rotvel_axis"] = (1, 0, 0); e["rotacc_axis"] = (1, 0, 0); e["vel"] = vel
    return e


def records(ents):
    return np.array(ents, ro.ENTITY_DT)


# --- hand case 1: one level-0 world section next to the camera, listed twice in visible_sections_vec (logic box and frustum), so
# its moved entities are pushed twice (:214-223, 443-446):
#   1 mover, large, CanCauseCollisions         -- the moved entity
#   2 at rest (no Velocity), touches 1         -- (1,2) and (2,1): both collision functions run (:640-647)
#   3 mover with CanCauseCollisions, touches 1 -- (1,3) from 1's pass and (3,1) from 3's pass, each only-to-self (:625-637)
#   4 static, touches 1                        -- static_entities are not searched (find_related_entities returns local_entities)
#   5 at rest, apart                           -- no overlap
#   6 mover WITHOUT CanCauseCollisions, touches 1 -- not a moved entity: treated like 2
#   7 at rest, touches 1 only along a face (closed intervals, range.rs:71)
HAND = dict(
    outline=16384, atomic=64,
    ents=[
        ent(1, (8210, 8210, 8210), 5.0, MV, (1, 0, 0)),
        ent(2, (8216, 8210, 8210), 2.0, 0),
        ent(3, (8204, 8210, 8210), 2.0, MV, (0, 1, 0)),
        ent(4, (8210, 8216, 8210), 2.0, ro.F_STATIC),
        ent(5, (8240, 8240, 8240), 2.0, 0),
        ent(6, (8210, 8204, 8210), 2.0, ro.F_HAS_VEL, (0, 0, 1)),
        ent(7, (8210, 8210, 8217), 2.0, 0),
    ],
    cam=((8210, 8210, 8290), (0, 0, -1), 1000.0),
    section=ro.pack_key(0, 8210 // 64, 8210 // 64, 8210 // 64),
    listed=2,
    once=[(1, 2), (2, 1), (1, 3), (3, 1), (1, 6), (6, 1), (1, 7), (7, 1)],
    # farther than 200 units from the section: nothing is tested (:553-558), although the section is still visible
    cam_far=((8210, 8210, 8210 + 64 + 260), (0, 0, -1), 1000.0),
)
HAND["expected"] = sorted(HAND["once"] * HAND["listed"])

# --- hand case 2: a moved entity stored under a Shared lookup that is the first to touch a world section creates the section's
# entry WITHOUT being pushed into it (logic_flow.rs:488-498), so alone it collides with nothing; a second moved entity in the same
# sections then does.  A large entity one level up is found through related_world_sections (the parent section).
SHARED = dict(
    outline=16384, atomic=64,
    base=[
        ent(10, (8256, 8210, 8210), 4.0, MV, (1, 0, 0)),          # straddles x = 8256: shared section of two level-0 sections
        ent(11, (8250, 8210, 8210), 3.0, 0),                        # at rest in the left section, touches 10
        ent(12, (8256, 8256, 8256), 50.0, 0),                       # level-1 section (parent of both), touches 10
    ],
    second=ent(20, (8256, 8212, 8212), 3.0, MV, (0, 1, 0)),        # same shared section, larger id
    cam=((8240, 8210, 8290), (0, 0, -1), 1000.0),
    expected_alone=[],                                               # 10 created both entries and is in neither
    # 20 is pushed into both sections' entries (10 created them): per section, 20 against 10 (moved: only-to-self), 11 and 12 (at rest: both ways)
    per_section=[(20, 10), (20, 11), (11, 20), (20, 12), (12, 20)],
    sections=2,
)
SHARED["expected"] = sorted(SHARED["per_section"] * SHARED["sections"])


# --- the reference's own known answer of find_related_entities (bounding_box_tree_v2.rs:2220-2303, tests/golden/tree_cells.json),
# turned into collision worlds: one world per golden entity, in which that entity is the lone moved entity (Velocity of zero and
# CanCauseCollisions) and every other golden entity is at rest.  The boxes are small integers, so the intersections are exact.
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tree_cells.json")))
_F = GOLDEN["find_related"]
GOLDEN_BOXES = [tuple(b) for b in _F["adds"]]
GOLDEN_CAM = ((70, 40, 150), (0, 0, -1), 1000.0)                  # every golden box lies within 200 units
# the case that must not be lost: entity 5, [128,138]x[0,10]x[0,10], touches entity 4, [0,128]^3, on the face x = 128 -- the boxes
# intersect (closed intervals), but their sections (0,4,0,0) and (2,0,0,0) are unrelated: no pair in either direction
GOLDEN_TOUCHING_UNRELATED = (4, 5)


def _key(s):
    return ro.pack_key(*[int(v) for v in s.split(",")])


def intersects(a, b):
    """StaticAABB::intersect (aabb.rs:68-73): closed intervals"""
    return all(a[2 * k] <= b[2 * k + 1] and a[2 * k + 1] >= b[2 * k] for k in range(3))


def golden_section(e):
    """('unique', key) or ('shared', (keys...)) of golden entity e, read off the golden queries"""
    for q in _F["queries"]:
        for k, members in q["unique"].items():
            if e in members:
                return "unique", _key(k)
        for s in q["shared"]:
            if e in s["entities"]:
                return "shared", tuple(ro.pack_key(*i) for i in s["ids"])
    raise KeyError(e)


def golden_world(mover):
    return records([box_ent(i, b, MV if i == mover else 0) for i, b in enumerate(GOLDEN_BOXES)])


def golden_expected(mover, listed):
    """the pairs of the world in which `mover` is the lone moved entity.  listed(key): how often the section is listed in
    visible_sections_vec for the camera in use (asserted by the caller from the visible set, not assumed here)."""
    kind, where = golden_section(mover)
    if kind == "shared":
        return []               # first to touch its sections through a Shared lookup: pushed into none (logic_flow.rs:488-498)
    q = [q for q in _F["queries"] if any(_key(k) == where for k in q["unique"])]
    assert len(q) >= 1 and all(x["unique"] == q[0]["unique"] and x["shared"] == q[0]["shared"] for x in q)
    partners = sorted({e for members in q[0]["unique"].values() for e in members} | {e for s in q[0]["shared"] for e in s["entities"]})
    out = []
    for o in partners:
        if o != mover and intersects(GOLDEN_BOXES[mover], GOLDEN_BOXES[o]):
            out += [(mover, o), (o, mover)] * listed(where)     # the partner is at rest: both directions (:640-647)
    return sorted(out)
