"""The collision broad phase on the device (re_collide: csrc/re_collide.hip and its host half), held to known answers and to the
oracle at the places where its own algorithm can go wrong.  re_collide does not walk related_world_sections: it decides "X is
related to R" from the topmost existing ancestor of X, on top of a region pre-filter around the camera, two key encodings, a
first-touch table and a scratch that cleans itself.  Every comparison is exact equality of the sorted pair multiset and of
n_total, every test states a floor on the number of pairs, and every test ends on assert_clean_publication.

Which key encoding a world runs on follows from its configuration alone (at most 512 world sections per axis: the compact 32-bit
keys; more: the 64-bit keys); re_get_stats does not report it, so the tests pick it through outline / atomic."""
from collections import Counter

import numpy as np
import pytest

import oracle as ro
from helpers import oracle_camera, to_oracle
from test_gpu_parity import R, build_pair, check_frame, sorted_pairs, assert_clean_publication, check_sections  # noqa: F401  (R: fixture)
import collision_cases as cases

pytestmark = pytest.mark.gpu

f32 = np.float32
MV = cases.MV


def pipeline_ents(R, recs):
    return np.ascontiguousarray(cases.records(recs) if isinstance(recs, list) else recs).view(R.ENTITY_DT)


def camera(R, c):
    return R.Camera(*c)


def collide_frame(R, p, w, cam, dups=False, twice=False):
    """one frame on both sides (visible sections and instances compared by check_frame), then the collision pass: n_total and the
    sorted pair multiset equal the oracle's.  Returns the pairs as a sorted list of tuples."""
    check_frame(R, p, w, cam, dups)
    want = sorted_pairs(w.collide(oracle_camera(cam)))
    for _ in range(2 if twice else 1):              # a second call in the same frame: k_col_clear left the table and the row bytes clean
        got, n_total = p.collide()
        assert n_total == len(want), (n_total, len(want))
        np.testing.assert_array_equal(sorted_pairs(got), want)
    assert_clean_publication(p)
    return [tuple(x) for x in want.tolist()]


def device_pairs(R, p, w, cam):
    """the device's pairs alone, for the tests whose expectation is written out (the oracle world only serves check_frame)"""
    check_frame(R, p, w, cam, False)
    got, n_total = p.collide()
    assert n_total == len(got)
    assert_clean_publication(p)
    return sorted(map(tuple, got.tolist()))


def tick_both(p, w, cam, dt=0.05):
    n_o, oob_o = w.tick(oracle_camera(cam), dt); t = p.tick(dt)
    assert t["n_changed"] == n_o and t["n_out_of_bounds"] == len(oob_o)


def listed(p):
    keys, mult = p.visible_sections()
    m = {int(k): int(v) for k, v in zip(keys, mult)}
    return lambda key: m.get(int(key), 0)


# ------------------------------------------------------------------------------------------------------------------------------
# a. known answers on the device, d. on both key encodings (the second outline of each pair: 1024 world sections per axis)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outline", [16384, 65536], ids=["keys32", "keys64"])
def test_hand_case_on_the_device(R, outline):
    """collision_cases.HAND against its written-out pairs: the section next to the camera is listed twice, so every pair comes
    twice; from the far camera the section is still visible, lies farther than 200 units, and nothing is tested"""
    H = cases.HAND
    p, w = build_pair(R, pipeline_ents(R, H["ents"]), outline=outline, atomic=H["atomic"])
    got = device_pairs(R, p, w, camera(R, H["cam"]))
    assert listed(p)(H["section"]) == H["listed"] == 2
    assert got == H["expected"] and len(got) >= 16
    assert all(c == 2 for c in Counter(got).values())                # e: a section listed twice gives multiplicity 2 on every pair
    got_far = device_pairs(R, p, w, camera(R, H["cam_far"]))
    assert listed(p)(H["section"]) >= 1                              # still visible
    assert got_far == []
    assert device_pairs(R, p, w, camera(R, H["cam"])) == H["expected"]   # and back
    p.close(); w.close()


@pytest.mark.parametrize("outline", [16384, 65536], ids=["keys32", "keys64"])
def test_shared_first_touch_on_the_device(R, outline):
    """collision_cases.SHARED against its written-out pairs: alone, the shared mover creates both section entries and is pushed
    into neither; a second mover of the same shared section is pushed into both and meets the parent section's entity from each"""
    S = cases.SHARED
    p, w = build_pair(R, pipeline_ents(R, S["base"]), outline=outline, atomic=S["atomic"])
    assert device_pairs(R, p, w, camera(R, S["cam"])) == S["expected_alone"] == []
    p.close(); w.close()
    p, w = build_pair(R, pipeline_ents(R, S["base"] + [S["second"]]), outline=outline, atomic=S["atomic"])
    got = device_pairs(R, p, w, camera(R, S["cam"]))
    assert got == S["expected"] and len(got) >= 10
    p.close(); w.close()


@pytest.mark.parametrize("outline", [cases.GOLDEN["outline"], 32768], ids=["keys32", "keys64"])
def test_reference_find_related_known_answer_on_the_device(R, outline):
    """the reference's find_related_entities fixture as collision worlds (collision_cases.golden_world), one per golden entity as
    the lone moved entity, against the pairs derived from the golden sets (test_collision_cases.py validates the derivation on
    the CPU).  Entity 5, [128,138]x[0,10]x[0,10], touches entity 4, [0,128]^3, on a face: the boxes intersect, the sections are
    unrelated, and there is no pair in either direction, whichever of the two moves."""
    atomic = cases.GOLDEN["atomic"]
    total = 0
    for mover in range(len(cases.GOLDEN_BOXES)):
        p, w = build_pair(R, pipeline_ents(R, cases.golden_world(mover)), outline=outline, atomic=atomic)
        got = device_pairs(R, p, w, camera(R, cases.GOLDEN_CAM))
        times = listed(p)
        kind, where = cases.golden_section(mover)
        for key in (where if kind == "shared" else (where,)):
            assert times(key) >= 1                                   # the mover's section is listed: an empty answer is the rule's, not the camera's
        assert got == cases.golden_expected(mover, times), mover
        big, small = cases.GOLDEN_TOUCHING_UNRELATED
        assert (big, small) not in got and (small, big) not in got
        if mover in (0, 1, 2, 4):
            assert len(got) >= 8
        total += len(got)
        p.close(); w.close()
    assert total >= 32


# ------------------------------------------------------------------------------------------------------------------------------
# b. the 200-unit cut
# ------------------------------------------------------------------------------------------------------------------------------
def distance_to_aabb(box, cam):
    """distance_to_aabb (helper_things/aabb_helper_functions.rs:58-72) in numpy float32: distance to the centre minus the radius of
    the sphere around the cube of the longest side"""
    box = np.asarray(box, f32); cam = np.asarray(cam, f32)
    h = max(box[1] - box[0], box[3] - box[2], box[5] - box[4]) / f32(2)
    rad = np.sqrt((h * h) * f32(3), dtype=f32)
    d = cam - np.array([(box[0] + box[1]) / f32(2), (box[2] + box[3]) / f32(2), (box[4] + box[5]) / f32(2)], f32)
    return max(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], dtype=f32) - rad, f32(0))


def cameras_at_200(R, box):
    """two cameras on the +x side of `box`, level with its centre and looking at it: the first at a distance of exactly 200.0 from it
    (distance_to_aabb), the second one float further along x"""
    box = np.asarray(box, f32)
    cy, cz = (box[2] + box[3]) / f32(2), (box[4] + box[5]) / f32(2)
    x = f32((box[0] + box[1]) / f32(2) + f32(200) + np.sqrt(f32(3) * ((box[1] - box[0]) / f32(2)) ** 2, dtype=f32))
    while distance_to_aabb(box, (x, cy, cz)) > f32(200):
        x = np.nextafter(x, f32(-np.inf))
    while distance_to_aabb(box, (np.nextafter(x, f32(np.inf)), cy, cz)) <= f32(200):
        x = np.nextafter(x, f32(np.inf))
    x2 = np.nextafter(x, f32(np.inf))
    assert distance_to_aabb(box, (x, cy, cz)) == f32(200.0) and distance_to_aabb(box, (x2, cy, cz)) > f32(200.0)
    return R.Camera((x, cy, cz), (-1, 0, 0), 1000.0), R.Camera((x2, cy, cz), (-1, 0, 0), 1000.0)


def test_cut_at_200_units_unique_section(R):
    """the reference drops a section when distance_to_aabb(section AABB, camera) > 200 (logic_flow.rs:553-558): at exactly 200.0
    the section is kept (!(d > 200)), one float further it is dropped.  One section with a mover (1) and an entity at rest inside
    the mover's box (2): (1,2) and (2,1) at 200.0, nothing beyond."""
    ents = [cases.ent(1, (40, 40, 40), 8.0, MV), cases.ent(2, (41, 41, 41), 2.0, 0)]
    p, w = build_pair(R, pipeline_ents(R, ents))
    cells = w.cells(); assert len(cells["keys"]) == 1
    tight = [float(cells["tight"][0][k]) for k in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")]
    keep, cut = cameras_at_200(R, tight)
    got = collide_frame(R, p, w, keep)
    times = listed(p)(int(cells["keys"][0]))
    assert times >= 1 and got == sorted([(1, 2), (2, 1)] * times)
    assert collide_frame(R, p, w, cut) == [] and listed(p)(int(cells["keys"][0])) >= 1     # still visible, now too far
    assert collide_frame(R, p, w, keep) == got
    p.close(); w.close()


def test_cut_at_200_units_shared_section(R):
    """the same cut on the AABB of a shared section (logic_flow.rs:561-566; k_col_shared).  Mover 1 lies in section (0,0,0); entity
    2, at rest, straddles y = 64 and touches 1 on the face y = 60, so it lives in the shared section of (0,0,0) and (0,1,0), whose
    AABB is 2's box.  With that box at exactly 200.0 from the camera: (1,2) and (2,1); one float further: nothing, while 1's own
    section stays well inside 200."""
    ents = [cases.ent(1, (20, 40, 40), 20.0, MV), cases.ent(2, (20, 64, 40), 4.0, 0)]
    p, w = build_pair(R, pipeline_ents(R, ents))
    sh = w.shared_sections(); assert len(sh) == 1 and sh[0]["active"].tolist() == [2]
    keep, cut = cameras_at_200(R, sh[0]["aabb"])
    sec = ro.pack_key(0, 0, 0, 0)
    cells = w.cells(); own = [float(cells["tight"][list(cells["keys"]).index(sec)][k]) for k in ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")]
    assert distance_to_aabb(own, cut.position) < f32(190)
    got = collide_frame(R, p, w, keep)
    times = listed(p)(sec)
    assert times >= 1 and got == sorted([(1, 2), (2, 1)] * times)
    assert collide_frame(R, p, w, cut) == [] and listed(p)(sec) >= 1
    assert collide_frame(R, p, w, keep) == got
    p.close(); w.close()


# ------------------------------------------------------------------------------------------------------------------------------
# c. closure through high ancestors, d. on both key encodings, with section counts around the 512-key chunks
# ------------------------------------------------------------------------------------------------------------------------------
LARGE, M1, REST, M2, M3, M4, M5, OUT, EDGE, OUT_REST, MID, M6 = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
FILLER0 = 1000


def closure_world(atomic, level, origin_cell, stacked=False, level0_sections=0):
    """Entities of different sibling sections can only meet on a face (a box inside one section may end ON the section's upper
    boundary, bounding_box_tree_v2.rs:1315-1346, and intersections are closed intervals) -- and only an existing common ancestor
    makes their sections related.  S = 2**level sections of level 0 per side of the ancestor's cell, b = S - 3, positions in units
    of the atomic length from the cell's origin:
      LARGE  at rest, [S/4, S]^3: the lone entity of the level-`level` section
      M1     mover in (b,b,b), ends on x = b+1 and begins on z = b
      REST   at rest in (b+1,b,b): touches M1 on x = b+1                       -> (M1,REST), (REST,M1) through the ancestor
      M6     mover in (b+1,b,b): touches M1 on x = b+1, overlaps REST          -> (M6,M1), (M1,M6), (M6,REST), (REST,M6)
      M3     mover in (b+1,b+1,b): touches REST on y = b+1                     -> (M3,REST), (REST,M3)
      M4     mover in (b+2,b,b): touches REST on x = b+2                       -> (M4,REST), (REST,M4)
      M5     mover in (b,b,b-1): touches M1 on z = b                           -> (M5,M1), (M1,M5)
      M2     mover in (b-1,b,b), three sections from M4: meets LARGE alone
      EDGE   at rest in (b+2,b,b), ends on x = S, the ancestor's boundary
      OUT    mover in (S,b,b), the next level-`level` cell: touches EDGE and LARGE on x = S -- adjacent, intersecting, and NOT related:
             no pair with either; OUT_REST, at rest inside OUT's own section, is all it meets
      MID    (stacked) at rest in the level-1 section over (b-1..b)^3, none at level 2: the topmost ancestor of M1's and M5's
             sections is still the level-`level` one
    every mover lies inside LARGE's box and meets it.  level0_sections > 0: filler sections of level 0 in the plane z = b+1, between
    the camera and the rest, one entity at rest each and a mover on every third, up to that many level-0 sections in all."""
    A = float(atomic); S = 1 << level; b = S - 3
    O = np.array(origin_cell, np.float64) * S * A

    def box(i, lo, hi, flags):
        lo = O + np.array(lo) * A; hi = O + np.array(hi) * A
        return cases.box_ent(i, (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]), flags)
    e = [
        box(LARGE, (S / 4, S / 4, S / 4), (S, S, S), 0),
        box(M1, (b + .25, b + .25, b), (b + 1, b + .75, b + .75), MV),
        box(REST, (b + 1, b + .25, b + .25), (b + 2, b + 1, b + .75), 0),
        box(M6, (b + 1, b + .3, b + .3), (b + 1.2, b + .6, b + .6), MV),
        box(M3, (b + 1.1, b + 1, b + .3), (b + 1.4, b + 1.5, b + .7), MV),
        box(M4, (b + 2, b + .25, b + .25), (b + 2.5, b + .75, b + .75), MV),
        box(M5, (b + .3, b + .3, b - .5), (b + .7, b + .7, b), MV),
        box(M2, (b - .75, b + .25, b + .25), (b - .25, b + .75, b + .75), MV),
        box(EDGE, (b + 2.6, b + .25, b + .25), (S, b + .75, b + .75), 0),
        box(OUT, (S, b + .25, b + .25), (S + .5, b + .75, b + .75), MV),
        box(OUT_REST, (S + .1, b + .3, b + .3), (S + .4, b + .6, b + .6), 0),
    ]
    if stacked:
        e.append(box(MID, (b - .8, b - .8, b - .8), (b + .9, b + .9, b + .9), 0))
    n0, i, k, fillers = 7, FILLER0, 0, []
    while n0 < level0_sections:
        x, y = b - 14 + k % 32, b - 14 + k // 32; k += 1
        e.append(box(i, (x + .3, y + .3, b + 1.3), (x + .7, y + .7, b + 1.7), 0)); fillers.append([i]); i += 1
        if (x + y - 2 * b) % 3 == 1:                                    # (b+1, b), the section in front of the camera, is one of them
            e.append(box(i, (x + .4, y + .4, b + 1.4), (x + .8, y + .8, b + 1.8), MV)); fillers[-1].append(i); i += 1
        n0 += 1
    cam = (tuple(O + np.array((b + 1.5, b + .5, b + 2.5)) * A), (0, 0, -1), 1000.0)
    return cases.records(e), cam, O, fillers


def closure_statements(pairs, stacked):
    """what must hold in closure_world, stated by hand; the caller compares the whole multiset with the oracle"""
    have = set(pairs)
    through_ancestor = [(M1, REST), (REST, M1), (M6, M1), (M1, M6), (M6, REST), (REST, M6), (M3, REST), (REST, M3), (M4, REST), (REST, M4), (M5, M1), (M1, M5)]
    assert all(x in have for x in through_ancestor), [x for x in through_ancestor if x not in have]
    for m in (M1, M2, M3, M4, M5, M6):
        assert (m, LARGE) in have and (LARGE, m) in have, m
    assert {x for x in have if OUT in x} == {(OUT, OUT_REST), (OUT_REST, OUT)}          # adjacent and intersecting, yet unrelated
    if stacked:
        assert (M1, MID) in have and (M5, MID) in have and (M6, MID) not in have
    assert len(pairs) >= 26


CLOSURE_WORLDS = [   # outline, atomic, level of the ancestor, its cell: the camera is farther than 200 units from that cell's origin
    pytest.param(16384, 64, 3, (16, 16, 16), id="atomic64-keys32"),
    pytest.param(16384, 16, 4, (32, 32, 32), id="atomic16-keys64"),
    pytest.param(8192, 16, 4, (16, 16, 16), id="atomic16-keys32"),
    pytest.param(65536, 64, 3, (16, 16, 16), id="atomic64-keys64"),
]


@pytest.mark.parametrize("stacked", [False, True], ids=["one-ancestor", "levels-1-and-3"])
@pytest.mark.parametrize("outline,atomic,level,cell", CLOSURE_WORLDS)
def test_closure_through_a_high_ancestor(R, outline, atomic, level, cell, stacked):
    """sections that are related only through a common ancestor of level >= 3 whose own cell origin is farther than 200 units from
    the camera (it reaches the device's short lists through the region of 200 + 4 sides); with `stacked`, an ancestor of level 1
    sits below it and none at level 2, so the topmost-ancestor search has to skip a missing level.  Then the large entity is
    deleted: the ancestor section goes, and with it every pair between sibling sections."""
    ents, cam, O, _ = closure_world(atomic, level, cell, stacked)
    p, w = build_pair(R, pipeline_ents(R, ents), outline=outline, atomic=atomic)
    levels = sorted({ro.unpack_key(k)[0] for k in w.cells()["keys"]})
    assert levels == ([0, 1, level] if stacked else [0, level])
    cam = camera(R, cam)
    assert np.linalg.norm(np.array(cam.position, np.float64) - O) > 200.0
    pairs = collide_frame(R, p, w, cam, twice=True)
    closure_statements(pairs, stacked)
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (R._capi.CHANGE_DELETE, LARGE, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    check_sections(p, w)
    after = set(collide_frame(R, p, w, cam))
    assert (M6, REST) in after and (OUT, OUT_REST) in after and len(after) >= 4
    assert not any(LARGE in x for x in after) and (M3, REST) not in after and (M4, REST) not in after and (M6, M1) not in after
    assert ((M5, M1) in after) == stacked                             # with the level-1 section left, M1's and M5's sections stay related
    p.close(); w.close()


@pytest.mark.parametrize("outline,atomic,level,cell,n0,tight", [
    (16384, 64, 3, (16, 16, 16), 510, True),      # level-0 run of 510 sections: not a multiple of 4
    (16384, 64, 3, (16, 16, 16), 511, True),      # one below a 512-key chunk
    (16384, 64, 3, (16, 16, 16), 513, True),      # one above
    (16384, 64, 3, (16, 16, 16), 513, False),     # with the spare slots of the default build
    (65536, 64, 3, (16, 16, 16), 511, True),      # the same on the 64-bit keys
    (65536, 64, 3, (16, 16, 16), 513, True),
    (16384, 16, 4, (32, 32, 32), 510, False),
], ids=lambda v: str(v))
def test_section_counts_around_the_key_chunks(R, outline, atomic, level, cell, n0, tight):
    """closure_world with filler sections, so that the level-0 run of the section table ends just below or above a 512-key chunk
    (the chunk carries the level of the compact keys, the run is padded to whole chunks with padding keys); then the entities of
    every fifth filler section are deleted, which leaves spare slots inside the run, and the large entity last."""
    ents, cam, O, fillers = closure_world(atomic, level, cell, True, level0_sections=n0)
    p, w = build_pair(R, pipeline_ents(R, ents), outline=outline, atomic=atomic, flags=R._capi.CFG_TIGHT_SLACK if tight else 0)
    keys = w.cells()["keys"]
    assert sum(1 for k in keys if ro.unpack_key(k)[0] == 0) == n0
    cam = camera(R, cam)
    pairs = collide_frame(R, p, w, cam, twice=True)
    closure_statements(pairs, True)
    assert sum(1 for a, b in pairs if a >= FILLER0) >= 4              # the filler mover in front of the camera meets its section's entity at rest and LARGE
    gone = [i for k, ids in enumerate(fillers) if k % 5 == 0 for i in ids]
    ch = np.zeros(len(gone), R.CHANGE_DT)
    for k, i in enumerate(gone):
        ch[k] = (R._capi.CHANGE_DELETE, i, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    check_sections(p, w)
    assert sum(1 for k in w.cells()["keys"] if ro.unpack_key(k)[0] == 0) < n0          # whole sections went
    pairs = collide_frame(R, p, w, cam, twice=True)
    closure_statements(pairs, True)
    ch = np.zeros(1, R.CHANGE_DT); ch[0] = (R._capi.CHANGE_DELETE, LARGE, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    after = collide_frame(R, p, w, cam)
    assert (M6, REST) in after and (M3, REST) not in after and len(after) >= 4
    p.close(); w.close()


# ------------------------------------------------------------------------------------------------------------------------------
# e. the moved-entity predicate (k_col_moved), one small world each
# ------------------------------------------------------------------------------------------------------------------------------
NEAR_CAM = ((8210, 8210, 8290), (0, 0, -1), 1000.0)


def test_always_execute_mover_in_a_section_out_of_view(R):
    """a mover behind the camera, in a section that is not visible but within 200 units: with AlwaysExecuteLogic it is processed
    (find_always_execute_entities, logic_flow.rs:803-836), once; without the flag it is not"""
    for flag, want in ((ro.F_ALWAYS_EXEC, [(1, 2), (2, 1)]), (0, [])):
        ents = [cases.ent(1, (8210, 8210, 8410), 5.0, MV | flag, (1, 0, 0)), cases.ent(2, (8213, 8210, 8410), 2.0, 0)]
        p, w = build_pair(R, pipeline_ents(R, ents))
        got = collide_frame(R, p, w, camera(R, NEAR_CAM))
        assert listed(p)(ro.pack_key(0, 8210 // 64, 8410 // 64, 8210 // 64)) == 0
        assert got == want and len(got) == (2 if flag else 0)
        p.close(); w.close()


def test_static_mover_is_not_a_moved_entity(R):
    """a static entity with Velocity and CanCauseCollisions lives in static_entities: update_positions never sees it, and
    find_related_entities does not return it.  The non-static mover 3 next to it meets the entity at rest only."""
    ents = [cases.ent(1, (8210, 8210, 8210), 5.0, MV | ro.F_STATIC, (1, 0, 0)), cases.ent(2, (8214, 8210, 8210), 2.0, 0),
            cases.ent(3, (8214, 8212, 8210), 2.0, MV, (0, 1, 0))]
    p, w = build_pair(R, pipeline_ents(R, ents))
    got = collide_frame(R, p, w, camera(R, NEAR_CAM))
    times = listed(p)(ro.pack_key(0, 128, 128, 128))
    assert times >= 1 and got == sorted([(3, 2), (2, 3)] * times)
    p.close(); w.close()


def test_shared_mover_behind_static_and_unseen_linking_sections(R):
    """movers 30 and 31 straddle y = 8256: the shared section of a = (128,128,128) and b = (128,128,129) [x, z, y].  A static
    entity straddling x = 8256 makes a second shared section on a, later in the canonical order and without active members, so a
    is a static world section although it links 30's.  Camera 1 looks away with a inside the logic box and b outside: a is
    visible but static, b is not visible, and update_positions reaches neither 30 nor 31 -- 31's AlwaysExecuteLogic does not count
    either, one of its sections being visible.  The unique mover 40 still meets 41.  Camera 2 sees b: 30 creates both entries, 31
    is pushed into both and meets 30 from each.  Camera 3 sees neither section: 31 alone is processed (always execute), is the
    first to touch both sections and meets nobody."""
    ents = [cases.ent(30, (8224, 8256, 8224), 4.0, MV, (1, 0, 0)), cases.ent(31, (8226, 8256, 8224), 3.0, MV | ro.F_ALWAYS_EXEC, (0, 0, 1)),
            cases.ent(35, (8256, 8224, 8224), 4.0, ro.F_STATIC),
            cases.ent(40, (8224, 8200, 8340), 5.0, MV, (1, 0, 0)), cases.ent(41, (8227, 8200, 8340), 2.0, 0)]
    p, w = build_pair(R, pipeline_ents(R, ents))
    a, b = ro.pack_key(0, 128, 128, 128), ro.pack_key(0, 128, 128, 129)
    cells = w.cells(); st = {int(k): int(s) for k, s in zip(cells["keys"], cells["is_static_section"])}
    assert st[a] == 1 and st[b] == 0
    got = collide_frame(R, p, w, R.Camera((8224, 8200, 8300), (0, 0, 1), 1000.0))
    times = listed(p)
    assert times(a) >= 1 and times(b) == 0
    assert got == sorted([(40, 41), (41, 40)] * times(ro.pack_key(0, 128, 8340 // 64, 128))) and len(got) >= 2
    got = collide_frame(R, p, w, R.Camera((8224, 8290, 8300), (0, 0, -1), 1000.0))
    assert listed(p)(b) >= 1
    assert Counter(got)[(31, 30)] == 2 and not any(x[0] == 30 for x in got)
    got = collide_frame(R, p, w, R.Camera((8224, 8200, 8420), (0, 0, 1), 1000.0))
    assert listed(p)(a) == 0 and listed(p)(b) == 0
    assert not any(x[0] in (30, 31) for x in got)
    p.close(); w.close()


def test_user_entity_under_a_shared_lookup(R):
    """the user entity always causes collisions and comes last (logic_flow.rs:236-240).  Here it straddles x = 8256: mover 1, in the
    left section, created that section's entry, so the user is pushed into it and meets 1 and 2 there; the right section's entry
    the user creates itself and is not pushed into it, so 3, which lives there and lies inside the user's box, is not met"""
    U = 900
    ents = [cases.ent(1, (8246, 8210, 8210), 4.0, MV, (1, 0, 0)), cases.ent(2, (8250, 8212, 8210), 2.0, 0),
            cases.ent(3, (8262, 8210, 8210), 2.0, 0), cases.ent(U, (8256, 8210, 8210), 6.0, ro.F_USER)]
    p, w = build_pair(R, pipeline_ents(R, ents))
    assert w.lookup(U)[0] == 2
    got = collide_frame(R, p, w, camera(R, NEAR_CAM))
    c = Counter(got)
    assert c[(U, 1)] == 1 and c[(U, 2)] == 1 and c[(2, U)] == 1 and c[(U, 3)] == 0 and c[(3, U)] == 0
    assert c[(1, U)] >= 1 and c[(1, 2)] >= 1 and len(got) >= 5
    p.close(); w.close()


def test_deleted_mover_and_deleted_partner(R):
    """DeleteRequest of a mover (its pairs go) and of an entity at rest (the pairs with it go); the rows stay, marked dead"""
    ents = [cases.ent(1, (8210, 8210, 8210), 5.0, MV, (1, 0, 0)), cases.ent(2, (8214, 8210, 8210), 2.0, 0),
            cases.ent(3, (8230, 8230, 8210), 5.0, MV, (0, 1, 0)), cases.ent(4, (8234, 8230, 8210), 2.0, 0), cases.ent(5, (8230, 8234, 8210), 2.0, 0)]
    p, w = build_pair(R, pipeline_ents(R, ents))
    cam = camera(R, NEAR_CAM)
    got = collide_frame(R, p, w, cam)
    t = listed(p)(ro.pack_key(0, 128, 128, 128))
    assert t >= 1 and got == sorted([(1, 2), (2, 1), (3, 4), (4, 3), (3, 5), (5, 3)] * t)
    ch = np.zeros(2, R.CHANGE_DT)
    ch[0] = (R._capi.CHANGE_DELETE, 1, 0, 0, (0, 0, 0, 0)); ch[1] = (R._capi.CHANGE_DELETE, 4, 0, 0, (0, 0, 0, 0))
    w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    got = collide_frame(R, p, w, cam, twice=True)
    assert got == sorted([(3, 5), (5, 3)] * t) and len(got) >= 2
    p.close(); w.close()


# ------------------------------------------------------------------------------------------------------------------------------
# f. scratch lifecycle: the scratch of re_collide is sized by the row and dynamic-slot CAPACITIES, which grow with slack, so rows
# and dynamic slots added inside the slack after a first collide are covered
# ------------------------------------------------------------------------------------------------------------------------------
def rest_block(n_side=6, centre=(8210.0, 8210.0, 8210.0), step=7.0, half=4.0, first_id=1, flags=0):
    """n_side^3 overlapping entities at rest around the camera's section"""
    e = []
    for k in range(n_side ** 3):
        x, y, z = k % n_side, (k // n_side) % n_side, k // (n_side * n_side)
        e.append(cases.ent(first_id + k, (centre[0] + (x - n_side / 2) * step, centre[1] + (y - n_side / 2) * step, centre[2] + (z - n_side / 2) * step), half, flags))
    return e


def movers(n, first_id, seed):
    rng = np.random.default_rng(seed)
    return [cases.ent(first_id + k, tuple(np.float32(8210.0) + rng.uniform(-18, 18, 3).astype(f32)), 3.0, MV, tuple(rng.uniform(-30, 30, 3).astype(f32))) for k in range(n)]


@pytest.mark.parametrize("via", ["re_add_entities", "RE_CHANGE_ADD_ENTITY"])
def test_movers_added_after_the_first_collide(R, via):
    """a world uploaded without movers; one mover added (rows and dynamic slots grow, with slack); a frame with collide (the scratch
    is sized); 30 more movers added near the camera (they fit the slack: nothing is re-sized); then frames with collide and
    ticks.  Sized by the counts in use, the scratch of the second collide was one mover's: the moved flags of the new rows lay
    beyond the allocation and the 31 (section, moved entity) entries exceeded a list of 16 (RE_E_CAPACITY)."""
    p, w = build_pair(R, pipeline_ents(R, rest_block()))
    cam = camera(R, NEAR_CAM)
    assert collide_frame(R, p, w, cam) == []                           # no mover, no pair; nothing is sized by this call's counts either way
    tick_both(p, w, cam)
    one = pipeline_ents(R, movers(1, 5000, 1))
    assert p.register_model_instances(one) == w.register(to_oracle(one)) == 0
    assert len(collide_frame(R, p, w, cam, twice=True)) >= 2
    tick_both(p, w, cam)
    more = pipeline_ents(R, movers(30, 6000, 2))
    if via == "re_add_entities":
        assert p.register_model_instances(more) == w.register(to_oracle(more)) == 0
    else:
        ch = np.zeros(len(more), R.CHANGE_DT)
        for i in range(len(more)):
            ch[i] = (R._capi.CHANGE_ADD_ENTITY, int(more["id"][i]), 0, i, (0, 0, 0, 0))
        w.apply_changes(ch.view(ro.CHANGE_DT), added=to_oracle(more)); p.apply_changes(ch, added=more)
    assert p.stats()["n_entities"] == 6 ** 3 + 31 and p.stats()["n_dynamic"] == 31
    total = 0
    for f in range(6):
        total += len(collide_frame(R, p, w, cam, twice=True))
        tick_both(p, w, cam)
    assert total >= 6 * 60
    p.close(); w.close()


def test_velocity_written_to_entities_registered_without_one(R):
    """Velocity written through change requests to entities registered without one takes dynamic slots without adding rows: one
    entity first (the dynamic table grows, with slack), a frame with collide (the scratch is sized), then 24 more (inside the
    slack), then frames with collide and ticks"""
    ents = rest_block(flags=ro.F_CAN_COLLIDE) + movers(1, 5000, 3)
    p, w = build_pair(R, pipeline_ents(R, ents))
    cam = camera(R, NEAR_CAM)
    assert len(collide_frame(R, p, w, cam, twice=True)) >= 2
    tick_both(p, w, cam)
    rng = np.random.default_rng(4)

    def write_velocity(ids):
        ch = np.zeros(len(ids), R.CHANGE_DT)
        for k, i in enumerate(ids):
            ch[k] = (R._capi.CHANGE_MODIFY, i, R._capi.C_VELOCITY, 0, tuple(rng.uniform(-30, 30, 3).astype(f32)) + (0,))
        w.apply_changes(ch.view(ro.CHANGE_DT)); p.apply_changes(ch)
    write_velocity([100])
    assert p.stats()["n_dynamic"] == 2
    assert len(collide_frame(R, p, w, cam, twice=True)) >= 4
    tick_both(p, w, cam)
    write_velocity(list(range(101, 125)))
    assert p.stats()["n_dynamic"] == 26
    total = 0
    for f in range(6):
        total += len(collide_frame(R, p, w, cam, twice=True))
        tick_both(p, w, cam)
    assert total >= 6 * 50
    p.close(); w.close()


# ------------------------------------------------------------------------------------------------------------------------------
# g. the pair buffer
# ------------------------------------------------------------------------------------------------------------------------------
def test_pair_buffer_beyond_the_minimum(R):
    """100 mutually overlapping entities in one section, 70 of them movers: every mover meets the 69 other movers (one call each)
    and the 30 at rest (two calls each), 70 * 129 = 9030 calls per listing of the section -- more than the library's smallest pair
    buffer (4096).  Truncated calls report the true total and fill what fits."""
    rng = np.random.default_rng(7)
    ents = [cases.ent(1 + k, tuple(np.float32(8210.0) + rng.uniform(-2, 2, 3).astype(f32)), 6.0, MV if k < 70 else 0) for k in range(100)]
    p, w = build_pair(R, pipeline_ents(R, ents))
    cam = camera(R, NEAR_CAM)
    check_frame(R, p, w, cam, False)
    times = listed(p)(ro.pack_key(0, 128, 128, 128))
    want = sorted_pairs(w.collide(oracle_camera(cam)))
    assert times >= 1 and len(want) == 9030 * times > 4096
    part, n = p.collide(capacity=16)
    assert n == len(want) and len(part) == 16
    have = Counter(map(tuple, want.tolist()))
    assert all(have[tuple(x)] >= 1 for x in part.tolist())
    none, n = p.collide(capacity=0)                                   # no buffer: the total alone
    assert n == len(want) and len(none) == 0
    full, n = p.collide(capacity=len(want))
    assert n == len(want)
    np.testing.assert_array_equal(sorted_pairs(full), want)
    part, n = p.collide(capacity=5)                                   # a small call after the large one
    assert n == len(want) and len(part) == 5 and all(have[tuple(x)] >= 1 for x in part.tolist())
    full, n = p.collide()
    np.testing.assert_array_equal(sorted_pairs(full), want)
    assert_clean_publication(p)
    p.close(); w.close()
