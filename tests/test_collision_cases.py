"""CPU check of the collision known answers derived from the reference's find_related_entities fixture (collision_cases.py):
the derivation is validated against the oracle's handle_collisions on a machine without a GPU; test_collision_gpu.py then holds
the device to the same written-out expectations."""
import numpy as np
import pytest

import oracle as ro
from render_engine_amd import Camera
from helpers import oracle_camera
import collision_cases as cases

G = cases.GOLDEN


def test_golden_sections_are_the_ones_the_tree_assigns():
    """the section of every golden entity, as read off the golden queries, is where the tree puts the identity-transform entity"""
    w = ro.World(G["outline"], G["atomic"])
    assert w.register(cases.golden_world(0)) == 0
    for e, box in enumerate(cases.GOLDEN_BOXES):
        kind, where = cases.golden_section(e)
        k, keys = w.lookup(e)
        assert (k, tuple(keys) if k == 2 else keys[0]) == ((2, where) if kind == "shared" else (1, where))
        np.testing.assert_array_equal(w.entity(e)["aabb"], np.float32(box))      # StaticAABB == the golden box
    w.close()


@pytest.mark.parametrize("mover", range(len(cases.GOLDEN_BOXES)))
def test_golden_derived_pairs_equal_the_oracle(mover):
    w = ro.World(G["outline"], G["atomic"])
    assert w.register(cases.golden_world(mover)) == 0
    cam = oracle_camera(Camera(*cases.GOLDEN_CAM))
    vis = w.cull(cam)
    kind, where = cases.golden_section(mover)
    for key in (where if kind == "shared" else (where,)):
        assert (vis == key).sum() >= 1, "the mover's section must be listed, or the case is empty for the wrong reason"
    want = cases.golden_expected(mover, lambda key: int((vis == key).sum()))
    got = sorted(map(tuple, w.collide(cam).tolist()))
    assert got == want
    w.close()


def test_golden_expectations_are_not_empty_and_keep_the_face_touch_apart():
    """what the derivation says, stated: movers 0, 1, 2 and 4 each meet their four related partners, the shared mover 3 and the
    unrelated mover 5 meet nobody -- although 5's box [128,138]x[0,10]x[0,10] touches 4's box [0,128]^3 on the face x = 128 and
    so intersects it (closed intervals): their sections are unrelated, no pair in either direction"""
    once = lambda key: 1
    n = [len(cases.golden_expected(m, once)) for m in range(6)]
    assert n == [8, 8, 8, 0, 8, 0]
    big, small = cases.GOLDEN_TOUCHING_UNRELATED
    assert cases.intersects(cases.GOLDEN_BOXES[big], cases.GOLDEN_BOXES[small])
    for m in (big, small):
        ex = cases.golden_expected(m, once)
        assert (big, small) not in ex and (small, big) not in ex
    assert cases.golden_expected(4, once) == sorted([(4, o) for o in (0, 1, 2, 3)] + [(o, 4) for o in (0, 1, 2, 3)])
