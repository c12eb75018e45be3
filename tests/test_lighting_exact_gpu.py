"""GPU: K5 (k_deferred_lighting) over whole images against the float64 reference of tests/lighting_ref.py -- full size, odd shapes, the radius
boundary, lights on a pixel, special radii, the list and slab edges, the other configurations and the from-world path.  Every unmasked channel is
within TOL of the reference; a channel within DELTA of the default-diffuse cutoff is within TOL of one of its two branch values."""
import numpy as np
import pytest

import lighting_ref as LR

TOL = 1e-4


def run_k5(pos, nrm, alb, L, w, h, max_spot=None, max_point=16):
    from render_engine_amd import lighting
    dl = lighting.DeferredLighting(w, h, max_spot_lights=max_spot or max(int(L["n_spot"]), 1), max_point_lights=max_point)
    try:
        dl.upload_gbuffer(pos, nrm, alb); dl.set_lights(L)
        dl.run()
        return dl.read()
    finally:
        dl.close()


def check(pos, nrm, alb, L, w, h, grid=True, **kw):
    got = run_k5(pos, nrm, alb, L, w, h, **kw)
    ref = LR.reference(pos, nrm, alb, L, grid=(w, h) if grid else None)
    LR.compare(got, ref, TOL)
    return got, ref


@pytest.mark.gpu
def test_full_size_against_float64():
    """configs[4] (4096 x 4096, 4096 radius-40 lights) over the whole image"""
    from render_engine_amd import lighting
    w = h = 4096
    pos, nrm, alb = lighting.synthetic_gbuffer(w, h)
    L = lighting.synthetic_lights(n_spot=4096, n_point=0)
    got = run_k5(pos, nrm, alb, L, w, h)
    ref = LR.reference(pos, nrm, alb, L, grid=(w, h))
    e_un, e_m, nm = LR.compare(got, ref, TOL)
    assert nm < 1e-3 * ref.mask.size, nm                               # the mask cannot excuse a broken image
    print(f"K5 vs float64 at 4096x4096x4096: max error {e_un:.3g} over the unmasked channels, {nm} channels masked "
          f"({nm / ref.mask.size:.2e}), masked max distance to a branch {e_m:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (31, 15), (33, 17), (1000, 999)])
def test_shapes_that_are_not_whole_tiles(w, h):
    from render_engine_amd import lighting
    patch = 0.5 * max(w, h) + 100.0
    pos, nrm, alb = lighting.synthetic_gbuffer(w, h, patch=patch)
    L = LR._lights(600 if w * h > 10000 else 200, n_point=2, scale=0.1, patch=patch, radius=40.0)
    check(pos, nrm, alb, L, w, h)


@pytest.mark.gpu
def test_radius_boundary_is_the_oracles():
    """pixels within an ulp or two of their light's radius, where the fused d2 and the oracle's unfused one fall on different sides: the GPU's
    membership is the oracle's predicate for every one of them (plus 3-4-5 distances on the boundary and 1 ulp either side)"""
    pos, nrm, alb, L, member = LR.boundary_scene()
    got = run_k5(pos, nrm, alb, L, 16, 8)
    Lin = dict(L); Lin["spot_radius"] = L["spot_radius"] * np.float32(1.01)
    Lout = dict(L); Lout["spot_radius"] = L["spot_radius"] * np.float32(0.99)
    lit, unlit = LR.reference(pos, nrm, alb, Lin).final, LR.reference(pos, nrm, alb, Lout).final
    gpu_member = np.abs(got[:, :3] - lit).max(axis=1) < np.abs(got[:, :3] - unlit).max(axis=1)
    wrong = np.flatnonzero(gpu_member != member)
    assert len(wrong) == 0, f"{len(wrong)} of {len(member)} pixels decided against the oracle's predicate: {wrong[:16]}"
    LR.compare(got, LR.reference(pos, nrm, alb, L), TOL)


@pytest.mark.gpu
def test_light_on_a_pixel():
    """radius lights (radii 10, 0, -0) and a cone light on pixels' exact positions (d2 == 0): those pixels get the oracle's ambient term and
    their neighbours are as the reference has them"""
    pos, nrm, alb, L, on = LR.zero_distance_scene()
    got, ref = check(pos, nrm, alb, L, 64, 48)
    for p in on:
        nb = [p + dy * 64 + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        np.testing.assert_allclose(got[nb, :3], ref.final[nb], atol=TOL, rtol=0)
        assert got[p, :3].min() > 0.05


@pytest.mark.gpu
def test_special_radii():
    """NaN (lights every pixel), +inf, -inf, 0, -0 and negative radii among ordinary lights"""
    pos, nrm, alb, L = LR.radii_scene(n_point=2)
    check(pos, nrm, alb, L, 96, 64)


LIST_CASES = [(k, lay) for lay in ("plain", "mixed") for k in (128, 129, 256, 257, 384, 385, 1100)] + [(383, "fill"), (384, "fill"), (385, "fill")]


@pytest.mark.gpu
@pytest.mark.parametrize("k,layout", LIST_CASES)
def test_listed_light_counts(k, layout):
    """listed-light counts per tile around the flush threshold (n + 256 > LIST_CAP) and its multiples, the list filled to exactly LIST_CAP,
    and far beyond; the host model of the tile's cull confirms that the tile lists all k lights"""
    pos, nrm, alb, L = LR.list_scene(k, layout)
    flushes, listed = LR.k5_list_flushes(pos, 32, 16, L)
    assert sum(flushes) == k and max(flushes) <= LR.LIST_CAP, flushes
    if layout == "fill":
        assert flushes == {383: [383], 384: [384], 385: [129, 256]}[k], flushes
    check(pos, nrm, alb, L, 32, 16)


@pytest.mark.gpu
def test_nan_radius_slab_reach():
    """NaN radii among finite ones and no infinite one: the tiles far along the slab axis from a NaN light reach its slab only through the
    NaN-aware largest radius of re_lighting_set_lights"""
    pos, nrm, alb, L = LR.nan_reach_scene()
    assert not np.isinf(L["spot_radius"]).any()
    check(pos, nrm, alb, L, 128, 32)


@pytest.mark.gpu
def test_lights_on_slab_boundaries():
    """the lights' x extent is 64 (inv_w = 64 exactly) and every light sits on a slab boundary, the pixels on integer x, radii integers"""
    from render_engine_amd import lighting
    rng = np.random.default_rng(6)
    pos, nrm, alb = lighting.synthetic_gbuffer(64, 32, patch=64.0, origin=(999.5, 1000.0, 999.5))
    n = 800
    L = LR._lights(n, scale=0.1, patch=64.0, radius=4.0)
    kx = rng.integers(0, 4097, n); kx[0] = 0; kx[1] = 4096
    L["spot_pos"][:, 0] = (1000.0 + kx / 64.0).astype(np.float32)
    L["spot_pos"][:, 1] = 1004.0; L["spot_pos"][:, 2] = rng.integers(1000, 1064, n).astype(np.float32)
    L["spot_radius"] = rng.integers(1, 7, n).astype(np.float32)
    check(pos, nrm, alb, L, 64, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one_point", "tiny_extent"])
def test_degenerate_slabs(case):
    """every light at one coordinate (no extent: inv_w = 0, one slab), and an extent too small to divide by (4096 / 1e-37 overflows)"""
    from render_engine_amd import lighting
    rng = np.random.default_rng(7)
    if case == "one_point":
        pos, nrm, alb = lighting.synthetic_gbuffer(64, 32, patch=64.0)
        L = LR._lights(100, scale=0.02, patch=64.0)
        L["spot_pos"][:] = (1030.0, 1010.0, 1020.0); L["spot_radius"] = rng.uniform(5.0, 40.0, 100).astype(np.float32); L["spot_radius"][:3] = 0.0
    else:
        pos, nrm, alb = lighting.synthetic_gbuffer(48, 32, patch=48.0, origin=(-24.0, 0.0, -24.0))
        L = LR._lights(50, scale=0.05, patch=48.0)
        L["spot_pos"][:] = (0.0, 5.0, 0.0); L["spot_pos"][::2, 0] = np.float32(1e-37)
        L["spot_radius"] = rng.uniform(10.0, 30.0, 50).astype(np.float32)
        L["camera_pos"] = np.array([0.0, 300.0, 0.0], np.float32)
    check(pos, nrm, alb, L, pos.shape[0] // 32, 32)


@pytest.mark.gpu
def test_shuffled_pixels():
    """a G-buffer whose pixels are shuffled: every tile's AABB spans the scene"""
    from render_engine_amd import lighting
    w, h = 128, 64
    pos, nrm, alb = lighting.synthetic_gbuffer(w, h, patch=128.0)
    L = lighting.synthetic_lights(n_spot=300, n_point=0, patch=128.0, radius=12.0)
    perm = np.random.default_rng(8).permutation(w * h)
    got = run_k5(pos[perm], nrm[perm], alb[perm], L, w, h)
    LR.compare(got, LR.reference(pos, nrm, alb, L, grid=(w, h)).permuted(perm), TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["none_visible", "cones_only", "full_slots"])
def test_other_configurations(case):
    from render_engine_amd import lighting
    if case == "none_visible":
        w, h = 37, 23
        pos, nrm, alb = lighting.synthetic_gbuffer(w, h, patch=60.0)
        L = lighting.synthetic_lights(n_spot=30, n_point=2, patch=60.0, radius=20.0); L["any_light_source_visible"] = 0
        check(pos, nrm, alb, L, w, h)
    elif case == "cones_only":
        w, h = 45, 29
        pos, nrm, alb = lighting.synthetic_gbuffer(w, h, patch=60.0)
        L = lighting.synthetic_lights(n_spot=0, n_point=5, patch=60.0)
        check(pos, nrm, alb, L, w, h, max_spot=64)
    else:
        w, h = 64, 48
        pos, nrm, alb = lighting.synthetic_gbuffer(w, h, patch=100.0)
        L = LR._lights(256, scale=0.3, patch=100.0, radius=20.0)
        check(pos, nrm, alb, L, w, h, max_spot=256)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["light_on_a_pixel", "special_radii", "nan_reach"])
def test_from_world_edges(case):
    """the same edge cases through re_lighting_set_lights_from_world, the radii from LightInformation (nan_reach: k_world_commit's slab reach):
    the host-fed image matches the reference, and the from-world one is bit-identical to it"""
    import render_engine_amd as R
    from render_engine_amd import lighting
    if case == "light_on_a_pixel":
        pos, nrm, alb, L, _ = LR.zero_distance_scene(n_point=0); w, h = 64, 48
    elif case == "special_radii":
        pos, nrm, alb, L = LR.radii_scene(); w, h = 96, 64
    else:
        pos, nrm, alb, L = LR.nan_reach_scene(); w, h = 128, 32
    n = int(L["n_spot"])
    ents = np.zeros(n, R.ENTITY_DT)
    ents["id"] = np.arange(n, dtype=np.uint32); ents["flags"] = R.F_LIGHT_SPOT; ents["pos"] = L["spot_pos"]
    ents["original"] = np.array([-0.5, 0.5, -0.5, 0.5, -0.5, 0.5], np.float32); ents["scale"] = 1.0; ents["rot_axis"] = (1.0, 0.0, 0.0)
    p = R.Pipeline(16384, 64)
    A = lighting.DeferredLighting(w, h, max_spot_lights=n, max_point_lights=16)
    B = lighting.DeferredLighting(w, h, max_spot_lights=n, max_point_lights=16)
    try:
        assert p.register_model_instances(ents) == 0
        I = np.zeros(n, R.LIGHT_INFORMATION_DT)
        I["radius"] = L["spot_radius"]; I["diffuse"] = L["spot_diffuse"]; I["specular"] = L["spot_specular"]; I["ambient"] = L["spot_ambient"]
        I["linear"] = L["spot_linear"]; I["quadratic"] = L["spot_quadratic"]
        p.set_light_information(ents["id"], I)
        A.upload_gbuffer(pos, nrm, alb); B.upload_gbuffer(pos, nrm, alb)
        cam = R.Camera(L["camera_pos"], (0.0, 0.0, -1.0), 2048.0)
        r = A.set_lights_from_world(p, cam, 8)
        assert r["n_slots"] == [0, 0, n], r["n_slots"]
        np.testing.assert_array_equal(r["slot_ids"][2], np.arange(n))
        B.set_lights(L)
        A.run(); B.run()
        host = B.read()
        LR.compare(host, LR.reference(pos, nrm, alb, L, grid=(w, h)), TOL)
        np.testing.assert_array_equal(A.read(), host)
    finally:
        A.close(); B.close(); p.close()
