"""The ray-traced shadow mask on the CPU: the builder's invariants (csrc/accel_build.cpp through toyrenderer_amd/accel.py), the walk of the
product's node arrays against brute force over every triangle for every texel of every case the GPU tests run (tests/shadow_scenes.py
CASES; zero differing texels allowed: a difference is a box that rejected a triangle the triangle test accepts), brute force against
an analytic shadow, the pieces of the convention, the constant block and the driver's refusals.  No GPU."""
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from suite_support import shadow_case_reference, sm  # noqa: E402, F401
from toyrenderer_amd import accel, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

F = np.float32
INNER = I.kAccelInner


# ---- 1. the builder ---------------------------------------------------------------------------------------------------------------------
def _walk_tree(nodes, leaf_capacity):
    """Checks the preorder / skip-link structure; returns [(node, depth)] of the leaves and the deepest level."""
    n = len(nodes)
    leaves, deepest = [], 0

    def visit(i, depth, end):
        nonlocal deepest
        assert i < n and nodes["skip"][i] == end, (i, int(nodes["skip"][i]), end)
        deepest = max(deepest, depth)
        if nodes["leaf"][i] != INNER:
            assert end == i + 1
            leaves.append(i)
            return
        left = i + 1
        right = int(nodes["skip"][left])
        assert left < right < end
        visit(left, depth + 1, right)
        visit(right, depth + 1, end)
        for c in (left, right):                                            # every box contains its children
            assert np.all(nodes["lo"][i] <= nodes["lo"][c]) and np.all(nodes["hi"][i] >= nodes["hi"][c]), (i, c)
    sys.setrecursionlimit(10000)
    visit(0, 0, n)
    return leaves, deepest


MESHES = {"one triangle": lambda: SS.strip(1), "L": lambda: SS.strip(SS.L), "L+1": lambda: SS.strip(SS.L + 1), "2L+1": lambda: SS.strip(2 * SS.L + 1),
          "degenerate": SS.with_degenerates, "blob 300": lambda: SS.blob(300, 4), "tetrahedron": SS.tetrahedron, "collinear 4096": SS.collinear_growing}


@pytest.mark.parametrize("name", list(MESHES))
def test_blas_invariants(name):
    """Every triangle with finite vertices sits in exactly one leaf, every box contains its triangles and its children, the depth is
    within trhip_accel_max_depth(), a leaf holds 1..L triangles, and a second build gives the same bytes."""
    assert accel.leaf_capacity() == SS.L and accel.max_depth() == 56
    p, idx = MESHES[name]()
    nodes, order, depth = accel.build_blas(p, idx)
    nodes2, order2, depth2 = accel.build_blas(p.copy(), idx.copy())
    assert nodes.tobytes() == nodes2.tobytes() and order.tobytes() == order2.tobytes() and depth == depth2
    tris = idx.reshape(-1, 3)
    finite = np.array([np.all(np.isfinite(p[t])) for t in tris])
    assert sorted(order.tolist()) == np.flatnonzero(finite).tolist()          # each finite triangle once, no other
    leaves, deepest = _walk_tree(nodes, SS.L)
    assert deepest == depth <= accel.max_depth()
    if name == "collinear 4096":
        assert depth <= 24 + 12, depth                                          # 24 heuristic levels, then halving 4096
    seen = []
    for i in leaves:
        first, count = int(nodes["leaf"][i]) & 0x3FFFFFFF, (int(nodes["leaf"][i]) >> 30) + 1
        assert 1 <= count <= SS.L and first + count <= len(order)
        for t in order[first:first + count]:
            v = p[tris[t]]
            assert np.all(nodes["lo"][i] <= v.min(0)) and np.all(nodes["hi"][i] >= v.max(0)), (i, t)
        seen += list(range(first, first + count))
    assert sorted(seen) == list(range(len(order)))                              # the leaves partition the order
    pad = F(2.0 ** -16) * F(np.abs(p[tris[finite]]).max())
    v = p[tris[order]].reshape(-1, 3)
    assert np.all(nodes["lo"][0] <= v.min(0) - pad * F(0.99)) and np.all(nodes["hi"][0] >= v.max(0) + pad * F(0.99))   # the boxes are padded


def test_blas_refusals_and_empty_meshes():
    from toyrenderer_amd import rhi
    p, idx = SS.strip(3)
    with pytest.raises(rhi.TrhipError, match="outside the 5 vertices"):
        accel.build_blas(p, np.array([0, 1, 9], np.uint32))
    with pytest.raises(rhi.TrhipError, match="whole triangles"):
        accel.build_blas(p, np.array([0, 1, 2, 3], np.uint32))
    nodes, order, depth = accel.build_blas(p, np.zeros(0, np.uint32))
    assert len(nodes) == 0 and len(order) == 0 and depth == 0
    q = p.copy(); q[:, 0] = np.nan
    nodes, order, _ = accel.build_blas(q, idx)
    assert len(nodes) == 0 and len(order) == 0                                  # nothing to hit


@pytest.mark.parametrize("n", SS.TLAS_COUNTS)
def test_tlas_invariants(n):
    """Each instance of the two lists sits in exactly one leaf (an instance in neither list in none), the levels list every inner
    node once with children before parents, the depth is within the bound, and a second build gives the same bytes."""
    sc = SS.scattered(n)
    sc["opaqueIds"] = sc["opaqueIds"][sc["opaqueIds"] != 0] if n > 2 else sc["opaqueIds"]         # instance 0 in neither list
    a, b = SR.Accel(sc), SR.Accel(sc)
    for k in ("nodes", "records", "level_nodes", "level_offsets"):
        assert a.tlas[k].tobytes() == b.tlas[k].tobytes(), k
    nodes, rec = a.tlas["nodes"], a.tlas["records"]
    present = np.flatnonzero(a.flags)
    leaves, deepest = _walk_tree(nodes, 1)
    assert deepest <= accel.max_depth() and len(nodes) == 2 * len(present) - 1
    assert sorted(int(nodes["leaf"][i]) for i in leaves) == present.tolist()
    for i in leaves:
        assert rec["leaf_node"][nodes["leaf"][i]] == i
    assert np.all(rec["leaf_node"][a.flags == 0] == INNER) and np.array_equal(rec["flags"], a.flags)
    off, lv, levels = a.tlas["level_offsets"], a.tlas["level_nodes"], a.tlas["num_levels"]
    assert levels <= accel.max_depth() and off[0] == 0 and off[levels] == len(nodes) - len(leaves)
    height = {i: 0 for i in leaves}
    for h in range(1, levels + 1):
        for i in lv[off[h - 1]:off[h]]:
            left, right = int(i) + 1, int(nodes["skip"][int(i) + 1])
            assert nodes["leaf"][i] == INNER and max(height[left], height[right]) == h - 1      # both children done, one in the level before
            height[int(i)] = h
    assert len(height) == len(nodes)


# ---- 2. the walk against brute force -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SS.CASES, ids=lambda c: c[0])
def test_walk_equals_brute_force(sm, case):
    """Every texel: 0 differing.  Far texels keep the mask's sentinel and get 0x7BFF; no other texel keeps a sentinel."""
    sc, acc, k, depth, g, noise, mask, lvd = shadow_case_reference(sm, case)
    got, got_lvd, (boxes, tris) = SR.trace(sm, k, acc, depth, g, noise, SR.WALK)
    far = depth == 0
    print(f"{case[0]}: occluded {int((mask == 0).sum())} of {int((~far).sum())} traced texels, {boxes} box tests, {tris} triangle tests")
    assert int(np.count_nonzero(got != mask)) == 0
    assert np.array_equal(got_lvd, lvd)
    assert np.all(mask[far] == SR.SENTINEL8) and np.all(lvd[far] == 0x7BFF)
    assert np.all(np.isin(mask[~far], (0, 255))) and not np.any(lvd[~far] == SR.SENTINEL16)
    if mask.size > 500 and not case[0].startswith("tlas ") or case[0] in ("tlas 64", "tlas 65", "tlas 257"):
        assert np.any(mask == 0) and np.any(mask == 255), "the case shows both outcomes"
        if len(sc["instances"]) >= 33:                                           # the tree prunes: under a quarter of brute force's triangle tests
            assert tris < (~far).sum() * sum(int(c) // 3 for c in acc.blas["index_counts"][sc["instances"]["m_MeshDataIdx"]]) / 4


def test_refit_follows_moved_instances(sm):
    """Matrices changed after the topology was built, one instance moved far outside its rest box: the walk over the refit arrays
    still equals brute force, the moved leaf's ancestors contain it, and the rest topology is untouched."""
    sc = SS.scattered(65)
    acc = SR.Accel(sc)
    moved = sc["instances"].copy()
    moved["m_WorldMatrix"][5] = SS.world_matrix(scale=(6.0, 0.3, 8.0), position=(0.5, 40.0, -6.0))          # a roof far above the rest box
    moved["m_WorldMatrix"][9] = SS.world_matrix(scale=(1, 1, 1), axis=(1, 0, 0), angle=1.0, position=(2.0, 2.5, -5.0))
    W, H = 67, 35
    k = SS.consts(W, H, SS.LIGHTS["up"], False, 0)
    depth, g = SS.images(W, H, 21)
    noise = SS.noise_image()
    rest, _, _ = SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE)
    brute, _, _ = SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE, instances=moved)
    walk, _, _ = SR.trace(sm, k, acc, depth, g, noise, SR.WALK, instances=moved)
    assert np.count_nonzero(brute != rest) > 100                                                           # the roof shadows what was lit
    assert np.count_nonzero(walk != brute) == 0
    nodes, rec = SR.refit(sm, acc, moved)
    assert np.array_equal(nodes["skip"], acc.tlas["nodes"]["skip"]) and np.array_equal(nodes["leaf"], acc.tlas["nodes"]["leaf"])
    leaf = int(rec["leaf_node"][5])
    assert nodes["hi"][leaf][1] > 39.0 and nodes["hi"][0][1] >= nodes["hi"][leaf][1] and acc.tlas["nodes"]["hi"][0][1] < 20.0
    _walk_tree(nodes, 1)                                                                                   # every box contains its children


# ---- 3. brute force against geometry -------------------------------------------------------------------------------------------------------
def test_brute_force_matches_an_analytic_shadow(sm):
    """One quad above a floor, hard shadows, the light straight up and oblique: a texel is occluded iff its ray meets the quad's plane
    inside the quad, for every texel whose ray passes farther than 1e-3 of the quad's size from the outline; those left out stay
    under 5 %."""
    half, height = 1.5, 2.0
    sc = SS.make_scene([SS.quad(half)], [(0, SS.world_matrix(position=(0.3, height, -5.0)), 0, "opaque")])
    acc = SR.Accel(sc)
    W, H = 96, 54
    v = synth.make_view(eye=SS.EYE, render=(W, H))
    # depth of the floor y = 0 under every pixel (float64), far where the view ray does not reach it
    c2w = I.clip_to_world(v.worldToView, v.viewToClip).astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    cx, cy = (xs + 0.5) / W * 2 - 1, (ys + 0.5) / H * -2 + 1
    depth = np.zeros((H, W), F)
    for d in np.geomspace(1e-3, 0.2, 4000):                                     # pick, per pixel, the depth whose world position is nearest y = 0
        h = cx[..., None] * c2w[0] + cy[..., None] * c2w[1] + d * c2w[2] + c2w[3]
        y = h[..., 1] / h[..., 3]
        better = (np.abs(y) < 0.02) & (depth == 0)
        depth[better] = d
    assert np.count_nonzero(depth) > 0.3 * W * H
    g = np.zeros((H, W, 4), np.uint32)
    g[..., 1] = 0x7FFF | 0xFFFF << 16                                           # a normal close to +y
    noise = SS.noise_image()
    for light in ((0.0, 1.0, 0.0), SS.unit((0.4, 1.0, -0.3))):
        k = SS.consts(W, H, light, False, 0, ray_start_offset=0.01)
        mask, _, _ = SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE)
        valid, o, d, _ = SR.texel_rays(sm, k, depth, g, noise)
        o, d = o.astype(np.float64), d.astype(np.float64)
        with np.errstate(all="ignore"):                                        # far texels have no ray: 0 / 0, masked by `valid`
            t = (height - o[..., 1]) / d[..., 1]
            qx, qz = o[..., 0] + t * d[..., 0] - 0.3, o[..., 2] + t * d[..., 2] + 5.0
        inside = (np.abs(qx) < half) & (np.abs(qz) < half) & (t > 0.01)
        margin = 1e-3 * 2 * half
        near_outline = np.abs(np.maximum(np.abs(qx), np.abs(qz)) - half) < margin       # the shared diagonal is no outline: the test is watertight
        judged = valid & ~near_outline
        assert np.count_nonzero(valid & near_outline) < 0.05 * np.count_nonzero(valid)
        assert np.array_equal(mask[judged] == 0, inside[judged])
        assert 50 < np.count_nonzero(inside & judged) < np.count_nonzero(judged) - 50


def test_a_shared_edge_does_not_leak(sm):
    """A roof of two triangles over everything, hard shadows, from above and obliquely: every texel is occluded, also those whose
    ray passes through the diagonal the two triangles share."""
    W, H = 64, 64
    sc = SS.make_scene([SS.quad(1.0)], [(0, SS.world_matrix(scale=(60.0, 1.0, 60.0), axis=(0, 1, 0), angle=0.3, position=(0.0, 30.0, 0.0)), 0, "opaque")])
    acc = SR.Accel(sc)
    depth, g = SS.images(W, H, 3, far_share=0.0)
    for light in ((0.0, 1.0, 0.0), SS.unit((0.3, 1.0, 0.2)), SS.unit((-0.2, 1.0, -0.4))):
        k = SS.consts(W, H, light, False, 0, ray_start_offset=0.0)
        mask, _, _ = SR.trace(sm, k, acc, depth, g, SS.noise_image(), SR.BRUTE)
        assert np.all(mask[depth != 0] == 0)


# ---- 4. pieces of the convention --------------------------------------------------------------------------------------------------------------
def test_half_rounding(sm):
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(0, 70000, 20000), 2.0 ** rng.uniform(-30, 17, 20000), [0.0, 65504.0, 65519.99, 65520.0, 65536.0, 1e10, np.inf, 2.0 ** -24, 2.0 ** -25,
                        2.0 ** -25 * 1.0001, 6.1e-5, 6.097e-5]]).astype(F)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    got = np.array([sm.sm_half_bits(float(v)) for v in x], np.uint16)
    assert np.array_equal(got, want)
    assert sm.sm_half_bits(float("nan")) == 0x7E00 and sm.sm_half_bits(-float("nan")) == 0x7E00


def test_object_from_world_inverts(sm):
    rng = np.random.default_rng(6)
    for i in range(200):
        scale = rng.uniform(0.2, 5.0, 3) * (1 if i % 3 else -1)
        Wm = SS.world_matrix(scale=scale, axis=rng.normal(size=3), angle=rng.uniform(0, 6.28), position=rng.uniform(-50, 50, 3))
        out = np.zeros(12, F)
        sm.sm_object_from_world(np.ascontiguousarray(Wm).ctypes.data, out.ctypes.data)
        M = np.eye(4)
        M[:, :3] = out.reshape(4, 3)
        assert np.allclose(Wm.astype(np.float64) @ M, np.eye(4), atol=2e-4), i


# ---- 5. the constant block, the settings and the driver's refusals ----------------------------------------------------------------------------
def test_consts_layout_and_values():
    dt = I.ShadowMaskConsts
    assert dt.itemsize == 112
    assert [dt.fields[n][1] for n in ("m_ClipToWorld", "m_DirectionalLightDirection", "m_NoisePhase", "m_CameraPosition", "m_TanSunAngularRadius", "m_OutputResolution",
                                      "m_bDoDenoising", "m_RayStartOffset")] == [0, 64, 76, 80, 92, 96, 104, 108]
    assert I.AccelNode.itemsize == 32 and I.BLASHeader.itemsize == 16 and I.TLASInstance.itemsize == 64 and I.RefitTLASConstants.itemsize == 12
    s = accel.check_settings(dict(noise=SS.noise_image()))
    assert s["soft"] is True and s["sun_angular_diameter"] == 0.533 and s["ray_start_offset"] == 0.1
    k = accel.shadow_consts(np.eye(4, dtype=F), (0.0, -1.0, 0.0), (1.0, 2.0, 3.0), 67, 35, s, 0x1FE)
    assert k["m_NoisePhase"][0] == F(0xFE) * F(1.61803398875) and k["m_bDoDenoising"][0] == 0
    assert k["m_TanSunAngularRadius"][0] == F(math.tan(math.radians(float(F(0.533)) / 2.0)))
    assert abs(float(k["m_TanSunAngularRadius"][0]) - 0.004651) < 1e-6
    assert tuple(k["m_OutputResolution"][0]) == (67, 35) and k["m_RayStartOffset"][0] == F(0.1)
    assert accel.shadow_consts(np.eye(4, dtype=F), (0, -1, 0), (0, 0, 0), 1, 1, {**s, "soft": False}, 256)["m_TanSunAngularRadius"][0] == 0
    assert accel.shadow_consts(np.eye(4, dtype=F), (0, -1, 0), (0, 0, 0), 1, 1, s, 256)["m_NoisePhase"][0] == 0
    words = accel.noise_words(SS.noise_image())
    assert words.shape == (128, 128) and words[0, 2] == 0 | 255 << 8 | int(SS.noise_image()[0, 2, 2]) << 16 | int(SS.noise_image()[0, 2, 3]) << 24


def test_settings_and_driver_refusals():
    from toyrenderer_amd.frame import FrameDriver
    noise = SS.noise_image()
    for bad, match in ((dict(), "noise"), (dict(noise=noise[:64]), "needs uint8"), (dict(noise=noise.astype(np.float32)), "needs uint8"),
                       (dict(noise=noise, sun_angular_diameter=-1.0), "sun_angular_diameter"), (dict(noise=noise, sun_angular_diameter=float("nan")), "sun_angular_diameter"),
                       (dict(noise=noise, ray_start_offset=-0.1), "ray_start_offset"), (dict(noise=noise, ray_start_offset=float("inf")), "ray_start_offset"),
                       (dict(noise=noise, denoise=True), "unknown setting"), ([noise], "dict")):
        with pytest.raises(ValueError, match=match):
            accel.check_settings(bad)
    view = synth.make_view(render=(64, 32))
    scene = types.SimpleNamespace(materials=object(), rt=None, numInstances=1)
    ok = dict(noise=noise)
    with pytest.raises(ValueError, match="needs gbuffer=True"):
        FrameDriver(None, scene, view, record_capacity=16, visibility=True, shadows=ok)
    with pytest.raises(ValueError, match="set_raytracing"):
        FrameDriver(None, scene, view, record_capacity=16, lighting=True, shadows=ok)
    scene.rt = {}
    with pytest.raises(ValueError, match="external shadow_mask"):
        FrameDriver(None, scene, view, record_capacity=16, lighting=True, shadows=ok, shadow_mask=object())
    with pytest.raises(ValueError, match="noise"):
        FrameDriver(None, scene, view, record_capacity=16, gbuffer=True, shadows={})


def test_registry_and_abi_list_the_feature():
    from toyrenderer_amd import rhi
    names = set(rhi.shader_names())
    assert "shadowmask_CS_ShadowMask" in names and "raytracing_CS_RefitTLAS" in names
    for n in ("trhip_blas_build", "trhip_tlas_build", "trhip_accel_max_depth", "trhip_blas_leaf_capacity", "trhip_accel_max_nodes"):
        assert n in rhi.ABI_SYMBOLS and hasattr(rhi.load(), n)
    assert rhi.load().trhip_abi_version() == 1
