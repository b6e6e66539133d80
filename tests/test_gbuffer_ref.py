"""The test reference of GBufferA (tests/gbuffer_ref.c) pinned by something other than itself, on the CPU: every pack
function against an independent numpy restatement and against its format's definition, the vertex normal against a
float64 evaluation, the cornell fixture's three wall colours, the fused motion against visibility_ref's, the loader's
material table, and the back end's and the facade's declarations."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gbuffer_ref as GR  # noqa: E402
from ref_build import layout_probe  # noqa: E402
from suite_support import cornell_fixture, gr, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from gbuffer_scenes import hostile_materials, wall, with_normals_and_materials  # noqa: E402
from scene_gen import all_meshlets_visible  # noqa: E402
from toyrenderer_amd import gltf_lite, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import city, consts, hostile_soup  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- independent numpy restatements (float32 arrays) ------------------------------------------------------------------
def np_saturate(x):
    return np.fmin(np.fmax(x, F(0)), F(1))


def np_rgba8(c):
    b = (np_saturate(np.asarray(c, F)) * F(255)).astype(np.uint32)
    return b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | b[:, 3] << 24


def np_oct(n):
    n = np.asarray(n, F)
    with np.errstate(all="ignore"):
        l1 = (np.abs(n[:, 0]) + np.abs(n[:, 1])) + np.abs(n[:, 2])
        x, y, z = n[:, 0] / l1, n[:, 1] / l1, n[:, 2] / l1
        wx = (F(1) - np.abs(y)) * np.where(x >= 0, F(1), F(-1))
        wy = (F(1) - np.abs(x)) * np.where(y >= 0, F(1), F(-1))
        up = z >= 0
        ox, oy = np.where(up, x, wx) * F(0.5) + F(0.5), np.where(up, y, wy) * F(0.5) + F(0.5)
        ux = np.rint(np_saturate(ox) * F(65535)).astype(np.uint32)
        uy = np.rint(np_saturate(oy) * F(65535)).astype(np.uint32)
    return ux | uy << 16


def np_r9g9b9e5(c):
    c = np.asarray(c, F)
    kmax, kmin = np.array([0x477F8000], np.uint32).view(F)[0], np.array([0x37800000], np.uint32).view(F)[0]
    c = np.fmin(np.fmax(c, F(0)), kmax)
    mx = np.fmax(np.fmax(kmin, c[:, 0]), np.fmax(c[:, 1], c[:, 2])).astype(F)
    bias_bits = ((mx.view(np.uint32).astype(np.uint64) + 0x07804000) & 0x7F800000).astype(np.uint32)
    bias = bias_bits.view(F)
    rgb = (c + bias[:, None]).astype(F).view(np.uint32).astype(np.uint64)
    e = ((bias_bits.astype(np.uint64) << 4) + 0x10000000) & 0xFFFFFFFF
    w = e | ((rgb[:, 2] << 18) & 0xFFFFFFFF) | ((rgb[:, 1] << 9) & 0xFFFFFFFF) | (rgb[:, 0] & 0x1FF)
    return w.astype(np.uint32)


def _edges():
    k255 = np.arange(256, dtype=np.float64) / 255.0
    k65535 = np.arange(0, 65536, 257, dtype=np.float64) / 65535.0
    below = lambda a: np.nextafter(a.astype(F), F(-1))      # noqa: E731
    return np.concatenate([np.array([0.0, 1.0, -0.0, np.nan, np.inf, -np.inf, -1.0, -0.25, 2.0, 1e30, -1e30], F), k255.astype(F), below(k255),
                           k65535.astype(F), below(k65535)]).astype(F)


def test_pack_rgba8_equals_the_numpy_restatement(gr):
    rng = np.random.default_rng(11)
    e = _edges()
    c = np.concatenate([rng.uniform(-0.25, 1.25, (1_000_000, 4)).astype(F), np.stack([e, e[::-1], np.roll(e, 7), np.roll(e, 13)], 1)])
    assert int(np.count_nonzero(GR.pack_rgba8(gr, c) != np_rgba8(c))) == 0
    assert GR.pack_rgba8(gr, [[1.0, 0.0, 0.0, 0.0]])[0] == 0xFF
    assert GR.pack_rgba8(gr, [[np.nan, np.inf, -np.inf, -0.0]])[0] == 0x0000FF00


def test_pack_oct_equals_the_numpy_restatement(gr):
    rng = np.random.default_rng(12)
    e = _edges()
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [0.0, -0.0, -0.0], [1, 1, -1e-30],
                     [np.nan, 0, 1], [np.inf, 1, 1], [1, 1, 1], [-1, -1, -1]], F)
    n = np.concatenate([rng.normal(size=(1_000_000, 3)).astype(F), np.stack([e, np.roll(e, 5), np.roll(e, 11)], 1), axes])
    assert int(np.count_nonzero(GR.pack_oct(gr, n) != np_oct(n))) == 0
    assert GR.pack_oct(gr, [[0.0, 0.0, 1.0]])[0] == 0x80008000          # rint(0.5 * 65535) = 32768 (half to even)
    assert GR.pack_oct(gr, [[np.nan, np.nan, np.nan]])[0] == 0


def test_pack_r9g9b9e5_equals_the_numpy_restatement(gr):
    rng = np.random.default_rng(13)
    e = _edges()
    mag = np.exp2(rng.uniform(-20.0, np.log2(1e6), (1_000_000, 3))).astype(F)
    mag[::7] *= F(-1)
    extra = np.array([[0, 0, 0], [2.0 ** -20, 0, 0], [1e6, 1e6, 1e6], [65408, 65407.9, 1], [np.nan, 1, 2], [np.inf, -np.inf, 0.5], [-0.0, -1, -2],
                      [255.75, 0.25, 0.125], [511.9, 511.9, 511.9]], F)
    c = np.concatenate([mag, np.stack([e, np.roll(e, 3), np.roll(e, 9)], 1), extra])
    assert int(np.count_nonzero(GR.pack_r9g9b9e5(gr, c) != np_r9g9b9e5(c))) == 0


def test_r9g9b9e5_meets_the_formats_definition(gr):
    """Largest channel in [2^-16, 65408): decoding the word (mantissa * 2^(E - 24), E = bits 27-31) is within half a step
    2^(E - 24) of every input channel; (0, 0, 0) packs to the word 0."""
    rng = np.random.default_rng(14)
    n = 1_000_000
    top = np.exp2(rng.uniform(-16.0, np.log2(65408.0), n))
    c = (top[:, None] * rng.uniform(0.0, 1.0, (n, 3))).astype(np.float64)
    c[np.arange(n), rng.integers(0, 3, n)] = top
    c = c.astype(F)
    mx = c.max(axis=1)
    keep = (mx >= F(2.0 ** -16)) & (mx < F(65408.0))
    c = c[keep]
    w = GR.pack_r9g9b9e5(gr, c)
    step = np.exp2((w >> 27).astype(np.float64) - 24.0)
    err = np.abs(GR.decode_r9g9b9e5(w) - c.astype(np.float64)) / step[:, None]
    print("largest error in steps:", err.max())
    assert err.max() <= 0.5
    assert GR.pack_r9g9b9e5(gr, [[0.0, 0.0, 0.0]])[0] == 0


def test_octahedral_round_trip(gr):
    """2e6 seeded unit vectors: the normalised decode (float64) is within sqrt(18) / 65535 + 2^-20 of the input.  Each stored
    half is off by at most half a step, 1/65535 in [-1, 1]; the implied z moves by at most the sum of the two, so the
    L1-normalised vector moves by at most sqrt(6) / 65535; normalising a vector of length >= 1/sqrt(3) multiplies that by
    at most sqrt(3); 2^-20 for the float32 encode."""
    rng = np.random.default_rng(15)
    n = rng.normal(size=(2_000_000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n32 = n.astype(F)
    back = GR.decode_oct(GR.pack_oct(gr, n32))
    err = np.linalg.norm(back - n32.astype(np.float64) / np.linalg.norm(n32.astype(np.float64), axis=1, keepdims=True), axis=1)
    print("largest round-trip error:", err.max())
    assert err.max() <= np.sqrt(18.0) / 65535.0 + 2.0 ** -20


def test_quick_random_float_and_mesh_lod_bytes(gr):
    seeds = np.concatenate([np.arange(1 << 15, dtype=np.uint32), np.random.default_rng(16).integers(0, 1 << 32, 1 << 15, dtype=np.uint64).astype(np.uint32)])
    want = np.array([((1664525 * int(s) + 1013904223) % (1 << 32) & 0xFFFFFF) / 16777216.0 for s in seeds], np.float64)
    got = GR.quick_random_float(gr, seeds)
    assert len(seeds) == 1 << 16 and np.array_equal(got.astype(np.float64), want)
    lods = np.arange(256, dtype=np.uint32)
    v = GR.mesh_lod_value(gr, lods)
    assert np.array_equal(v, lods.astype(F) / F(255.0))
    rgba = np.zeros((256, 4), F); rgba[:, 3] = v
    assert np.array_equal(GR.pack_rgba8(gr, rgba) >> 24, lods), "every LOD byte lands on itself"


def test_unpack_normal(gr):
    q = np.arange(1024, dtype=np.uint32)
    for shift, comp in ((20, 0), (10, 1), (0, 2)):
        got = GR.unpack_normal(gr, q << shift)
        want = (q.astype(F) / F(1023.0)) * F(2.0) - F(1.0)
        assert np.array_equal(got[:, comp], want)
        others = [c for c in range(3) if c != comp]
        assert np.all(got[:, others] == F(-1.0))
    words = np.random.default_rng(17).integers(0, 1 << 32, 100_000, dtype=np.uint64).astype(np.uint32)
    got = GR.unpack_normal(gr, words)
    want = np.stack([((words >> s) & 0x3FF).astype(F) / F(1023.0) * F(2.0) - F(1.0) for s in (20, 10, 0)], 1)
    assert np.array_equal(got, want)
    assert np.array_equal(GR.unpack_normal(gr, [0x3FFFFFFF, 0, 0xC0000000]), np.array([[1, 1, 1], [-1, -1, -1], [-1, -1, -1]], F))


def test_the_kernels_division_free_unorm10_is_the_quotient():
    """visibility_resolve.hip.h computes q / 1023.0f as x * rc, one residual, one correction (rc = RN(1/1023)): restated here
    with exact fused multiply-adds, equal to the float32 quotient for all 1024 inputs."""
    rc = F(1.0) / F(1023.0)
    assert float(rc).hex() == "0x1.0040100000000p-10"
    for q in range(1024):
        x = F(q)
        q0 = F(x * rc)
        got = I.fmaf(I.fmaf(-q0, F(1023.0), x), rc, q0)
        assert got == F(x / F(1023.0)), q


def _raster(vr, k, sc, v, vid, tri, rec, lst, slot=0):
    H, W = int(k["m_OutputResolution"][0][1]), int(k["m_OutputResolution"][0][0])
    geo = VR.Geometry(sc, v, vid, tri)
    depth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
    VR.raster(vr, k, geo, rec, lst, slot, depth, vis)
    recs = [rec if s == slot else None for s in range(4)]
    lsts = [lst if s == slot else None for s in range(4)]
    return geo, vis, recs, lsts


@pytest.mark.parametrize("word,scale,axis,angle,grid", [(0x2FF7FDFF, (1.0, 2.0, 4.0), (0.3, 1.0, 0.2), 0.5, 1), (0x2FF7FDFF, (1.0, 2.0, 4.0), (0.3, 1.0, 0.2), 0.5, 6),
                                                        (0x0007FDFF, (4.0, 1.0, 1.0), (1.0, 0.0, 0.0), -0.4, 6), (0x3FF00000 | 700, (2.0, 0.5, 1.5), (0.0, 0.2, 1.0), 2.0, 1),
                                                        (123 << 20 | 900 << 10 | 40, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.0, 6)])
def test_wall_normal_is_the_adjugate_transform_of_the_unpacked_word(gr, vr, word, scale, axis, angle, grid):
    """A wall whose four vertices (grid 1; 49 at grid 6) carry one packed normal word, under a rotated instance with non-uniform
    scale of ratio <= 4: every covered texel decodes to normalize(unpack(word) * adj(W)) evaluated in float64 from the same
    10-bit word within 1e-4 (6.6e-5 for the 16-bit output, see the round-trip test; the rest for float32 rounding through an
    adjugate of condition <= 16).  Equal vertex normals make the interpolation a multiple of one vector."""
    sc, v, vid, tri, rec, lst = wall(word, scale, axis, angle, grid)
    k = consts(synth.make_view(render=(320, 200)))
    geo, vis, recs, lsts = _raster(vr, k, sc, v, vid, tri, rec, lst)
    mats = synth.materials(1, 4)
    g, _ = GR.gbuffer(gr, k, geo, recs, lsts, vis, mats)
    cov = vis != 0
    assert cov.sum() > 2000
    u = np.array([(word >> 20) & 0x3FF, (word >> 10) & 0x3FF, word & 0x3FF], np.float64) / 1023.0 * 2.0 - 1.0
    Wm = sc["instances"]["m_WorldMatrix"][0].astype(np.float64)[:3, :3]
    adj = np.stack([np.cross(Wm[1], Wm[2]), np.cross(Wm[2], Wm[0]), np.cross(Wm[0], Wm[1])])
    want = u @ adj
    want /= np.linalg.norm(want)
    err = np.linalg.norm(GR.decode_oct(g[cov][:, 1]) - want, axis=1)
    print("largest normal error:", err.max())
    assert err.max() <= 1e-4
    assert np.all(g[~cov] == 0)
    # the single-vertex entry point agrees with a float64 evaluation too
    n1 = GR.vertex_normal(gr, word, sc["instances"]["m_WorldMatrix"][0]).astype(np.float64)
    assert np.linalg.norm(n1 - want) < 1e-5


def test_cornell_fixture_shows_its_three_walls(gr, vr, oracle):
    """Every covered texel's albedo bytes are floor(c * 255) in float32 of one of the asset's three baseColorFactors
    (tests/golden/cornell_materials.json), z = 0, w = 0xFF, and all three colours occur."""
    with open(os.path.join(ROOT, "tests", "golden", "cornell_materials.json")) as f:
        cm = json.load(f)
    _, s, camera = cornell_fixture()
    assert cm["primitiveMaterial"] == [0, 1, 2] and len(cm["baseColorFactor"]) == 3 and len(s.instances) == 3
    mats = gltf_lite.material_table([{"pbrMetallicRoughness": {"baseColorFactor": c, "metallicFactor": 0}} for c in cm["baseColorFactor"]])
    s.materials, s.primMaterial = mats, np.array(cm["primitiveMaterial"], np.uint32)
    inst = gltf_lite.apply_materials(s)
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    sc = dict(s.as_oracle()); sc["instances"] = inst
    view = gltf_lite.view_of(camera, (320, 180))
    rec, lst = all_meshlets_visible(s)
    k = consts(view)
    geo, vis, recs, lsts = _raster(vr, k, sc, s.vertices, s.meshletVertexIds, s.meshletTriangles, rec, lst)
    g, _ = GR.gbuffer(gr, k, geo, recs, lsts, vis, mats)
    cov = vis != 0
    colours = [tuple(int(x) for x in (np.asarray(c[:3], F) * F(255)).astype(np.uint32)) for c in cm["baseColorFactor"]]
    assert len(set(colours)) == 3
    got = GR.albedo_bytes(g[cov][:, 0])
    counts = [int(np.count_nonzero(np.all(got == np.array(c), axis=1))) for c in colours]
    print("texels per colour:", dict(zip(colours, counts)))
    assert sum(counts) == int(cov.sum()) and all(c > 1000 for c in counts)
    assert np.all(g[cov][:, 0] >> 24 == 0) and np.all(g[cov][:, 2] == 0) and np.all(g[cov][:, 3] == 0xFF)
    # the walls' normals: unit length within the 16-bit encoding (interpolated unit normals of flat walls)
    _, slot, pos, _ = VR.decode(vis[cov])
    owner = rec["m_InstanceConstIdx"][lst[pos] >> 5]
    for p, c in enumerate(colours):
        assert np.all(got[owner == cm["primitiveMaterial"].index(p)] == np.array(c))


def test_fused_motion_equals_visibility_ref_on_the_city(tmp_path, oracle, gr, vr):
    s, sc = city(tmp_path, oracle)
    v, sc, mats = with_normals_and_materials(s, sc)
    cam = s.cameras[0]
    render = (480, 270)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    view = synth.View(synth.world_to_view((0.3, 0.1, -0.2), cam.orientation), synth.world_to_view((0.0, 0.0, 0.0), cam.orientation), P,
                      float(np.float32(cam.znear)), *render)
    rec, lst = all_meshlets_visible(s)
    k = consts(view)
    geo, vis, recs, lsts = _raster(vr, k, sc, v, s.meshletVertexIds, s.meshletTriangles, rec, lst, slot=1)
    g, m = GR.gbuffer(gr, k, geo, recs, lsts, vis, mats, debug_mode=3)
    assert np.array_equal(m.view(np.uint32), VR.motion(vr, k, geo, recs, lsts, vis).view(np.uint32))
    cov = vis != 0
    assert cov.sum() > 0.2 * cov.size and np.count_nonzero(m) > 0.2 * cov.size
    assert len(np.unique(g[cov][:, 1])) > 1000, "seeded vertex normals: the interpolation varies over the screen"
    assert len(np.unique(g[cov][:, 0] >> 24)) > 8, "ColorizeMeshlets: several debug bytes"
    assert np.all(g[~cov] == 0) and np.all(g[cov][:, 3] == 0xFF)


@pytest.mark.parametrize("seed", [0, 1])
def test_fused_motion_equals_visibility_ref_on_a_hostile_soup(gr, vr, seed):
    sc, v, vid, tri, rec, lst = hostile_soup(seed)
    v = v.copy()
    v["m_PackedNormal"] = np.random.default_rng(seed).integers(0, 1 << 32, len(v), dtype=np.uint64).astype(np.uint32)
    k = consts(synth.make_view(render=(320, 200)))
    geo, vis, recs, lsts = _raster(vr, k, sc, v, vid, tri, rec, lst, slot=3)
    g, m = GR.gbuffer(gr, k, geo, recs, lsts, vis, hostile_materials(seed), debug_mode=2)
    assert np.array_equal(m.view(np.uint32), VR.motion(vr, k, geo, recs, lsts, vis).view(np.uint32))
    # out-of-range material indices: those texels keep their initial value in both outputs
    sc2 = dict(sc); sc2["instances"] = sc["instances"].copy(); sc2["instances"]["m_MaterialDataIdx"][1] = 8
    geo2 = VR.Geometry(sc2, v, vid, tri)
    init = np.full(vis.shape + (4,), 0xABCD1234, np.uint32)
    g2, m2 = GR.gbuffer(gr, k, geo2, recs, lsts, vis, hostile_materials(seed), debug_mode=2, gbuffer_init=init)
    _, _, pos, _ = VR.decode(vis)
    second = (vis != 0) & (rec["m_InstanceConstIdx"][lst[pos] >> 5] == 1)
    assert second.any() and np.all(g2[second] == 0xABCD1234) and np.all(m2[second] == 0)
    first = (vis != 0) & ~second
    assert first.any() and np.array_equal(g2[first], g[first]) and np.all(g2[vis == 0] == 0xABCD1234)


# ---- loader ---------------------------------------------------------------------------------------------------------------
def _gltf_with_materials(materials, prim_materials):
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    prims = [{"attributes": {"POSITION": 0}, **({"material": m} if m is not None else {})} for m in prim_materials]
    g = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}], "materials": materials,
         "meshes": [{"primitives": prims}], "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"}],
         "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 36}], "buffers": [{"byteLength": 36}]}
    return g, [tri.tobytes()]


def test_loader_builds_the_material_table():
    mats = [{"name": "a", "pbrMetallicRoughness": {"baseColorFactor": [0.25, 0.5, 0.75, 1.0], "metallicFactor": 0.125, "roughnessFactor": 0.625},
             "emissiveFactor": [1.0, 0.5, 0.25], "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 4.0}}, "alphaCutoff": 0.25},
            {"name": "b", "emissiveFactor": [0.005, 0.005, 0.005]},                       # squared length 7.5e-5 <= 1e-4: no emissive
            {"name": "c", "pbrMetallicRoughness": {}, "alphaMode": "MASK"},
            {"name": "d", "extensions": {"KHR_materials_pbrSpecularGlossiness": {"diffuseFactor": [0.1, 0.2, 0.3, 1.0], "specularFactor": [0.2, 0.9, 0.4],
                                                                                "glossinessFactor": 0.75}}}]
    g, blobs = _gltf_with_materials(mats, [0, None, 3, 2])
    s = gltf_lite.load(g, blobs, lods=False)
    m = s.materials
    assert m.dtype == I.MaterialData and len(m) == 5 and I.MaterialData.itemsize == 124
    assert s.primMaterial.tolist() == [0, 4, 3, 2] and s.primMaterial.dtype == np.uint32
    assert np.array_equal(m["m_ConstAlbedo"][0], np.array([0.25, 0.5, 0.75, 1.0], F)) and np.array_equal(m["m_ConstEmissive"][0], np.array([4.0, 2.0, 1.0], F))
    assert (m["m_AlphaCutoff"][0], m["m_ConstMetallic"][0], m["m_ConstRoughness"][0]) == (F(0.25), F(0.125), F(0.625))
    assert np.all(m["m_ConstEmissive"][1] == 0) and np.all(m["m_ConstAlbedo"][1] == 1) and (m["m_ConstRoughness"][1], m["m_ConstMetallic"][1]) == (1, 0)
    assert m["m_AlphaCutoff"][1] == F(0.5)
    assert np.all(m["m_ConstAlbedo"][2] == 1) and (m["m_ConstRoughness"][2], m["m_ConstMetallic"][2]) == (1, 1), "glTF defaults of pbrMetallicRoughness"
    assert np.array_equal(m["m_ConstAlbedo"][3], np.array([0.1, 0.2, 0.3, 1.0], F)) and m["m_ConstMetallic"][3] == F(0.9) and m["m_ConstRoughness"][3] == F(1.0) - F(0.75)
    assert np.array_equal(m["m_ConstAlbedo"][4], np.array([1.0, 0.078, 0.576, 1.0], F)) and m["m_ConstRoughness"][4] == 1, "the default material comes last"
    assert np.all(m["m_MaterialFlags"] == 0)
    for t in ("m_AlbedoTexture", "m_NormalTexture", "m_MetallicRoughnessTexture", "m_EmissiveTexture"):
        assert np.all(m[t]["m_GlobalIndex"] == 0xFFFFFFFF) and np.all(m[t]["m_DescriptorIndex"] == 0xFFFFFFFF) and np.all(m[t]["m_IsWrapSampler"] == 0)
    # load() leaves the instances as they were; apply_materials() writes the indices into a copy
    assert np.all(s.instances["m_MaterialDataIdx"] == 0)
    inst = gltf_lite.apply_materials(s)
    assert inst["m_MaterialDataIdx"].tolist() == [0, 4, 3, 2] and np.all(s.instances["m_MaterialDataIdx"] == 0)
    other = inst.copy(); other["m_MaterialDataIdx"] = 0
    assert other.tobytes() == s.instances.tobytes()
    assert s.alphaMaskIds.tolist() == [3]


@pytest.mark.parametrize("where", ["baseColorTexture", "metallicRoughnessTexture", "emissiveTexture", "normalTexture", "diffuseTexture"])
def test_loader_refuses_a_textured_material(where):
    mat = {"name": "textured"}
    if where in ("baseColorTexture", "metallicRoughnessTexture"):
        mat["pbrMetallicRoughness"] = {where: {"index": 0}}
    elif where == "diffuseTexture":
        mat["extensions"] = {"KHR_materials_pbrSpecularGlossiness": {where: {"index": 0}}}
    else:
        mat[where] = {"index": 0}
    g, blobs = _gltf_with_materials([mat], [0])
    with pytest.raises(ValueError, match=where):
        gltf_lite.load(g, blobs, lods=False)


def test_synthetic_materials():
    m = synth.materials(5)
    assert m.dtype == I.MaterialData and len(m) == 64 and np.all(m["m_MaterialFlags"] == 0)
    assert np.all((m["m_ConstAlbedo"][:, :3] >= 0) & (m["m_ConstAlbedo"][:, :3] < 1)) and np.any(m["m_ConstEmissive"] > 0) and np.any(np.all(m["m_ConstEmissive"] == 0, axis=1))
    assert m.tobytes() == synth.materials(5).tobytes() and m.tobytes() != synth.materials(6).tobytes()
    assert len(synth.materials(5, 8)) == 8


# ---- declarations ---------------------------------------------------------------------------------------------------------
def test_exports_and_declarations():
    from toyrenderer_amd import host, rhi
    h = open(os.path.join(ROOT, "include", "trhip.h")).read()
    assert re.search(r"TRHIP_FORMAT_RGBA32_UINT\s*=\s*5", h) and rhi.FORMAT_RGBA32_UINT == 5
    assert "basepass_PS_Main_GBuffer" in h
    lib = rhi.load()
    assert lib.trhip_abi_version() == 1
    names = set(rhi.shader_names())
    assert {"basepass_PS_Main_motion", "basepass_PS_Main_GBuffer"} <= names
    t = open(os.path.join(ROOT, "include", "trhost.h")).read()
    assert re.search(r"int\s+trhost_load_materials\s*\(\s*const\s+void\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", t)
    assert re.search(r"int\s+trhost_set_gbuffer\s*\(\s*int\s+\w+\s*\)\s*;", t)
    assert re.search(r"int\s+trhost_set_debug_view_mode\s*\(\s*uint32_t\s+\w+\s*\)\s*;", t)
    assert re.search(r"int\s+trhost_download_gbuffer_a\s*\(\s*uint32_t\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*\)\s*;", t)
    for f in ("trhost_load_materials", "trhost_set_gbuffer", "trhost_set_debug_view_mode", "trhost_download_gbuffer_a"):
        assert f in host.HOST_SYMBOLS and hasattr(host.load(), f), f
    for m in ("load_materials", "set_gbuffer", "set_debug_view_mode", "download_gbuffer_a"):
        assert callable(getattr(host.Renderer, m, None)), m
    assert (I.MaterialFlag_UseAlbedoTexture, I.MaterialFlag_UseNormalTexture, I.MaterialFlag_UseMetallicRoughnessTexture, I.MaterialFlag_UseEmissiveTexture) == (1, 2, 4, 8)


def test_material_struct_layout_matches_numpy(tmp_path):
    """A g++-compiled probe prints sizeof / offsetof of interop::MaterialData and interop::TextureData (csrc/ShaderInterop.h):
    124 and 20 bytes, every field where the numpy dtype has it."""
    fields = [n for n in I.MaterialData.names]
    prints = [("sizeof", "sizeof(interop::MaterialData)"), ("texture", "sizeof(interop::TextureData)")]
    prints += [(f, f"offsetof(interop::MaterialData, {f})") for f in fields]
    prints += [(f"t_{f}", f"offsetof(interop::TextureData, {f})") for f in I.TextureData.names]
    out = layout_probe(tmp_path, prints)
    assert int(out["sizeof"]) == 124 == I.MaterialData.itemsize and int(out["texture"]) == 20 == I.TextureData.itemsize
    for f in fields:
        assert int(out[f]) == I.MaterialData.fields[f][1], f
    for f in I.TextureData.names:
        assert int(out["t_" + f]) == I.TextureData.fields[f][1], f
