"""The restatement of the textured G-buffer resolve (tests/material_textures_ref.c) against hand-derived cases, the sRGB table,
interop.make_mips, the glTF loader's texture coordinates and images=, and the declarations of the new symbols.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import material_texture_scenes as S  # noqa: E402
import material_textures_ref as MT  # noqa: E402
from suite_support import mt  # noqa: E402, F401
from toyrenderer_amd import gltf_lite  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_srgb_table_is_the_float64_formula_rounded_once(mt):
    from toyrenderer_amd import rhi
    c = np.arange(256, dtype=np.float64) / 255.0
    want = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(np.float32)
    assert np.array_equal(MT.srgb_table(mt), want), "the reference's table"
    assert np.array_equal(rhi.srgb_table(), want), "the back end's table (trhip_srgb_table)"
    assert want[0] == 0 and want[255] == 1 and np.all(np.diff(want) > 0)
    assert want[10] == F(10 / 255 / 12.92) and abs(float(want[128]) - 0.21586) < 1e-5


def test_half_to_float_is_exact_for_every_half(mt):
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = np.array([mt.mt_half_to_float(int(x)) for x in h], np.float32)
    want = h.view(np.float16).astype(np.float32)
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)]) and np.all(np.isnan(got[np.isnan(want)]))


def test_make_mips_on_a_hand_computed_image():
    """4 x 2 -> 2 x 1 -> 1 x 1.  UNORM: plain means, rounded half to even.  sRGB: the mean of the decoded values, encoded; alpha stays
    linear.  The second level comes from the first level's unrounded float64 values."""
    img = np.zeros((2, 4, 4), np.uint8)
    img[0, :, 0] = (0, 10, 100, 200); img[1, :, 0] = (20, 30, 101, 201)            # red: means 15 and 150.5 -> 150 (half to even)
    img[..., 1] = 255; img[0, 0, 1] = 0                                             # green: (0 + 255 * 3) / 4 = 191.25 and 255
    img[..., 3] = np.array([[1, 2, 3, 4], [5, 6, 7, 8]])                           # alpha: 3.5 -> 4, 5.5 -> 6
    m = I.make_mips(img, srgb=False)
    assert [x.shape for x in m] == [(2, 4, 4), (1, 2, 4), (1, 1, 4)] and np.array_equal(m[0], img)
    assert m[1][0, :, 0].tolist() == [15, 150] and m[1][0, :, 1].tolist() == [191, 255] and m[1][0, :, 3].tolist() == [4, 6]
    assert m[2][0, 0].tolist() == [83, 223, 0, 4]                                   # (15 + 150.5) / 2 = 82.75, (191.25 + 255) / 2 = 223.125, 4.5 -> 4
    s = I.make_mips(img, srgb=True)
    dec = lambda b: I.srgb_to_linear(np.asarray(b, np.float64) / 255.0)             # noqa: E731
    enc = lambda x: int(np.rint(I.linear_to_srgb(x) * 255.0))                       # noqa: E731
    assert s[1][0, 0, 0] == enc(dec([0, 10, 20, 30]).mean()) and s[1][0, 1, 0] == enc(dec([100, 200, 101, 201]).mean())
    assert s[1][0, 0, 1] == enc(0.75) == 225 and s[1][0, :, 3].tolist() == [4, 6], "linear-light mean of 0, 1, 1, 1; alpha linear"
    assert s[1][0, 0, 0] > m[1][0, 0, 0], "a mean in linear light is brighter than the mean of the codes"
    odd = I.make_mips(np.arange(5 * 12 * 4, dtype=np.uint16).reshape(5, 12, 4).astype(np.uint8), srgb=False)
    assert [x.shape[:2] for x in odd] == [(5, 12), (2, 6), (1, 3), (1, 1)], "max(w >> k, 1) x max(h >> k, 1)"
    assert len(I.make_mips(img, False, levels=2)) == 2
    with pytest.raises(ValueError):
        I.make_mips(np.zeros((4, 4, 3), np.uint8), False)


def _texture(fmt=MT.FORMAT_RGBA8):
    """8 x 8 with 4 levels; texel (x, y) of level k is (16 x + k, 16 y + k, 255 - 16 x, 100 + k)."""
    mips = []
    for k in range(4):
        n = 8 >> k
        m = np.zeros((n, n, 4), np.uint8)
        m[..., 0] = 16 * np.arange(n)[None, :] + k
        m[..., 1] = 16 * np.arange(n)[:, None] + k
        m[..., 2] = 255 - 16 * np.arange(n)[None, :]
        m[..., 3] = 100 + k
        mips.append(m)
    return MT.Texture(mips, fmt)


def test_sampler_at_texel_centres_returns_the_texel(mt):
    t, srgb = _texture(), _texture(MT.FORMAT_SRGBA8)
    table = MT.srgb_table(mt)
    for x, y in ((0, 0), (3, 5), (7, 7), (6, 1)):
        uv = ((x + 0.5) / 8, (y + 0.5) / 8)
        for wrap in (0, 1):
            v, n, lod = MT.sample(mt, t, wrap, uv, (1 / 8, 0), (0, 1 / 8))
            assert (n, lod) == (1, 0.0) and np.array_equal(v, t.mips[0][y, x].astype(F) / F(255)), (x, y, wrap)
            v, n, lod = MT.sample(mt, srgb, wrap, uv, (1 / 8, 0), (0, 1 / 8))
            assert np.array_equal(v[:3], table[t.mips[0][y, x, :3]]) and v[3] == F(100) / F(255), "R, G, B through the table, alpha linear"


def test_sampler_wrap_seam_and_clamp_edge(mt):
    t = _texture()
    px = lambda x, y: t.mips[0][y, x].astype(F) / F(255)                            # noqa: E731
    # u = 0 is the seam: wrap averages columns 7 and 0, clamp reads column 0 twice; v at a texel centre
    uv = (0.0, 2.5 / 8)
    w, _, _ = MT.sample(mt, t, 1, uv, (1 / 8, 0), (0, 1 / 8))
    c, _, _ = MT.sample(mt, t, 0, uv, (1 / 8, 0), (0, 1 / 8))
    assert np.array_equal(w, px(7, 2) + F(0.5) * (px(0, 2) - px(7, 2))) and np.array_equal(c, px(0, 2))
    # far outside: wrap repeats (u = 2 + 3.5 / 8 and u = -3 + 3.5 / 8 are column 3), clamp holds the border texel
    for u in (2 + 3.5 / 8, -3 + 3.5 / 8):
        v, _, _ = MT.sample(mt, t, 1, (u, 2.5 / 8), (1 / 8, 0), (0, 1 / 8))
        assert np.array_equal(v, px(3, 2)), u
    assert np.array_equal(MT.sample(mt, t, 0, (2.4, 2.5 / 8), (1 / 8, 0), (0, 1 / 8))[0], px(7, 2))
    assert np.array_equal(MT.sample(mt, t, 0, (-1.5, -1.5), (1 / 8, 0), (0, 1 / 8))[0], px(0, 0))
    assert np.all(np.isnan(MT.sample(mt, t, 0, (np.nan, 2.5 / 8), (1 / 8, 0), (0, 1 / 8))[0])), "a NaN coordinate reads column 0 with a NaN weight"
    # the bottom-right corner under wrap: all four corners of the texture
    v, _, _ = MT.sample(mt, t, 1, (1.0, 1.0), (1 / 8, 0), (0, 1 / 8))
    top, bot = px(7, 7) + F(0.5) * (px(0, 7) - px(7, 7)), px(7, 0) + F(0.5) * (px(0, 0) - px(7, 0))
    assert np.array_equal(v, top + F(0.5) * (bot - top))


def test_sampler_lod_is_clamped_at_both_ends_and_blends_between(mt):
    t = _texture()
    centre = (0.5, 0.5)
    # magnified: a quarter texel per pixel -> lod = -2 -> 0, level 0 alone
    v, n, lod = MT.sample(mt, t, 0, centre, (0.25 / 8, 0), (0, 0.25 / 8))
    assert (n, lod) == (1, 0.0)
    # 64 texels per pixel -> lod = 6 -> 3 (the last level): its one texel, from both levels of the blend
    v, n, lod = MT.sample(mt, t, 0, centre, (8.0, 0), (0, 8.0))
    assert (n, lod) == (1, 3.0) and np.array_equal(v, t.mips[3][0, 0].astype(F) / F(255))
    # 2 texels per pixel: exactly level 1 (log2Soft is exact at powers of two)
    v, n, lod = MT.sample(mt, t, 0, (2.5 / 4, 1.5 / 4), (2 / 8, 0), (0, 2 / 8))
    assert (n, lod) == (1, 1.0) and np.array_equal(v, t.mips[1][1, 2].astype(F) / F(255))
    # 3 texels per pixel: lod = log2(3) = 1.585, between level 1 and level 2 at their shared texel centre
    v, n, lod = MT.sample(mt, t, 0, (0.25, 0.25), (3 / 8, 0), (0, 3 / 8))
    f = F(lod) - F(1)
    assert n == 1 and abs(lod - np.log2(3)) < 1e-6
    b1 = np.mean([t.mips[1][y, x].astype(F) / F(255) for y in (0, 1) for x in (0, 1)], axis=0)    # u = 0.25 is the corner of four level-1 texels
    b2 = t.mips[2][0, 0].astype(F) / F(255)                                                     # and the centre of level 2's texel (0, 0)
    assert np.allclose(v, b1 + f * (b2 - b1), rtol=0, atol=2e-7)
    # zero derivatives: Pmax = 0 -> lod 0; NaN derivatives -> 16 taps, lod 0
    assert MT.sample(mt, t, 0, centre, (0, 0), (0, 0))[1:] == (16, 0.0)
    assert MT.sample(mt, t, 0, centre, (np.nan, 0), (0, 1 / 8))[1] == 16


@pytest.mark.parametrize("ratio, taps", [(1.0, 1), (2.0, 2), (1.5, 2), (5.0, 5), (4.01, 5), (16.0, 16), (40.0, 16)])
def test_sampler_tap_count_and_lod(mt, ratio, taps):
    """Pmin = 1 texel per pixel along v, Pmax = ratio along u: N = min(ceil(ratio), 16), lod = log2(ratio / N); with the ratio
    capped the footprint no longer fits and the level rises (40 / 16 = 2.5 texels per tap)."""
    t = _texture()
    for dx, dy in (((ratio / 8, 0), (0, 1 / 8)), ((0, 1 / 8), (ratio / 8, 0))):       # the major axis is ddx, then ddy
        v, n, lod = MT.sample(mt, t, 1, (0.3, 0.4), dx, dy)
        assert n == taps
        assert abs(lod - max(np.log2(ratio / taps), 0.0)) < 1e-6
    # the taps: N equally spaced points along the major axis, centred on uv; level 0 here, so the mean of N bilinear values
    if ratio / taps <= 1.0:
        v, n, _ = MT.sample(mt, t, 1, (0.3, 0.4), (ratio / 8, 0), (0, 1 / 8))
        acc = np.zeros(4, F)
        for i in range(n):
            k = (F(i) + F(0.5)) / F(n) - F(0.5)
            u = F(0.3) + F(ratio / 8) * k
            acc = acc + MT.sample(mt, t, 1, (u, 0.4), (0.5 / 8, 0), (0, 0.5 / 8))[0]   # an isotropic, magnified sample: one bilinear value
        assert np.array_equal(v, acc / F(n))


def test_sampler_with_pmin_zero_takes_sixteen_taps(mt):
    t = _texture()
    v, n, lod = MT.sample(mt, t, 1, (0.3, 0.4), (4 / 8, 0), (0, 0))
    assert n == 16 and lod == 0.0                                                     # 4 / 16 texels per tap
    v, n, lod = MT.sample(mt, t, 1, (0.3, 0.4), (64 / 8, 0), (0, 0))
    assert n == 16 and lod == 2.0


# ---- the loader -------------------------------------------------------------------------------------------------------------
def test_loader_fills_texcoords_and_maps_textures():
    g, blobs, images = S.textured_gltf()
    s = gltf_lite.load(g, blobs, lods=False, images=images)
    uv = np.frombuffer(blobs[0], np.float32, 16 * 2, 16 * 12 * 2).reshape(16, 2)
    assert np.array_equal(s.vertices["m_TexCoord"][:16].view(np.float16), uv.astype(np.float16)), "TEXCOORD_0 as half2"
    assert np.array_equal(s.vertices["m_TexCoord"][:16], s.vertices["m_TexCoord"][16:32]) and float(uv.min()) == -1.5 and float(uv.max()) == 2.5
    m = s.materials
    A, N, MR, E = S.ALBEDO, S.NORMAL, S.MR, S.EMISSIVE
    assert m["m_MaterialFlags"].tolist() == [A | N | MR | E, A, 0, A, 0]
    # (glTF texture, format) pairs in order of first use: base colour and emissive sRGB, normal and metallic-roughness UNORM
    assert [(f, t[0].shape) for t, f in s.textures] == [(11, (8, 8, 4)), (10, (8, 8, 4)), (10, (5, 12, 4)), (11, (5, 12, 4)), (11, (5, 12, 4)), (11, (1, 1, 4))]
    assert [len(t) for t, _ in s.textures] == [4, 4, 4, 4, 4, 1]
    assert np.array_equal(s.textures[0][0][0], images[0]) and np.array_equal(s.textures[0][0][1], I.make_mips(images[0], True)[1])
    assert np.array_equal(s.textures[1][0][1], I.make_mips(images[0], False)[1])
    assert m["m_AlbedoTexture"]["m_DescriptorIndex"].tolist() == [0, 4, S.NONE, 5, S.NONE]
    assert (m["m_NormalTexture"]["m_DescriptorIndex"][0], m["m_MetallicRoughnessTexture"]["m_DescriptorIndex"][0], m["m_EmissiveTexture"]["m_DescriptorIndex"][0]) == (1, 2, 3)
    assert m["m_AlbedoTexture"]["m_GlobalIndex"].tolist() == [0, 2, S.NONE, 3, S.NONE], "the glTF texture index"
    assert m["m_AlbedoTexture"]["m_IsWrapSampler"].tolist() == [1, 0, 0, 1, 0], "REPEAT, CLAMP_TO_EDGE, none, REPEAT"
    assert m["m_MetallicRoughnessTexture"]["m_IsWrapSampler"][0] == 1, "a texture without a sampler repeats"
    for slot in S.SLOTS:
        assert np.all(m[slot]["m_FeedbackTextureDescriptorIndex"] == S.NONE) and np.all(m[slot]["m_MinMapTextureDescriptorIndex"] == S.NONE)
    # mips handed in are taken as they are
    own = [images[0], np.zeros((4, 4, 4), np.uint8)]
    s2 = gltf_lite.load(g, blobs, lods=False, images=[own, images[1], images[2]])
    assert len(s2.textures[0][0]) == 2 and np.array_equal(s2.textures[0][0][1], own[1])


def test_loader_without_images_still_raises_and_refuses_what_it_cannot_map():
    g, blobs, images = S.textured_gltf()
    with pytest.raises(ValueError, match="baseColorTexture"):
        gltf_lite.load(g, blobs, lods=False)
    assert gltf_lite.load(g, blobs, lods=False, images=images).textures is not None
    sg = dict(g); sg["materials"] = [{"extensions": {"KHR_materials_pbrSpecularGlossiness": {"diffuseTexture": {"index": 0}}}}] + g["materials"][1:]
    with pytest.raises(ValueError, match="diffuseTexture"):
        gltf_lite.load(sg, blobs, lods=False, images=images)
    mirrored = dict(g); mirrored["samplers"] = [{"wrapS": 33648, "wrapT": 33648}, g["samplers"][1]]
    with pytest.raises(ValueError, match="sampler 0"):
        gltf_lite.load(mirrored, blobs, lods=False, images=images)
    with pytest.raises(ValueError, match="no image"):
        gltf_lite.load(g, blobs, lods=False, images=images[:1])


# ---- declarations -----------------------------------------------------------------------------------------------------------
def test_exports_and_declarations():
    from toyrenderer_amd import frame, host, rhi
    h = open(os.path.join(ROOT, "include", "trhip.h")).read()
    assert re.search(r"TRHIP_FORMAT_SRGBA8_UNORM\s*=\s*11", h) and rhi.FORMAT_SRGBA8_UNORM == 11
    assert re.search(r"TRHIP_BIND_TEXTURE_TABLE\s*=\s*7", h) and rhi.BIND_TEXTURE_TABLE == 7 and rhi.TEXTURE_TABLE_SLOT == 19 and "t19" in h
    for f in ("trhip_texture_table_create", "trhip_texture_table_retain", "trhip_texture_table_release", "trhip_texture_table_capacity",
              "trhip_texture_table_set", "trhip_texture_table_clear", "trhip_srgb_table"):
        assert f in rhi.ABI_SYMBOLS and hasattr(rhi.load(), f) and re.search(r"\b" + f + r"\s*\(", h), f
    t = open(os.path.join(ROOT, "include", "trhost.h")).read()
    assert re.search(r"int\s+trhost_create_material_texture\s*\(\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*\)\s*;", t)
    assert "trhost_create_material_texture" in host.HOST_SYMBOLS and hasattr(host.load(), "trhost_create_material_texture")
    assert callable(host.Renderer.create_material_texture) and callable(host.Renderer.load_textures) and callable(frame.GpuScene.set_textures)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "t19" in design and "material_textures_ref.c" in design
