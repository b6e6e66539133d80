"""Textured materials on the GPU: "basepass_PS_Main_GBuffer" with a texture table at t19 (csrc/visibility_resolve.hip.h,
csrc/material_textures.hip.h), every word of GBufferA and of the motion target against tests/material_textures_ref.c, through
raw dispatches; the tie to the texture-free kernel, the level of detail against geometry, bounds and misuse."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gbuffer_ref as GR  # noqa: E402
import material_texture_scenes as S  # noqa: E402
import material_textures_ref as MT  # noqa: E402
from suite_support import dev, gr, host_renderer, mt, same, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import consts  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xABCD1234


def _upload(dev, textures, capacity=None):
    """(table, [textures]) of a list of (mips, format) or None (an empty entry)."""
    table = dev.create_texture_table(capacity or max(len(textures), 1))
    made = []
    for i, t in enumerate(textures):
        if t is not None:
            made.append(dev.create_sampled_texture(t[0], t[1], f"material texture {i}"))
            table.set(i, made[-1])
    return table, made


def _dispatch(dev, k, scene, render, materials, table, clear_to=FILL, debug_mode=0):
    """One visibility dispatch and one G-buffer resolve (with `table` at t19 unless None): (vis, GBufferA, motion halves, the
    profile's basepass_PS names)."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, PUSH, SRV, TEX_SRV, TEX_TABLE, TEX_UAV
    sc, v, vid, tri, rec, lst = scene
    W, H = render
    k = np.ascontiguousarray(k).copy()
    k["m_DebugMode"] = debug_mode
    bufs = [dev.buffer_from(sc["instances"], "inst", uav=False), dev.buffer_from(v, "v", uav=False, min_bytes=20),
            dev.buffer_from(sc["meshData"], "md", uav=False), dev.buffer_from(sc["meshlets"], "ml", uav=False, min_bytes=32),
            dev.buffer_from(vid, "vid", uav=False), dev.buffer_from(tri, "tri", uav=False), dev.buffer_from(rec, "rec", min_bytes=12),
            dev.buffer_from(lst, "lst"), dev.buffer_from(np.ascontiguousarray(materials, I.MaterialData), "materials", uav=False, min_bytes=124)]
    empty = dev.create_buffer(16, "empty")
    args = dev.create_buffer(12, "drawArgs", stride=12, indirect=True)
    args.upload(np.array([len(lst), 1, 1], np.uint32))
    depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
    vis = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "VisibilityBuffer")
    mot = dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, "GBufferMotion")
    gba = dev.create_texture(W, H, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA")
    cl = dev.create_command_list()
    try:
        cl.open()
        cl.clear_texture_f32(depth, 0.0); cl.clear_texture_u32(vis, 0); cl.clear_texture_f32(mot, 0.0); cl.clear_texture_u32(gba, clear_to)
        cb = cl.constant_buffer(k, "BasePassConstants")
        geo = [CB(0, cb), SRV(0, bufs[0]), SRV(1, bufs[1]), SRV(2, bufs[2]), SRV(4, bufs[3]), SRV(5, bufs[4]), SRV(6, bufs[5])]
        cl.dispatch_indirect("basepass_MS_Main_visibility", geo + [SRV(7, bufs[6]), SRV(9, bufs[7]), TEX_UAV(0, depth, 0), TEX_UAV(1, vis, 0), PUSH(1)],
                             args, push=np.array([0], np.uint32))
        slots = []
        for s in range(4):
            slots += [SRV(10 + s, bufs[6] if s == 0 else empty), SRV(14 + s, bufs[7] if s == 0 else empty)]
        bind = geo + slots + [SRV(3, bufs[8]), TEX_SRV(18, vis), TEX_UAV(0, gba, 0), TEX_UAV(1, mot, 0)]
        cl.dispatch("basepass_PS_Main_GBuffer", bind + ([TEX_TABLE(table)] if table is not None else []), ((W + 7) // 8, (H + 7) // 8, 1))
        cl.close()
        dev.profile_reset(); dev.profile_enable(True)
        try:
            dev.execute(cl); dev.wait_idle()
            prof = dev.profile()
        finally:
            dev.profile_enable(False)
        return vis.download_mip(0), gba.download_mip(0), mot.download_mip(0).view(np.uint16), sorted(n for n in prof if n.startswith("basepass_PS"))
    finally:
        cl.release(); depth.release(); vis.release(); mot.release(); gba.release(); args.release(); empty.release()
        for b in bufs:
            b.release()


def _reference(vr, mt, k, scene, render, materials, textures, clear_to=FILL, debug_mode=0):
    sc, v, vid, tri, rec, lst = scene
    W, H = render
    geo = VR.Geometry(sc, v, vid, tri)
    depth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
    VR.raster(vr, k, geo, rec, lst, 0, depth, vis)
    table = [None if t is None else MT.Texture(*t) for t in textures]
    g, m, taps = MT.gbuffer(mt, k, geo, [rec, None, None, None], [lst, None, None, None], vis, materials, table, debug_mode,
                            gbuffer_init=np.full((H, W, 4), clear_to, np.uint32))
    return vis, g, VR.to_half_bits(m), taps


def _both(dev, vr, mt, k, scene, materials, textures, render=S.RENDER, what="", capacity=None):
    """Runs the scene on the GPU and in the reference, asserts every word equal, returns (vis, GBufferA, taps)."""
    table, made = _upload(dev, textures, capacity)
    try:
        vis, g, mot, names = _dispatch(dev, k, scene, render, materials, table)
    finally:
        table.release()
        for t in made:
            t.release()
    rvis, rg, rmot, taps = _reference(vr, mt, k, scene, render, materials, textures[:capacity] if capacity else textures)
    same(vis, rvis, what + ": visibility texels")
    same(g, rg, what + ": GBufferA")
    same(mot, rmot, what + ": motion")
    assert names == ["basepass_PS_Main_GBuffer#textured"], names
    return vis, g, taps


ALL = S.ALBEDO | S.NORMAL | S.MR | S.EMISSIVE
EMIT = (2.0, 0.5, 4.0)
CASES = {
    "albedo alone, sRGB, wrap": dict(flags=S.ALBEDO, indices=(0, S.NONE, S.NONE, S.NONE)),
    "albedo alone, UNORM, wrap": dict(flags=S.ALBEDO, indices=(6, S.NONE, S.NONE, S.NONE)),
    "normal map alone": dict(flags=S.NORMAL, indices=(S.NONE, 1, S.NONE, S.NONE)),
    "metallic-roughness alone": dict(flags=S.MR, indices=(S.NONE, S.NONE, 2, S.NONE)),
    "emissive alone": dict(flags=S.EMISSIVE, indices=(S.NONE, S.NONE, S.NONE, 3), emissive=EMIT),
    "all four, wrap": dict(flags=ALL, indices=(0, 1, 2, 3), emissive=EMIT),
    "all four, clamp": dict(flags=ALL, indices=(0, 1, 2, 3), emissive=EMIT, wrap=(0, 0, 0, 0)),
    "all four, the non-square texture": dict(flags=ALL, indices=(4, 4, 4, 4), emissive=EMIT, wrap=(1, 0, 1, 0)),
    "all four, the 1 x 1 texture": dict(flags=ALL, indices=(5, 5, 5, 5), emissive=EMIT),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_word_equals_the_restatement(dev, vr, mt, case):
    """A camera-facing quad with UVs in [-1.5, 2.5] (wrap repeats it four times, clamp smears its border), rotated a little about
    z so that both derivatives have two components, larger than a 16 x 16 tile; each texture alone and all four, sRGB and UNORM."""
    c, s = np.cos(0.3), np.sin(0.3)
    world = np.array([[c, s, 0, 0], [-s, c, 0, 0], [0, 0, 1, 0], [0.1, -0.05, 0, 1]])
    scene = S.build([S.facing(material=0, world=world)])
    vis, g, taps = _both(dev, vr, mt, consts(S.view()), scene, S.material(**CASES[case]), S.standard_textures(), what=case)
    cov = vis != 0
    assert cov.sum() > 1500 and np.all(g[~cov] == FILL)
    ys, xs = np.nonzero(cov)
    assert xs.min() < 16 < xs.max() and ys.min() < 16 < ys.max(), "the quad crosses a tile border of the resolve"
    flags = CASES[case]["flags"]
    for bit in range(4):
        assert np.all((taps[cov][:, bit] > 0) == bool(flags & (1 << bit)))
    if not flags & S.MR:
        assert np.all(g[cov][:, 3] == 0xFF)
    elif "1 x 1" not in case:
        assert len(np.unique(g[cov][:, 3])) > 50, "roughness and metallic vary over the quad"
    if flags & S.ALBEDO and "1 x 1" not in case:
        assert len(np.unique(g[cov][:, 0])) > 100


def test_a_grazing_floor_takes_every_tap_count(dev, vr, mt):
    """The floor's footprint ratio runs from below 2 at the bottom of the screen to beyond 16 at the horizon: the reference's own N
    takes many values and reaches the cap, and every word still agrees."""
    scene = S.build([S.floor(material=0)])
    mats = S.material(flags=ALL, indices=(0, 1, 2, 3), emissive=EMIT)
    vis, g, taps = _both(dev, vr, mt, consts(S.view()), scene, mats, S.standard_textures(), what="floor")
    cov = vis != 0
    n = np.unique(taps[cov][:, 0])
    assert cov.sum() > 1000 and n.max() == 16 and n.min() <= 3 and len(n) >= 8, n
    assert np.array_equal(taps[cov][:, 0], taps[cov][:, 2]), "textures of one size share their footprint"


def test_magnified_and_minified_quads_and_a_degenerate_mapping(dev, vr, mt):
    """Left: a quad so close that a texel covers many pixels (level 0, magnified).  Right: a quad so far that its footprint is larger
    than the whole texture (the last mip alone: the albedo of solid-coloured mips is the last colour).  Bottom: a quad whose three
    texture coordinates coincide, under a normal map: the derivatives are 0 or rounding noise, the tangent frame is NaN or arbitrary,
    and the words still agree."""
    last = (10, 200, 90)
    textures = S.standard_textures() + [(S.solid_mips([(250, 0, 0), (0, 250, 0), (0, 0, 250), last]), S.RGBA8)]
    quads = [S.facing(z=-1.2, half=0.35, uv_lo=0.2, uv_hi=0.45, material=0, centre=(-0.3, 0.1)),
             S.facing(z=-30.0, half=5.0, uv_lo=0.0, uv_hi=64.0, material=1, centre=(7.0, 2.0)),
             S.facing(z=-3.0, half=0.5, uv_lo=0.3, uv_hi=0.3, material=2, centre=(0.0, -0.8))]
    mats = np.concatenate([S.material(flags=ALL, indices=(0, 1, 2, 3), emissive=EMIT),
                           S.material(flags=S.ALBEDO, albedo=(1.0, 1.0, 1.0, 1.0), indices=(7, S.NONE, S.NONE, S.NONE)),
                           S.material(flags=S.ALBEDO | S.NORMAL, indices=(0, 1, S.NONE, S.NONE))])
    scene = S.build(quads)
    vis, g, taps = _both(dev, vr, mt, consts(S.view()), scene, mats, textures, what="near, far, degenerate")
    _, _, pos, _ = VR.decode(vis)
    owner = np.where(vis != 0, scene[4]["m_InstanceConstIdx"][scene[5][pos] >> 5], 99)
    assert all((owner == i).sum() > 60 for i in range(3)), [(owner == i).sum() for i in range(3)]
    want = (np.array(last, np.float32) / np.float32(255.0) * np.float32(255.0)).astype(np.uint32)        # packRGBA8 truncates
    assert np.all(GR.albedo_bytes(g[owner == 1][:, 0]) == want), "the far quad reads the last mip alone"
    assert np.all(taps[owner == 0][:, 0] <= 2)
    assert np.all(taps[owner == 2][:, :2] >= 1)


def test_uniform_textures_tie_to_the_texture_free_kernel(dev, vr, mt):
    """No new reference here.  A metallic-roughness texture of (0, 255, 0), white sRGB albedo and emissive textures, the normal flag
    off: GBufferA is bit-identical to the texture-free kernel's frame of the same scene (no table bound).  With a uniform albedo
    texel c the albedo bytes are packRGBA8(m_ConstAlbedo * decode(c)).  A lerp of equal values is exact; a sum of N equal values
    divided by N is exact for N = 1 and 2 only, which is what a camera-facing quad with a 1 x 1 texture takes."""
    from toyrenderer_amd import rhi
    one = lambda rgb: [np.array([[list(rgb) + [255]]], np.uint8)]
    c = (200, 31, 117)
    textures = [(one((255, 255, 255)), S.SRGBA8), (one((0, 255, 0)), S.RGBA8), (one(c), S.SRGBA8), (one(c), S.RGBA8)]
    scene = S.build([S.facing(material=0)])
    k = consts(S.view())
    plain = S.material(emissive=EMIT)
    table, made = _upload(dev, textures)
    try:
        vis0, g0, mot0, names0 = _dispatch(dev, k, scene, S.RENDER, plain, None)
        assert names0 == ["basepass_PS_Main_GBuffer#main"]
        mats = S.material(flags=S.ALBEDO | S.MR | S.EMISSIVE, indices=(0, S.NONE, 1, 0), emissive=EMIT)
        vis1, g1, mot1, names1 = _dispatch(dev, k, scene, S.RENDER, mats, table)
        assert names1 == ["basepass_PS_Main_GBuffer#textured"]
        same(vis1, vis0, "texels"); same(g1, g0, "GBufferA against the texture-free kernel"); same(mot1, mot0, "motion")
        cov = vis0 != 0
        assert cov.sum() > 1500
        for index, decode in ((2, rhi.srgb_table()), (3, (np.arange(256, dtype=np.float32) / np.float32(255.0)))):
            _, g2, _, _ = _dispatch(dev, k, scene, S.RENDER, S.material(flags=S.ALBEDO, indices=(index, S.NONE, S.NONE, S.NONE)), table)
            want = np.clip(plain["m_ConstAlbedo"][0][:3] * decode[list(c)], 0, 1) * np.float32(255.0)
            assert np.all(GR.albedo_bytes(g2[cov][:, 0]) == want.astype(np.uint32)), index
    finally:
        table.release()
        for t in made:
            t.release()


@pytest.mark.parametrize("k_level", [0, 1, 2])
def test_lod_follows_the_texel_to_pixel_ratio(dev, vr, mt, k_level):
    """A camera-facing quad over a 64 x 64 orthographic view (w = 1, corners on the screen's corners: every quantity of the resolve
    is a dyadic number, so both derivatives are exactly equal and N = ceil(Pmax / Pmin) is 1; with any rounding in them N would be
    2 and the level one lower, which is why this test does not use the 80 x 56 perspective view) with 1.5 * 2^k texels per pixel:
    lod = k + log2(1.5), so every albedo channel lies strictly between mip k's and mip k + 1's colour."""
    colours = [(0, 255, 64), (64, 191, 128), (128, 127, 192), (192, 63, 255)]
    render = (64, 64)
    span = 1.5 * 2 ** k_level * 64 / 8                               # texels per pixel * pixels / texels per repeat
    scene = S.build([S.quad((-1, -1, 0), (1, -1, 0), (-1, 1, 0), (1, 1, 0), (0, span), (span, span), (0, 0), (span, 0), grid=1)])
    mats = S.material(flags=S.ALBEDO, albedo=(1.0, 1.0, 1.0, 1.0), indices=(0, S.NONE, S.NONE, S.NONE))
    vis, g, taps = _both(dev, vr, mt, S.ortho_consts(render), scene, mats, [(S.solid_mips(colours), S.RGBA8)], render=render, what=f"k = {k_level}")
    cov = vis != 0
    assert cov.sum() > 3500 and np.all(taps[cov][:, 0] == 1)
    got = GR.albedo_bytes(g[cov][:, 0]).astype(np.int64)
    lo, hi = np.array(colours[k_level]), np.array(colours[k_level + 1])
    assert np.all((got - lo) * np.sign(hi - lo) > 0) and np.all((hi - got) * np.sign(hi - lo) > 0), (got.min(0), got.max(0), lo, hi)


def test_indices_past_the_table_and_cleared_entries_leave_their_pixels(dev, vr, mt):
    """Three quads side by side: the middle one's material names descriptor index 9 of a table of 8, then (second run) an entry
    that was set and cleared again, then an entry holding a texture of another format: its pixels keep the initial fill in both
    targets, the neighbours' are still correct."""
    from toyrenderer_amd import rhi
    quads = [S.facing(half=0.45, material=i, centre=(-1.0 + i, 0.0), grid=1) for i in range(3)]
    scene = S.build(quads)
    k = consts(S.view())
    textures = S.standard_textures()
    for bad in (9, 7, 6):
        mats = np.concatenate([S.material(flags=ALL, indices=(0, 1, 2, 3), emissive=EMIT),
                               S.material(flags=S.ALBEDO | S.MR, indices=(0, S.NONE, bad, S.NONE)),
                               S.material(flags=S.ALBEDO, indices=(4, S.NONE, S.NONE, S.NONE), wrap=(0, 0, 0, 0))])
        table, made = _upload(dev, textures[:6], capacity=8)
        other = dev.create_texture(4, 4, 1, rhi.FORMAT_R8_UNORM, "another format", uav=False)
        try:
            table.set(7, made[0]); table.clear(7)
            table.set(6, other)
            vis, g, mot, _ = _dispatch(dev, k, scene, S.RENDER, mats, table)
        finally:
            table.release(); other.release()
            for t in made:
                t.release()
        rvis, rg, rmot, _ = _reference(vr, mt, k, scene, S.RENDER, mats, textures[:6] + [None, None])
        same(vis, rvis, "texels"); same(g, rg, f"GBufferA, index {bad}"); same(mot, rmot, "motion")
        _, _, pos, _ = VR.decode(vis)
        owner = np.where(vis != 0, scene[4]["m_InstanceConstIdx"][scene[5][pos] >> 5], 99)
        assert all((owner == i).sum() > 100 for i in range(3))
        assert np.all(g[owner == 1] == FILL) and np.all(mot[owner == 1] == 0), "the broken material's pixels are untouched"
        assert np.all(g[owner == 0][:, 0] != FILL) and np.all(g[owner == 2][:, 0] != FILL)


def test_misuse_is_refused_at_record_time_and_the_next_dispatch_is_correct(dev, vr, mt):
    from toyrenderer_amd import rhi
    with pytest.raises(rhi.TrhipError, match="one mip"):
        dev.create_texture(8, 8, 4, rhi.FORMAT_RGBA8_UNORM, "a back buffer with mips", uav=True)
    with pytest.raises(rhi.TrhipError, match="one mip"):
        dev.create_texture(8, 8, 2, rhi.FORMAT_R8_UNORM, "a mask with mips", uav=False)
    with pytest.raises(rhi.TrhipError, match="unsupported format"):
        dev.create_texture(8, 8, 1, 9, "format 9", uav=False)
    scene = S.build([S.facing(material=0)])
    k = consts(S.view())
    mats = S.material(flags=S.ALBEDO, indices=(0, S.NONE, S.NONE, S.NONE))
    textures = S.standard_textures()[:1]
    writable = dev.create_texture(8, 8, 1, rhi.FORMAT_RGBA8_UNORM, "a UAV-capable texture", uav=True)
    table, made = _upload(dev, textures, capacity=2)
    try:
        table.set(1, writable)
        with pytest.raises(rhi.TrhipError, match="UAV"):
            _dispatch(dev, k, scene, S.RENDER, mats, table)
        with pytest.raises(rhi.TrhipError, match="capacity"):
            table.set(2, made[0])
        table.clear(1)
        cl = dev.create_command_list()
        depth = dev.create_texture(8, 8, 1, rhi.FORMAT_R32_FLOAT, "depth")
        target = dev.create_texture(8, 8, 1, rhi.FORMAT_R11G11B10_FLOAT, "target")
        try:                                                             # a table on a shader, or at a slot, that declares none
            cl.open()
            with pytest.raises(rhi.TrhipError, match="texture table"):
                cl.dispatch("sky_PS_HosekWilkieSky", [rhi.TEX_SRV(0, depth), rhi.TEX_UAV(0, target, 0), rhi.TEX_TABLE(table)], (1, 1, 1))
            with pytest.raises(rhi.TrhipError, match="t19"):
                cl.dispatch("basepass_PS_Main_GBuffer", [rhi.TEX_TABLE(table, 20)], (1, 1, 1))
            cl.close()
        finally:
            cl.release(); depth.release(); target.release()
        table.clear(1)
        vis, g, mot, _ = _dispatch(dev, k, scene, S.RENDER, mats, table)
    finally:
        table.release(); writable.release()
        for t in made:
            t.release()
    rvis, rg, rmot, _ = _reference(vr, mt, k, scene, S.RENDER, mats, textures + [None])
    same(vis, rvis, "texels"); same(g, rg, "GBufferA after the refusals"); same(mot, rmot, "motion")


# ---- through the glTF loader, FrameDriver and the host mirror -------------------------------------------------------------------
def _loaded(oracle):
    from toyrenderer_amd import gltf_lite
    g, blobs, images = S.textured_gltf()
    s = gltf_lite.load(g, blobs, lods=False, images=images)
    inst = gltf_lite.apply_materials(s)
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    sc = dict(s.as_oracle()); sc["instances"] = inst
    return s, sc, inst, gltf_lite.view_of(s.cameras[0], S.RENDER)


def _frame_reference(oracle, vr, mt, s, sc, view, materials, textures):
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    ref = oracle.frame(sc, view.as_dict(), oracle.HzbTexture(*view.hzb_dims), np.zeros((view.renderH, view.renderW), np.float32), cullingFlags=7,
                       record_capacity=4096, raster=(I.world_to_clip(view.worldToView, view.viewToClip), *geo_v))
    k = consts(view)
    geo = VR.Geometry(sc, *geo_v)
    vis, _ = VR.frame_visibility(vr, k, geo, ref, view.renderW, view.renderH)
    recs = [ref.records[i] if ref.passRan[i] else None for i in range(4)]
    lsts = [ref.visibleList[i] if ref.passRan[i] else None for i in range(4)]
    g, m, taps = MT.gbuffer(mt, k, geo, recs, lsts, vis, materials, [MT.Texture(*t) for t in textures])
    return vis, g, VR.to_half_bits(m), taps


def test_a_textured_gltf_through_the_driver_and_the_facade(dev, oracle, vr, mt):
    """gltf_lite.load(images=...) -> GpuScene.set_textures / set_materials -> FrameDriver(gbuffer=True), which binds the table by
    itself, and -> host.Renderer.load_textures / load_materials / set_gbuffer: GBufferA and the motion target of both equal the
    restatement in every word; the four materials (all textures, a clamped base colour, none, one texel) all show."""
    from toyrenderer_amd import host
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    s, sc, inst, view = _loaded(oracle)
    vis_ref, g_ref, m_ref, taps = _frame_reference(oracle, vr, mt, s, sc, view, s.materials, s.textures)
    cov = vis_ref != 0
    assert cov.sum() > 1200 and (taps[cov][:, 0] > 0).sum() > 600 and (taps[cov][:, 1] > 0).sum() > 200 and (taps[cov].max(1) == 0).sum() > 100
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(s.vertices, s.meshletVertexIds, s.meshletTriangles)
    with pytest.raises(ValueError, match="texture"):
        gs.set_materials(s.materials)                                    # before set_textures: the indices name nothing
    assert gs.set_textures(s.textures) == list(range(len(s.textures)))
    gs.set_materials(s.materials)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, gbuffer=True)
    try:
        dev.profile_reset(); dev.profile_enable(True)
        try:
            drv.record(); drv.run(); drv.results()
            names = {n for n in dev.profile() if n.startswith("basepass_PS")}
        finally:
            dev.profile_enable(False)
        assert names == {"basepass_PS_Main_GBuffer#textured"}
        same(drv.visibility.download_mip(0), vis_ref, "driver: texels")
        same(drv.gbufferA.download_mip(0), g_ref, "driver: GBufferA")
        same(drv.motion.download_mip(0).view(np.uint16), m_ref, "driver: motion")
    finally:
        drv.release(); gs.release()
    with host_renderer(s, inst, (s.vertices, s.meshletVertexIds, s.meshletTriangles), render=S.RENDER, max_groups=4096) as r:
        with pytest.raises(host.HostError, match="texture"):
            r.load_materials(s.materials)                                # no texture created yet
        with pytest.raises(host.HostError, match="format"):
            r.create_material_texture(s.textures[0][0], 7)
        with pytest.raises(host.HostError, match="bytes"):
            r.create_material_texture(s.textures[0][0][:1] + s.textures[0][0][:1], 10)
        assert r.load_textures(s.textures) == list(range(len(s.textures)))
        streamed = s.materials.copy(); streamed["m_AlbedoTexture"]["m_MinMapTextureDescriptorIndex"][0] = 0
        with pytest.raises(host.HostError, match="texture"):
            r.load_materials(streamed)
        r.load_materials(s.materials)
        r.set_gbuffer(True)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        r.set_camera(view)
        r.frame(); r.results()
        same(r.download_visibility(), vis_ref, "host: texels")
        same(r.download_gbuffer_a(), g_ref, "host: GBufferA")
        r.frame(); r.results()                                           # a second frame: the previous projection is this camera's
        same(r.download_gbuffer_a(), g_ref, "host: GBufferA, second frame")
        same(r.download_motion().view(np.uint16).reshape(m_ref.shape), m_ref, "host: motion")


def test_frames_without_textures_record_the_texture_free_kernel(dev, oracle, vr, mt, gr):
    """The same scene with its texture flags taken off, with the textures still loaded: the frame records exactly the launches of
    a frame that never saw a texture (shader and kernel names and their counts), and GBufferA equals the texture-free reference.
    A texture flag with index 0xFFFFFFFF is still refused, by both upload paths."""
    from toyrenderer_amd import host
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    s, sc, inst, view = _loaded(oracle)
    plain = s.materials.copy(); plain["m_MaterialFlags"] = 0
    profiles = []
    for with_textures in (False, True):
        gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
        gs.set_geometry(s.vertices, s.meshletVertexIds, s.meshletTriangles)
        if with_textures:
            gs.set_textures(s.textures)
        gs.set_materials(plain)
        drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, gbuffer=True)
        try:
            dev.profile_reset(); dev.profile_enable(True)
            try:
                drv.record(); drv.run(); drv.results()
                profiles.append({n: c for n, (c, _) in dev.profile().items()})
            finally:
                dev.profile_enable(False)
            g = drv.gbufferA.download_mip(0)
            bad = plain.copy(); bad["m_MaterialFlags"][1] = I.MaterialFlag_UseAlbedoTexture; bad["m_AlbedoTexture"]["m_DescriptorIndex"][1] = 0xFFFFFFFF
            with pytest.raises(ValueError, match="texture"):
                gs.set_materials(bad)
        finally:
            drv.release(); gs.release()
    assert profiles[0] == profiles[1] and profiles[0]["basepass_PS_Main_GBuffer#main"] == 1 and not any("textured" in n for n in profiles[1])
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    ref = oracle.frame(sc, view.as_dict(), oracle.HzbTexture(*view.hzb_dims), np.zeros((view.renderH, view.renderW), np.float32), cullingFlags=7,
                       record_capacity=4096, raster=(I.world_to_clip(view.worldToView, view.viewToClip), *geo_v))
    k = consts(view)
    geo = VR.Geometry(sc, *geo_v)
    vis_ref, _ = VR.frame_visibility(vr, k, geo, ref, *S.RENDER)
    g_ref, _ = GR.frame_gbuffer(gr, k, geo, ref, vis_ref, plain)
    same(g, g_ref, "GBufferA of the texture-free frame")
    r = host.Renderer(render=S.RENDER, max_groups=4096)
    try:
        r.load_scene(inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
        r.load_textures(s.textures[:1])
        with pytest.raises(host.HostError, match="texture"):
            r.load_materials(bad)
    finally:
        r.shutdown()
