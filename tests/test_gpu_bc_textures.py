"""Block-compressed material textures on the GPU (csrc/material_textures.hip.h's fetchQuad): a BC texture samples, in every pass
that samples material textures, exactly as its decoded twin would.  The twins are decoded by tests/bc_ref.c; the references are the
existing ones, tests/material_textures_ref.c and tests/alpha_test_ref.c, run on the twins; every word is compared, nothing excluded.
Then the round trips and refusals of the back end, and the host mirror's two ways in."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import alpha_test_ref as AT  # noqa: E402
import alpha_test_scenes as A  # noqa: E402
import bc_blocks as B  # noqa: E402
import bc_passes as P  # noqa: E402
import bc_ref  # noqa: E402
import material_texture_scenes as S  # noqa: E402
import material_textures_ref as MT  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from suite_support import at, dev, host_renderer, mt, same, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import consts  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = S.ALBEDO | S.NORMAL | S.MR | S.EMISSIVE
EMIT = (2.0, 0.5, 4.0)


@pytest.fixture(scope="module")
def bc(tmp_path_factory):
    return bc_ref.load(tmp_path_factory.mktemp("bc_ref"))


# ---- 1. GBufferA ------------------------------------------------------------------------------------------------------------------
# (width, height, levels, the formats of the albedo, normal, metallic-roughness and emissive textures): every size at which the
# fetch can go wrong, and between them every format in a slot that decodes through the sRGB table and in one that does not
SIZES = [(1, 1, 1, (B.BC1_SRGB, B.BC5, B.BC4, B.BC3_SRGB)),            # a single texel
         (4, 4, 3, (B.BC2_SRGB, B.BC5, B.BC1, B.BC1_SRGB)),            # one block per level
         (5, 7, 3, (B.BC3_SRGB, B.BC5, B.BC3, B.BC2)),                 # edge blocks, their padding texels filled
         (8, 8, 4, (B.BC1, B.BC3, B.BC2, B.BC2_SRGB)),                 # several blocks per level
         (20, 12, 5, (B.BC1_SRGB, B.BC5, B.BC4, B.BC3_SRGB)),          # non-square
         (64, 4, 7, (B.BC3, B.BC1, B.BC5, B.BC1_SRGB))]                # one block row


def _quads():
    """Magnified (a texel covers many pixels), minified (the footprint is larger than the texture), and wrap and clamp with uv in
    [-1.5, 2.5], rotated a little so that both derivatives have two components; materials 0 (wrap) and 1 (clamp)."""
    c, s = np.cos(0.3), np.sin(0.3)
    turn = np.array([[c, s, 0, 0], [-s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return [S.facing(z=-1.2, half=0.3, uv_lo=0.2, uv_hi=0.45, material=0, centre=(-0.45, 0.25)),
            S.facing(z=-30.0, half=5.0, uv_lo=0.0, uv_hi=64.0, material=0, centre=(7.0, 5.0)),
            S.facing(z=-3.0, half=0.42, uv_lo=-1.5, uv_hi=2.5, material=0, centre=(-0.55, -0.7), world=turn),
            S.facing(z=-3.0, half=0.42, uv_lo=-1.5, uv_hi=2.5, material=1, centre=(0.75, -0.55), world=turn)]


def _owners(scene, vis):
    _, _, pos, _ = VR.decode(vis)
    return np.where(vis != 0, scene[4]["m_InstanceConstIdx"][scene[5][pos] >> 5], 99)


def _both(dev, vr, mt, bc, scene, materials, textures, what):
    """Runs the scene on the GPU with `textures` and in the reference with their twins; every word equal.  Returns (vis, taps)."""
    k = consts(S.view())
    table, made = P.upload(dev, textures)
    try:
        vis, g, mot, names = P.resolve(dev, k, scene, S.RENDER, materials, table)
    finally:
        table.release()
        for t in made:
            t.release()
    rvis, rg, rmot, taps = P.reference(vr, mt, k, scene, S.RENDER, materials, P.twins(bc, textures))
    same(vis, rvis, what + ": visibility texels")
    same(g, rg, what + ": GBufferA")
    same(mot, rmot, what + ": motion")
    assert names == ["basepass_PS_Main_GBuffer#textured"], names
    assert np.all(g[vis == 0] == P.FILL), what + ": nothing drawn, nothing written"
    return vis, taps


@pytest.mark.parametrize("w, h, levels, formats", SIZES, ids=[f"{s[0]}x{s[1]}" for s in SIZES])
def test_gbuffer_equals_the_reference_on_the_twins(dev, vr, mt, bc, w, h, levels, formats):
    """All four slots bound from BC textures made of the generator's blocks; the quads, then the grazing floor (anisotropic)."""
    assert levels == min(B.full_chain(w, h), levels) and (levels == B.full_chain(w, h) or (w, h) == (4, 4))
    textures = [(B.block_mips(10 + i, w, h, levels, f), f) for i, f in enumerate(formats)]
    mats = np.concatenate([S.material(flags=ALL, indices=(0, 1, 2, 3), emissive=EMIT), S.material(flags=ALL, indices=(0, 1, 2, 3), emissive=EMIT, wrap=(0, 0, 0, 0))])
    scene = S.build(_quads())
    vis, taps = _both(dev, vr, mt, bc, scene, mats, textures, f"{w} x {h} quads")
    owner = _owners(scene, vis)
    assert all((owner == i).sum() > 60 for i in range(4)), [(owner == i).sum() for i in range(4)]
    assert np.all(taps[vis != 0] > 0), "every slot of every covered pixel was sampled"
    if w == h:
        assert np.all(taps[owner == 0][:, 0] <= 2), "magnified: a square texture on a facing square has an isotropic footprint"
    scene = S.build([S.floor(material=0)])
    vis, taps = _both(dev, vr, mt, bc, scene, mats, textures, f"{w} x {h} floor")
    n = np.unique(taps[vis != 0][:, 0])
    assert (vis != 0).sum() > 1000 and n.max() >= 10 and len(n) >= 8, n      # the reference's own N takes many values


def test_one_table_mixes_the_formats_within_a_wave(dev, vr, mt, bc):
    """Two rows of seven quads of eight pixels side by side, each with its own entry of one table: BC1, BC1_SRGB, BC3_SRGB, BC5, BC4,
    RGBA8 and SRGBA8, in all four slots, at 8 x 8 with four levels and (the BC ones of the upper row) at 5 x 7 with three.  An
    8 x 8 pixel square holds pixels of two or three quads, so lanes of one wave fetch through different formats in the same call."""
    formats = (B.BC1, B.BC1_SRGB, B.BC3_SRGB, B.BC5, B.BC4, S.RGBA8, S.SRGBA8)
    textures = []
    for (w, h, levels) in ((8, 8, 4), (5, 7, 3)):
        for i, f in enumerate(formats):
            textures.append((S.random_mips(40 + i, w, h, levels), f) if f in (S.RGBA8, S.SRGBA8) else (B.block_mips(40 + i, w, h, levels, f), f))
    quads, mats = [], []
    for row in range(2):
        for i in range(7):
            d = 7 * row + i
            quads.append(S.facing(z=-3.0, half=0.17, uv_lo=-0.5, uv_hi=1.5, material=d, grid=1, centre=(-1.02 + 0.34 * i, 0.45 - 0.9 * row)))
            mats.append(S.material(flags=ALL, indices=(d, (d + 1) % 14, (d + 2) % 14, (d + 3) % 14), emissive=EMIT, wrap=(i & 1, 1, 0, 1)))
    scene = S.build(quads)
    vis, taps = _both(dev, vr, mt, bc, scene, np.concatenate(mats), textures, "mixed table")
    owner = _owners(scene, vis)
    assert all((owner == i).sum() > 40 for i in range(14)), [(owner == i).sum() for i in range(14)]
    H, W = owner.shape
    most = max(len(set(owner[y:y + 8, x:x + 8].ravel()) - {99}) for y in range(0, H, 8) for x in range(0, W, 8))
    assert most >= 2, "some 8 x 8 square of the resolve holds pixels of more than one quad"


# ---- 2. alpha -----------------------------------------------------------------------------------------------------------------------
# the table of tests/alpha_test_scenes.py (0: 8 x 8, full chain; 1: 5 x 3, three levels; 2: 4 x 4, one level) in the three formats
# with an alpha channel, rotated: every format at every size; BC1's alpha is its punch-through (three-colour mode, index 3)
ALPHA_TABLES = [(B.BC1, B.BC2, B.BC3), (B.BC2, B.BC3, B.BC1), (B.BC3, B.BC1, B.BC2)]


def _alpha_textures(formats, srgb):
    sizes = ((8, 8, 4), (5, 3, 3), (4, 4, 1))
    return [(B.block_mips(60 + i, w, h, levels, f), f + int(srgb)) for i, ((w, h, levels), f) in enumerate(zip(sizes, formats))]


def _gpu_scene(dev, sc, raytracing=False):
    from toyrenderer_amd.frame import GpuScene
    gs = GpuScene(dev, sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
    gs.set_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
    gs.set_textures(sc["textures"])
    gs.set_materials(sc["materials"])
    if raytracing:
        gs.set_raytracing(sc["indices"], sc["index_counts"])
    return gs


def _frame(dev, sc, **kw):
    from toyrenderer_amd.frame import FrameDriver
    gs = _gpu_scene(dev, sc)
    drv = FrameDriver(dev, gs, A.view(), record_capacity=4096, culling_flags=1, alpha_test=True, **kw)
    try:
        dev.profile_reset(); dev.profile_enable(True)
        try:
            drv.record(); drv.run(); drv.results()
            names = set(dev.profile())
        finally:
            dev.profile_enable(False)
        out = dict(depth=drv.depth.download_mip(0).view(np.uint32), names=names)
        if drv.visibility is not None:
            out["vis"] = drv.visibility.download_mip(0)
        return out
    finally:
        drv.release(); gs.release()


@pytest.mark.parametrize("formats", ALPHA_TABLES, ids=["BC1-BC2-BC3", "BC2-BC3-BC1", "BC3-BC1-BC2"])
def test_both_rasters_discard_by_the_decoded_alpha(dev, oracle, at, bc, formats):
    """The depth raster on the _UNORM formats and the visibility raster on the same bytes as _SRGB, against tests/alpha_test_ref.c
    on the twins: depth and visibility texels, every word; and the two rasters' depths equal each other, so the same bytes give
    the same alpha whatever the transfer function of the colour."""
    view = A.view()
    got = {}
    for srgb, kw in ((False, dict(raster_depth=True)), (True, dict(visibility=True))):
        tex = _alpha_textures(formats, srgb)
        sc = A.standard(tex=tex)
        got[srgb] = _frame(dev, sc, **kw)
        (ref, vis, depth), = AT.frames(oracle, at, dict(sc, textures=P.twins(bc, tex)), view, 1, True, 1)
        stem = "basepass_MS_Main_" + ("visibility" if srgb else "depth") + " ALPHA_MASK_MODE=1"
        assert {n for n in got[srgb]["names"] if n.startswith(stem)} == {stem + "#main", stem + "#tiles"}, got[srgb]["names"]
        same(got[srgb]["depth"], depth.view(np.uint32), f"{formats}, sRGB {srgb}: depth")
        if srgb:
            same(got[srgb]["vis"], vis, f"{formats}: visibility texels")
            _, slot, _, _ = VR.decode(vis)
            solid, = AT.frames(oracle, at, dict(sc, textures=P.twins(bc, tex)), view, 1, False, 1)
            kept, drawn = (slot == 2).sum(), (VR.decode(solid[1])[1] == 2).sum()
            assert 300 < kept < drawn - 300, (kept, drawn)              # the alpha test both keeps and discards
    same(got[True]["depth"], got[False]["depth"], f"{formats}: the same bytes as _UNORM and as _SRGB")


def _shadow(dev, at, bc, fmt, base):
    """The shadow mask of the cut-out scene with the caster's texture as `fmt` (blocks generated for `base`), checked against the
    reference on the twin."""
    from toyrenderer_amd.frame import FrameDriver
    tex = A.textures()
    tex[A.CHECKER] = (B.block_mips(70, 8, 8, 4, base), fmt)
    sc = A.shadow_scene()
    sc["textures"] = tex
    acc = SR.Accel(sc)
    gs = _gpu_scene(dev, sc, raytracing=True)
    settings = dict(noise=SS.noise_image(3), ray_start_offset=0.01, soft=False, sun_angular_diameter=3.0)
    try:
        drv = FrameDriver(dev, gs, A.view(), record_capacity=4096, culling_flags=1, gbuffer=True, shadows=settings, dir_light=(SS.unit((0.15, 0.9, -0.25)), 2.0), alpha_test=True)
        try:
            H, W = A.RENDER[::-1]
            drv.shadow_mask_texture.upload_mip(0, np.full((H, W), SR.SENTINEL8, np.uint8))
            drv.linear_view_depth.upload_mip(0, np.full((H, W), SR.SENTINEL16, np.uint16))
            drv.frame_counter = 5
            dev.profile_reset(); dev.profile_enable(True)
            try:
                drv.record(); drv.run(); drv.results()
                names = set(dev.profile())
            finally:
                dev.profile_enable(False)
            assert {n.split("#")[1] for n in names if n.startswith("shadowmask_CS_ShadowMask")} == {"textured"}, names
            depth, gb = drv.depth.download_mip(0), drv.gbufferA.download_mip(0)
            want, want_lvd = AT.trace(at, drv.shadow_consts, acc, depth, gb, settings["noise"], P.twins(bc, tex))
            same(drv.download_shadow_mask(), want, f"format {fmt}: mask")
            same(drv.linear_view_depth.download_mip(0), want_lvd, f"format {fmt}: linear view depth")
            solid, _ = AT.trace(at, drv.shadow_consts, acc, depth, gb, settings["noise"], None)
            _, slot, _, _ = VR.decode(drv.visibility.download_mip(0))
            shadowed = (slot == 0) & (solid == 0)                      # the floor texels in the solid card's shadow
            assert shadowed.sum() > 300 and (want[shadowed] == 255).sum() > 40 and (want[shadowed] == 0).sum() > 40, (shadowed.sum(), (want[shadowed] == 255).sum())
            return want
        finally:
            drv.release()
    finally:
        gs.release()


@pytest.mark.parametrize("fmt", [B.BC1, B.BC2, B.BC3], ids=["BC1", "BC2", "BC3"])
def test_sun_rays_through_a_bc_cut_out(dev, at, bc, fmt):
    """The cut-out caster of tests/alpha_test_scenes.py above a floor, its texture in a BC format: the shadow mask and the linear
    view depth equal tests/alpha_test_ref.c's brute force on the twin, no differing texel, and the floor below the card shows both
    lit and shadowed texels.  BC3: the same bytes as BC3_UNORM_SRGB cast the same shadow."""
    mask = _shadow(dev, at, bc, fmt, fmt)
    if fmt == B.BC3:
        same(_shadow(dev, at, bc, B.BC3_SRGB, B.BC3), mask, "the same bytes as _UNORM and as _SRGB")


# ---- 3. round trips and refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", range(B.BC1, B.BC5 + 1))
def test_every_level_round_trips_and_mip_info_answers_texels(dev, fmt):
    from toyrenderer_amd import rhi
    nb = rhi.format_block_bytes(fmt)
    for w, h in ((5, 7), (20, 12), (1, 1)):
        levels = B.full_chain(w, h)
        mips = B.block_mips(80, w, h, levels, fmt)
        t = dev.create_sampled_texture(mips, fmt, "round trip")
        try:
            assert (t.w, t.hgt, t.mips, t.format) == (w, h, levels, fmt)
            end = 0
            for k in range(levels):
                mw, mh, off = t.mip_info(k)
                assert (mw, mh) == (max(w >> k, 1), max(h >> k, 1)) and off % 256 == 0 and off >= end, (k, mw, mh, off)
                got = t.download_mip(k)
                assert got.shape == ((mh + 3) // 4, (mw + 3) // 4, nb) and got.tobytes() == mips[k].tobytes(), (w, h, k)
                end = off + got.nbytes
            with pytest.raises(rhi.TrhipError, match="bytes, got"):
                t.upload_mip(0, np.zeros(mips[0].size + nb, np.uint8))
            with pytest.raises(rhi.TrhipError, match="bytes, got"):
                t.upload_mip(levels - 1, np.zeros(4, np.uint8))
            with pytest.raises(rhi.TrhipError, match="bytes, got"):
                rhi._check(rhi.load().trhip_texture_download(t.h, 0, np.zeros(4, np.uint8).ctypes.data, 4))
            with pytest.raises(rhi.TrhipError, match="mip"):
                t.mip_info(levels)
            t.upload_mip(0, bytes(mips[0].size))                        # bytes are taken too
            assert not t.download_mip(0).any()
        finally:
            t.release()


def test_refusals_name_their_cause(dev):
    from toyrenderer_amd import rhi
    bc1 = B.block_mips(81, 8, 8, 2, B.BC1)
    for fmt in rhi.BC_FORMATS:
        with pytest.raises(rhi.TrhipError, match="cannot be an array"):
            dev.create_texture_array(8, 8, 2, fmt, "a BC array")
        with pytest.raises(rhi.TrhipError, match="no UAV or render-target bit"):
            dev.create_texture(8, 8, 1, fmt, "a BC UAV", uav=True)
    d = rhi.TextureDesc(8, 8, 1, B.BC3, rhi.TEXTURE_RENDER_TARGET, 0, b"a BC render target")
    hd = rhi.C.c_void_p()
    with pytest.raises(rhi.TrhipError, match="no UAV or render-target bit"):
        rhi._check(rhi.load().trhip_texture_create(dev.h, rhi.C.byref(d), rhi.C.byref(hd)))
    with pytest.raises(rhi.TrhipError, match="bad dimensions"):
        dev.create_texture(8, 8, 17, B.BC1, "too many levels", uav=False)
    with pytest.raises(ValueError, match="BlockMips"):
        dev.create_sampled_texture([np.zeros((8, 8, 4), np.uint8)], B.BC1)
    t = dev.create_sampled_texture(bc1, B.BC1, "a BC1 texture")
    same_format = dev.create_texture(8, 8, 2, B.BC1, "another BC1 texture", uav=False)
    srgb = dev.create_texture(8, 8, 2, B.BC1_SRGB, "a BC1_SRGB texture", uav=False)
    rgba = dev.create_texture(8, 8, 2, rhi.FORMAT_RGBA8_UNORM, "an RGBA8 texture", uav=False)
    depth = dev.create_texture(8, 8, 1, rhi.FORMAT_R32_FLOAT, "depth")
    target = dev.create_texture(8, 8, 1, rhi.FORMAT_R11G11B10_FLOAT, "target")
    table = dev.create_texture_table(1)
    cl = dev.create_command_list()
    try:
        table.set(0, t)                                                  # the table takes it
        cl.open()
        with pytest.raises(rhi.TrhipError, match="block-compressed texture has no clear"):
            cl.clear_texture_f32(t, 0.0)
        with pytest.raises(rhi.TrhipError, match="block-compressed texture has no clear"):
            cl.clear_texture_u32(t, 0)
        for other in (srgb, rgba):
            with pytest.raises(rhi.TrhipError, match="its own format only"):
                cl.copy_texture(other, t)
            with pytest.raises(rhi.TrhipError, match="its own format only"):
                cl.copy_texture(t, other)
        with pytest.raises(rhi.TrhipError, match="through the texture table only"):
            cl.dispatch("sky_PS_HosekWilkieSky", [rhi.TEX_SRV(0, t), rhi.TEX_UAV(0, target, 0)], (1, 1, 1))
        with pytest.raises(rhi.TrhipError, match="through the texture table only"):
            cl.dispatch("sky_PS_HosekWilkieSky", [rhi.TEX_SRV(0, depth), rhi.TEX_UAV(0, t, 0)], (1, 1, 1))
        with pytest.raises(rhi.TrhipError, match="through the texture table only"):
            cl.dispatch("basepass_PS_Main_GBuffer", [rhi.TEX_SRV(18, t)], (1, 1, 1))
        cl.copy_texture(same_format, t)                                  # whole chains of one format are copied
        cl.close()
        dev.execute(cl); dev.wait_idle()
        for k in range(2):
            assert same_format.download_mip(k).tobytes() == bc1[k].tobytes()
    finally:
        cl.release(); table.release()
        for x in (t, same_format, srgb, rgba, depth, target):
            x.release()


# ---- 4. the host mirror -----------------------------------------------------------------------------------------------------------------
def test_host_paths_equal_the_python_driver(dev, oracle, vr, mt, bc):
    """tests/material_texture_scenes.py's glTF with its images as .dds files (BC1, BC5, a DX10 BC3): FrameDriver on
    gltf_lite.load's textures equals the reference on the twins, and the host mirror gives the same GBufferA both through
    trhost_create_material_texture with block bytes and through trhost_create_material_texture_dds."""
    from toyrenderer_amd import gltf_lite, host
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    g, blobs, _ = S.textured_gltf()
    files = [B.make_dds(8, 8, list(B.block_mips(1, 8, 8, 4, B.BC1)), fourcc=b"DXT1"),
             B.make_dds(12, 5, list(B.block_mips(2, 12, 5, 4, B.BC5)), fourcc=b"ATI2"),
             B.make_dds(1, 1, list(B.block_mips(3, 1, 1, 1, B.BC3)), dxgi=78)]
    s = gltf_lite.load(g, blobs, lods=False, images=files)
    inst = gltf_lite.apply_materials(s)
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    sc = dict(s.as_oracle()); sc["instances"] = inst
    view = gltf_lite.view_of(s.cameras[0], S.RENDER)
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    ref = oracle.frame(sc, view.as_dict(), oracle.HzbTexture(*view.hzb_dims), np.zeros((view.renderH, view.renderW), np.float32), cullingFlags=7,
                       record_capacity=4096, raster=(I.world_to_clip(view.worldToView, view.viewToClip), *geo_v))
    k = consts(view)
    geo = VR.Geometry(sc, *geo_v)
    vis_ref, _ = VR.frame_visibility(vr, k, geo, ref, view.renderW, view.renderH)
    recs = [ref.records[i] if ref.passRan[i] else None for i in range(4)]
    lsts = [ref.visibleList[i] if ref.passRan[i] else None for i in range(4)]
    g_ref, _, taps = MT.gbuffer(mt, k, geo, recs, lsts, vis_ref, s.materials, [MT.Texture(*t) for t in P.twins(bc, s.textures)])
    assert (taps[vis_ref != 0][:, 0] > 0).sum() > 600
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(*geo_v)
    assert gs.set_textures(s.textures) == list(range(len(s.textures)))
    gs.set_materials(s.materials)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, gbuffer=True)
    try:
        drv.record(); drv.run(); drv.results()
        same(drv.visibility.download_mip(0), vis_ref, "driver: texels")
        want = drv.gbufferA.download_mip(0)
        same(want, g_ref, "driver: GBufferA")
    finally:
        drv.release(); gs.release()
    # (file, sRGB) of every entry of s.textures, in order: what a caller of the DDS entry point passes
    by_file = [(0, 1), (0, 0), (1, 0), (1, 0), (2, 1)]
    assert [(I.parse_dds(files[f])[0][0], I.srgb_variant(I.parse_dds(files[f])[1], srgb)) for f, srgb in by_file] == [(bytes(m[0]), fmt) for m, fmt in s.textures]
    for way in ("block bytes", "dds"):
        with host_renderer(s, inst, geo_v, render=S.RENDER, max_groups=4096) as r:
            if way == "block bytes":
                with pytest.raises(host.HostError, match="bytes"):
                    r.create_material_texture(I.BlockMips(list(s.textures[0][0])[:2], 8, 8), B.BC3)
                assert r.load_textures(s.textures) == list(range(len(s.textures)))
            else:
                with pytest.raises(host.HostError, match="BC7"):
                    r.create_material_texture_dds(B.make_dds(8, 8, [b"\0" * 64], dxgi=98), True)
                with pytest.raises(host.HostError, match="shorter than its"):
                    r.create_material_texture_dds(files[0][:-1], True)
                assert [r.create_material_texture_dds(files[f], bool(srgb)) for f, srgb in by_file] == list(range(len(by_file)))
            r.load_materials(s.materials)
            r.set_gbuffer(True)
            r.set_culling(7)
            r.set_node_transforms(s.nodes)
            r.set_camera(view)
            r.frame(); r.results()
            same(r.download_visibility(), vis_ref, f"host, {way}: texels")
            same(r.download_gbuffer_a(), want, f"host, {way}: GBufferA")
