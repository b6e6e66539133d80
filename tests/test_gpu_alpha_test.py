"""The alpha test on the GPU: "basepass_MS_Main_depth ALPHA_MASK_MODE=1" and "basepass_MS_Main_visibility ALPHA_MASK_MODE=1"
(csrc/k_raster.hip) and the textured alpha test of "shadowmask_CS_ShadowMask" (csrc/k_shadowmask.hip), through
FrameDriver(alpha_test=True) and the host mirror, every word of every pixel against tests/alpha_test_ref.c.

The rasters' path switches under the alpha test (kSmallBox, the tile rounds, kBinCapacity, the queue-overflow path with 2^20 +
65 536 queued triangles, the grid stride, the early-out under discards) and rules 5 and 6 of the convention are in
tests/test_gpu_alpha_raster_paths.py; this file's scenes have one bin, one collect round and nothing near a capacity."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import alpha_test_ref as AT  # noqa: E402
import alpha_test_scenes as A  # noqa: E402
import material_textures_ref as MT  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from suite_support import at, dev, mt, same, sm, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import consts  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
ALPHA = " ALPHA_MASK_MODE=1"


def _gpu_scene(dev, sc, raytracing=False):
    from toyrenderer_amd.frame import GpuScene
    gs = GpuScene(dev, sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
    gs.set_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
    gs.set_textures(sc["textures"])
    gs.set_materials(sc["materials"])
    if raytracing:
        gs.set_raytracing(sc["indices"], sc["index_counts"])
    return gs


def _run(dev, drv):
    """One frame of the driver: its images and the names the profile saw."""
    dev.profile_reset(); dev.profile_enable(True)
    try:
        drv.record(); drv.run(); drv.results()
        names = set(dev.profile())
    finally:
        dev.profile_enable(False)
    out = dict(depth=drv.depth.download_mip(0).view(np.uint32), names=names)
    if drv.visibility is not None:
        out["vis"] = drv.visibility.download_mip(0)
        out["motion"] = drv.motion.download_mip(0).view(np.uint16)
    if drv.gbufferA is not None:
        out["gbuffer"] = drv.gbufferA.download_mip(0)
    return out


def _frames(dev, sc, count=1, **kw):
    from toyrenderer_amd.frame import FrameDriver
    gs = _gpu_scene(dev, sc)
    drv = FrameDriver(dev, gs, A.view(), record_capacity=4096, **kw)
    try:
        return [_run(dev, drv) for _ in range(count)]
    finally:
        drv.release(); gs.release()


def _raster_names(names):
    return {n.split("#")[0] for n in names if n.startswith("basepass_MS_Main")}


# ---- 1. the rasters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [3, 1], ids=["early+late", "early only"])
@pytest.mark.parametrize("mode", ["depth", "gbuffer"])
def test_rasters_equal_the_reference(dev, oracle, at, mt, mode, flags):
    """Two frames of the standard scene.  depth: FrameDriver(raster_depth=True).  gbuffer: FrameDriver(gbuffer=True): the
    visibility rasters, and GBufferA and the motion target resolved from what they left (the textured resolve).  Every word of
    every pixel, no exclusions.  flags 3: frustum and occlusion culling, so the alpha-mask instances go through the early and the
    late pass, and frame 2 culls against the HZB of frame 1's alpha-tested depth (the quad behind the checker passes its early
    cull only then: tests/test_alpha_test_ref.py); flags 1: the early pass alone."""
    sc = A.standard()
    view = A.view()
    kw = dict(raster_depth=True) if mode == "depth" else dict(gbuffer=True)
    got = _frames(dev, sc, 2, culling_flags=flags, alpha_test=True, **kw)
    want = AT.frames(oracle, at, sc, view, flags, True, 2)
    k = consts(view)
    geo = VR.Geometry(sc, sc["vertices"], sc["vertexIds"], sc["triangles"])
    table = [MT.Texture(*t) for t in sc["textures"]]
    stem = "basepass_MS_Main_" + ("depth" if mode == "depth" else "visibility")
    for f, (g, (ref, vis, depth)) in enumerate(zip(got, want)):
        what = f"{mode}, flags {flags}, frame {f}"
        assert _raster_names(g["names"]) == {stem, stem + ALPHA}, g["names"]
        assert {n for n in g["names"] if n.startswith(stem + ALPHA)} == {stem + ALPHA + "#main", stem + ALPHA + "#tiles"}
        same(g["depth"], depth.view(np.uint32), what + ": depth")
        if mode == "depth":
            continue
        same(g["vis"], vis, what + ": visibility texels")
        recs = [ref.records[s] if ref.passRan[s] else None for s in range(4)]
        lsts = [ref.visibleList[s] if ref.passRan[s] else None for s in range(4)]
        gb, m, taps = MT.gbuffer(mt, k, geo, recs, lsts, vis, sc["materials"], table)
        same(g["gbuffer"], gb, what + ": GBufferA")
        same(g["motion"], VR.to_half_bits(m), what + ": motion")
        assert (taps[..., 0] > 0).sum() > 1500 and "basepass_PS_Main_GBuffer#textured" in g["names"]


# ---- 2. the metamorphic checks of tests/test_alpha_test_ref.py, on the GPU -------------------------------------------------------------
def test_an_opaque_texture_changes_nothing(dev):
    mats = A.materials()
    mats["m_ConstAlbedo"][:, 3] = 1.0
    sc = A.standard(mats, A.with_uniform_alpha(A.textures(), 255))
    off, = _frames(dev, sc, culling_flags=1, visibility=True, alpha_test=False)
    on, = _frames(dev, sc, culling_flags=1, visibility=True, alpha_test=True)
    assert _raster_names(on["names"]) == {"basepass_MS_Main_visibility", "basepass_MS_Main_visibility" + ALPHA}
    for name in ("depth", "vis", "motion"):
        same(on[name], off[name], "all-255 textures: " + name)
    assert (VR.decode(on["vis"])[1] == 2).sum() > 1500


def test_a_transparent_texture_removes_the_instances(dev):
    mats = A.materials()
    mats["m_ConstAlbedo"][[A.M_CONST_ABOVE, A.M_CONST_BELOW], 3] = 0.25
    sc = A.standard(mats, A.with_uniform_alpha(A.textures(), 0))
    on, = _frames(dev, sc, culling_flags=1, visibility=True, alpha_test=True)
    bare, = _frames(dev, A.without_alpha_instances(sc), culling_flags=1, visibility=True, alpha_test=True)
    assert _raster_names(bare["names"]) == {"basepass_MS_Main_visibility"}
    for name in ("depth", "vis", "motion"):
        same(on[name], bare[name], "all-0 textures: " + name)


def test_the_tie_is_kept_and_the_next_cutoff_discards(dev):
    kept, gone = A.tie_scene(A.TIE), A.tie_scene(np.nextafter(A.TIE, F(1)))
    solid, = _frames(dev, kept, culling_flags=1, visibility=True, alpha_test=False)
    wall, = _frames(dev, A.without_alpha_instances(kept), culling_flags=1, visibility=True)
    a, = _frames(dev, kept, culling_flags=1, visibility=True, alpha_test=True)
    b, = _frames(dev, gone, culling_flags=1, visibility=True, alpha_test=True)
    for name in ("depth", "vis"):
        same(a[name], solid[name], "alpha == cutoff: kept whole: " + name)
        same(b[name], wall[name], "the next cutoff: gone whole: " + name)
    assert (VR.decode(a["vis"])[1] == 2).sum() > 2000


# ---- 3. the option off ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [3, 1])
def test_option_off_draws_solid_cards(dev, oracle, at, vr, flags):
    """alpha_test=False (the default): the shader names of before, and the words of the existing reference without the discard."""
    sc = A.standard()
    view = A.view()
    got, = _frames(dev, sc, culling_flags=flags, visibility=True)
    assert _raster_names(got["names"]) == {"basepass_MS_Main_visibility"}
    ref = oracle.frame(sc, view.as_dict(), oracle.HzbTexture(*view.hzb_dims), np.zeros(A.RENDER[::-1], F), cullingFlags=flags, record_capacity=4096,
                       raster=(I.world_to_clip(view.worldToView, view.viewToClip), sc["vertices"], sc["vertexIds"], sc["triangles"]))
    geo = VR.Geometry(sc, sc["vertices"], sc["vertexIds"], sc["triangles"])
    vis, depth = VR.frame_visibility(vr, consts(view), geo, ref, *A.RENDER)
    same(got["vis"], vis, "texels"); same(got["depth"], depth.view(np.uint32), "depth")
    same(got["motion"], VR.to_half_bits(VR.frame_motion(vr, consts(view), geo, ref, vis)), "motion")


# ---- 4. shadows -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_a_textured_cut_out_casts_the_shadow_of_its_kept_texels(dev, at, sm, soft):
    """The checker cut-out above a floor.  alpha_test=True: the mask equals brute force with textured alpha, no differing texel,
    and the floor shows both lit and shadowed texels below the card.  alpha_test=False: the mask equals today's reference (the
    whole card, m_ConstAlbedo.w >= m_AlphaCutoff), which the new reference without a table restates."""
    from toyrenderer_amd.frame import FrameDriver
    sc = A.shadow_scene()
    acc = SR.Accel(sc)
    gs = _gpu_scene(dev, sc, raytracing=True)
    settings = dict(noise=SS.noise_image(3), ray_start_offset=0.01, soft=soft, sun_angular_diameter=3.0)
    light = SS.unit((0.15, 0.9, -0.25))
    masks = {}
    try:
        for alpha_test in (True, False):
            drv = FrameDriver(dev, gs, A.view(), record_capacity=4096, culling_flags=1, gbuffer=True, shadows=settings, dir_light=(light, 2.0), alpha_test=alpha_test)
            try:
                H, W = A.RENDER[::-1]
                drv.shadow_mask_texture.upload_mip(0, np.full((H, W), SR.SENTINEL8, np.uint8))
                drv.linear_view_depth.upload_mip(0, np.full((H, W), SR.SENTINEL16, np.uint16))
                drv.frame_counter = 5
                g = _run(dev, drv)
                trace = {n.split("#")[1] for n in g["names"] if n.startswith("shadowmask_CS_ShadowMask")}
                assert trace == ({"textured"} if alpha_test else {"main"}), g["names"]
                depth, gb = drv.depth.download_mip(0), drv.gbufferA.download_mip(0)
                want, want_lvd = AT.trace(at, drv.shadow_consts, acc, depth, gb, settings["noise"], sc["textures"] if alpha_test else None)
                same(drv.download_shadow_mask(), want, f"alpha_test {alpha_test}: mask")
                same(drv.linear_view_depth.download_mip(0), want_lvd, f"alpha_test {alpha_test}: linear view depth")
                if not alpha_test:
                    today, _, _ = SR.trace(sm, drv.shadow_consts, acc, depth, gb, settings["noise"], SR.BRUTE)
                    same(want, today, "the reference without a table is today's")
                _, slot, _, _ = VR.decode(g["vis"])
                masks[alpha_test] = (want, slot == 0)
            finally:
                drv.release()
    finally:
        gs.release()
    (on, floor), (off, _) = masks[True], masks[False]
    shadowed = floor & (off == 0)                                     # the floor texels in the solid card's shadow
    assert shadowed.sum() > 300 and (on[shadowed] == 255).sum() > 60 and (on[shadowed] == 0).sum() > 60, (shadowed.sum(), (on[shadowed] == 255).sum())


# ---- 5. the host mirror ---------------------------------------------------------------------------------------------------------------------
def test_host_path_equals_the_python_driver(dev):
    """One frame through trhost_* with trhost_set_alpha_test(1): depth, visibility texels and GBufferA equal FrameDriver's."""
    from toyrenderer_amd import host
    sc = A.standard()
    view = A.view()
    want, = _frames(dev, sc, culling_flags=3, gbuffer=True, alpha_test=True)
    n = len(sc["instances"])
    nodes = np.zeros(n, I.NodeLocalTransform)                         # one node per instance, the identity (as the scene's world matrices)
    nodes["m_ParentNodeIdx"] = 0xFFFFFFFF
    nodes["m_Rotation"][:, 3] = 1.0
    nodes["m_Scale"] = 1.0
    r = host.Renderer(render=A.RENDER, max_groups=4096)
    try:
        r.load_scene(sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
        r.load_nodes(nodes, np.arange(n, dtype=np.uint32))
        r.load_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
        r.load_textures(sc["textures"])
        with pytest.raises(host.HostError, match="rasters are off"):
            r.set_alpha_test(True)
        r.set_raster_depth(True)
        with pytest.raises(host.HostError, match="no materials"):
            r.set_alpha_test(True)
        r.load_materials(sc["materials"])
        r.set_gbuffer(True)
        r.set_alpha_test(True)
        r.set_culling(3)
        r.set_node_transforms(nodes)
        r.set_camera(view)
        r.frame(); r.results()
        same(r.instances(n)["m_WorldMatrix"], sc["instances"]["m_WorldMatrix"], "host: the identity nodes give the scene's matrices")
        same(r.download_depth().view(np.uint32), want["depth"], "host: depth")
        same(r.download_visibility(), want["vis"], "host: texels")
        same(r.download_gbuffer_a(), want["gbuffer"], "host: GBufferA")
        r.set_alpha_test(False)
        r.frame(); r.results()
        assert np.count_nonzero(r.download_visibility() != want["vis"]) > 500, "off again: solid cards"
    finally:
        r.shutdown()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_at_record_time(dev):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    from toyrenderer_amd.rhi import CB, PUSH, SRV, TEX_TABLE, TEX_UAV
    sc = A.standard()
    W, H = A.RENDER
    gs = _gpu_scene(dev, sc)
    bare = GpuScene(dev, sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
    bare.set_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
    try:
        with pytest.raises(ValueError, match="raster_depth"):
            FrameDriver(dev, gs, A.view(), record_capacity=4096, alpha_test=True)
        with pytest.raises(ValueError, match="set_materials"):
            FrameDriver(dev, bare, A.view(), record_capacity=4096, raster_depth=True, alpha_test=True)
    finally:
        bare.release()
    rec, lst = dev.buffer_from(sc["records"], "rec", min_bytes=12), dev.buffer_from(sc["list"], "lst")
    args = dev.create_buffer(12, "drawArgs", stride=12, indirect=True)
    args.upload(np.array([len(sc["list"]), 1, 1], np.uint32))
    depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
    vis = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "VisibilityBuffer")
    writable = dev.create_texture(8, 8, 1, rhi.FORMAT_RGBA8_UNORM, "a UAV-capable texture", uav=True)
    table = dev.create_texture_table(2)
    table.set(0, gs.textures[0]); table.set(1, writable)
    cl = dev.create_command_list()
    try:
        cl.open()
        cb = cl.constant_buffer(consts(A.view()), "BasePassConstants")
        b = [CB(0, cb), SRV(0, gs.instances), SRV(1, gs.vertices), SRV(2, gs.meshData), SRV(4, gs.meshlets), SRV(5, gs.meshletVertexIds), SRV(6, gs.meshletTriangles),
             SRV(7, rec), SRV(9, lst), TEX_UAV(0, depth, 0)]
        for name, extra, push in (("basepass_MS_Main_depth" + ALPHA, [], None),
                                  ("basepass_MS_Main_visibility" + ALPHA, [TEX_UAV(1, vis, 0), PUSH(1)], np.array([2], np.uint32))):
            with pytest.raises(rhi.TrhipError, match=name + ".*t3"):
                cl.dispatch_indirect(name, b + extra, args, push=push)
            with pytest.raises(rhi.TrhipError, match=name + ".*t19.*UAV"):
                cl.dispatch_indirect(name, b + extra + [SRV(3, gs.materials), TEX_TABLE(table)], args, push=push)
            with pytest.raises(rhi.TrhipError, match="t19"):
                cl.dispatch_indirect(name, b + extra + [SRV(3, gs.materials), TEX_TABLE(table, 20)], args, push=push)
        with pytest.raises(rhi.TrhipError, match="texture table"):                  # the plain rasters declare none
            cl.dispatch_indirect("basepass_MS_Main_depth", b + [TEX_TABLE(gs.texture_table)], args)
        cl.close()
    finally:
        cl.release(); table.release(); writable.release(); depth.release(); vis.release(); args.release(); rec.release(); lst.release(); gs.release()
