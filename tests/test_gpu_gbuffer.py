"""GBufferA and the fused motion target ("basepass_PS_Main_GBuffer", csrc/k_gbuffer.hip) on the GPU, every texel and every
word against tests/gbuffer_ref.c: through FrameDriver(gbuffer=True) under all culling flags and the debug views, through
direct dispatches on a near wall with exact ties and on hostile soups, over animated frames through all four pass slots,
through the host mirror, and misuse."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gbuffer_ref as GR  # noqa: E402
from suite_support import compare_frame, dev, gpu_scene, gr, host_renderer, lit_cornell, op_counts, same, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from gbuffer_scenes import hostile_materials, wall, with_normals_and_materials  # noqa: E402
from toyrenderer_amd import gltf_lite, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import city, consts, hostile_soup, inside_view, with_duplicates  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_MODES = (0, 2, 3, 12)


def _random_byte(seeds):
    """uint(QuickRandomFloat(seed) * 255): the LCG in 64-bit integers, the float steps in numpy float32."""
    x = ((np.asarray(seeds, np.uint64) * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFF)).astype(np.float32)
    return (x / np.float32(16777216.0) * np.float32(255.0)).astype(np.uint32)


@pytest.mark.parametrize("flags", range(8))
def test_frames_match_the_reference_under_every_flag(dev, oracle, vr, gr, tmp_path, flags):
    """Two frames of a moving camera, one gbuffer=True driver per debug mode next to a visibility=True driver: GBufferA and
    motion equal the reference in every texel; the motion target, depth, HZB, every cull output, the visibility texels
    and the pipeline statistics equal the visibility=True run."""
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    v, sc, mats = with_normals_and_materials(s, sc)
    gs = gpu_scene(dev, s, sc["instances"], v, mats)
    cam = s.cameras[0]
    render = (640, 360)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V0 = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    view = synth.View(V0, V0.copy(), P, float(np.float32(cam.znear)), *render)
    base = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=flags, visibility=True)
    drivers = {m: FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=flags, gbuffer=True, debug_mode=m) for m in DEBUG_MODES}
    queries = {m: dev.create_pipeline_stats() for m in (None,) + DEBUG_MODES}
    geo = VR.Geometry(sc, v, s.meshletVertexIds, s.meshletTriangles)
    hzb = oracle.HzbTexture(*view.hzb_dims)
    depth = np.zeros((render[1], render[0]), np.float32)
    prevV = V0
    try:
        for f, eye in enumerate([(0.0, 0.0, 0.0), (0.4, 0.1, -0.3)]):
            V = synth.world_to_view(eye, cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            prevV = V
            for m, d in [(None, base)] + list(drivers.items()):
                d.view = view
                d.record(queries[m]); d.run()
            got_base = base.results()
            ref = oracle.frame(sc, view.as_dict(), hzb, depth, cullingFlags=flags, record_capacity=4096,
                               raster=(I.world_to_clip(V, P), v, s.meshletVertexIds, s.meshletTriangles))
            compare_frame(got_base, ref)
            k = consts(view)
            vis_ref, _ = VR.frame_visibility(vr, k, geo, ref, *render)
            base_vis, base_depth, base_motion, base_hzb = base.visibility.download_mip(0), base.depth.download_mip(0), base.motion.download_mip(0), base.hzb.download_chain()
            same(base_vis, vis_ref, f"flags {flags} frame {f}: visibility=True texels")
            stats = queries[None].get()
            for m, d in drivers.items():
                what = f"flags {flags} frame {f} debug mode {m}"
                compare_frame(d.results(), ref)
                g_ref, m_ref = GR.frame_gbuffer(gr, k, geo, ref, vis_ref, mats, m)
                g = d.gbufferA.download_mip(0)
                same(g, g_ref, what + ": GBufferA")
                mot = d.motion.download_mip(0).view(np.uint16)
                same(mot, VR.to_half_bits(m_ref), what + ": motion against the reference")
                same(mot, base_motion.view(np.uint16), what + ": motion against the visibility=True run")
                same(d.visibility.download_mip(0), base_vis, what + ": visibility texels")
                same(d.depth.download_mip(0).view(np.uint32), base_depth.view(np.uint32), what + ": depth")
                same(d.hzb.download_chain(), base_hzb, what + ": HZB")
                if flags & 2:
                    got = d.results()
                    assert got["lateCount"] == got_base["lateCount"] and np.array_equal(got["lateArgs"], got_base["lateArgs"])
                assert queries[m].get() == stats, what + ": pipeline statistics"
                cov = vis_ref != 0
                assert cov.sum() > 0.2 * cov.size and np.all(g[~cov] == 0) and np.all(g[cov][:, 3] == 0xFF)
                assert len(np.unique(g[cov][:, 1])) > 1000 and len(np.unique(g[cov][:, 0] & 0xFFFFFF)) > 8
                debug = g[cov][:, 0] >> 24
                _, slot, pos, _ = VR.decode(vis_ref[cov])                               # the debug byte from Python integers / numpy
                owner, lods, meshlet = (np.zeros(len(pos), np.uint32) for _ in range(3))
                for sl in range(4):
                    if ref.passRan[sl]:
                        sel = slot == sl
                        e = ref.visibleList[sl][pos[sel]]
                        rec = np.ascontiguousarray(ref.records[sl]).view(I.MeshletAmplificationData).reshape(-1)[e >> 5]
                        owner[sel], lods[sel], meshlet[sel] = rec["m_InstanceConstIdx"], rec["m_MeshLOD"], rec["m_MeshletGroupOffset"] + (e & 31)
                want = {0: np.zeros(len(pos), np.uint32), 2: _random_byte(owner), 3: _random_byte(meshlet), 12: lods}[m]
                assert np.array_equal(debug, want), what + ": the debug byte"
                if m in (2, 3):
                    assert len(np.unique(debug)) > 3
            assert stats["MSInvocations"] > 0
    finally:
        for q in queries.values():
            q.release()
        for d in list(drivers.values()) + [base]:
            d.release()
        gs.release()


def _direct(dev, k, sc, v, vid, tri, rec, lst, render, materials, slot=0, debug_mode=0, clear_to=0, profile=False):
    """One direct visibility dispatch (after clears) and one G-buffer resolve of its texels:
    (vis, GBufferA, motion halves, motion halves of "basepass_PS_Main_motion" on the same texels, profile)."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, PUSH, SRV, TEX_SRV, TEX_UAV
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
    mot2 = dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, "GBufferMotion (motion shader)")
    gba = dev.create_texture(W, H, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA")
    cl = dev.create_command_list()
    prof = None
    try:
        cl.open()
        cl.clear_texture_f32(depth, 0.0); cl.clear_texture_u32(vis, 0); cl.clear_texture_f32(mot, 0.0); cl.clear_texture_f32(mot2, 0.0)
        cl.clear_texture_u32(gba, clear_to)
        cb = cl.constant_buffer(k, "BasePassConstants")
        geo = [CB(0, cb), SRV(0, bufs[0]), SRV(1, bufs[1]), SRV(2, bufs[2]), SRV(4, bufs[3]), SRV(5, bufs[4]), SRV(6, bufs[5])]
        cl.dispatch_indirect("basepass_MS_Main_visibility", geo + [SRV(7, bufs[6]), SRV(9, bufs[7]), TEX_UAV(0, depth, 0), TEX_UAV(1, vis, 0), PUSH(1)],
                             args, push=np.array([slot], np.uint32))
        slots = []
        for s in range(4):
            slots += [SRV(10 + s, bufs[6] if s == slot else empty), SRV(14 + s, bufs[7] if s == slot else empty)]
        groups = ((W + 7) // 8, (H + 7) // 8, 1)
        cl.dispatch("basepass_PS_Main_GBuffer", geo + slots + [SRV(3, bufs[8]), TEX_SRV(18, vis), TEX_UAV(0, gba, 0), TEX_UAV(1, mot, 0)], groups)
        cl.dispatch("basepass_PS_Main_motion", geo + slots + [TEX_SRV(18, vis), TEX_UAV(0, mot2, 0)], groups)
        cl.close()
        if profile:
            dev.profile_reset(); dev.profile_enable(True)
        try:
            dev.execute(cl); dev.wait_idle()
            if profile:
                prof = dev.profile()
        finally:
            if profile:
                dev.profile_enable(False)
        return vis.download_mip(0), gba.download_mip(0), mot.download_mip(0).view(np.uint16), mot2.download_mip(0).view(np.uint16), prof
    finally:
        cl.release(); depth.release(); vis.release(); mot.release(); mot2.release(); gba.release(); args.release(); empty.release()
        for b in bufs:
            b.release()


def _reference(vr, gr, k, sc, v, vid, tri, rec, lst, render, materials, slot=0, debug_mode=0, clear_to=0):
    W, H = render
    geo = VR.Geometry(sc, v, vid, tri)
    depth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
    VR.raster(vr, k, geo, rec, lst, slot, depth, vis)
    recs = [rec if s == slot else None for s in range(4)]
    lsts = [lst if s == slot else None for s in range(4)]
    g, m = GR.gbuffer(gr, k, geo, recs, lsts, vis, materials, debug_mode, gbuffer_init=np.full((H, W, 4), clear_to, np.uint32))
    return vis, g, VR.to_half_bits(m)


def test_near_wall_with_exact_ties(dev, oracle, vr, gr, tmp_path):
    """The camera inside the city's wall (triangles through "tiles" and "main"), every instance duplicated with the identical
    matrix but another material: every sample ties exactly, the duplicate wins, and GBufferA shows the duplicate's material."""
    s, sc = city(tmp_path, oracle)
    v, sc, mats = with_normals_and_materials(s, sc)
    n0 = len(sc["instances"])
    sc, rec, lst, n = with_duplicates(s, sc, n0)
    sc["instances"]["m_MaterialDataIdx"][n:] = (sc["instances"]["m_MaterialDataIdx"][:n0] + 1) % len(mats)
    render = (1280, 720)
    k = consts(inside_view(s.cameras[0], render))
    for mode in (3, 2):
        vis, g, mot, mot2, prof = _direct(dev, k, sc, v, s.meshletVertexIds, s.meshletTriangles, rec, lst, render, mats, slot=2, debug_mode=mode, profile=True)
        rvis, rg, rmot = _reference(vr, gr, k, sc, v, s.meshletVertexIds, s.meshletTriangles, rec, lst, render, mats, slot=2, debug_mode=mode)
        same(vis, rvis, "texels"); same(g, rg, f"GBufferA, debug mode {mode}"); same(mot, rmot, "motion"); same(mot2, mot, "motion shader's words")
        assert {n_ for n_ in prof if n_.startswith("basepass_PS")} == {"basepass_PS_Main_GBuffer#main", "basepass_PS_Main_motion#main"}
        assert prof["basepass_PS_Main_GBuffer#main"][0] == 1
    cov = vis != 0
    assert cov.sum() > 0.3 * cov.size
    _, _, pos, _ = VR.decode(vis[cov])
    owners = rec["m_InstanceConstIdx"][lst[pos] >> 5]
    assert np.all(owners >= n)
    want = GR.pack_rgba8(gr, np.concatenate([mats["m_ConstAlbedo"][sc["instances"]["m_MaterialDataIdx"][owners]][:, :3], np.zeros((len(owners), 1), np.float32)], 1))
    assert np.array_equal(g[cov][:, 0] & 0xFFFFFF, want & 0xFFFFFF), "the albedo is the winning duplicate's material"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hostile_soup(dev, vr, gr, seed):
    """NaN / inf / 1e30 vertices, degenerate and out-of-contract triangles, random normal words, NaN / inf / negative material
    constants, and instance 1's material index out of range for odd seeds: exact, and texels that cannot be resolved keep
    the value GBufferA was cleared to."""
    sc, v, vid, tri, rec, lst = hostile_soup(seed)
    v = v.copy()
    v["m_PackedNormal"] = np.random.default_rng(seed).integers(0, 1 << 32, len(v), dtype=np.uint64).astype(np.uint32)
    mats = hostile_materials(seed)
    sc["instances"]["m_MaterialDataIdx"] = [1 + seed, 8 if seed % 2 else 3]
    render = (320, 200)
    k = consts(synth.make_view(render=render))
    vis, g, mot, mot2, _ = _direct(dev, k, sc, v, vid, tri, rec, lst, render, mats, slot=3, debug_mode=2, clear_to=0xABCD1234)
    rvis, rg, rmot = _reference(vr, gr, k, sc, v, vid, tri, rec, lst, render, mats, slot=3, debug_mode=2, clear_to=0xABCD1234)
    same(vis, rvis, "texels"); same(g, rg, "GBufferA"); same(mot, rmot, "motion")
    cov = vis != 0
    assert cov.sum() > 1000 and np.all(g[~cov] == 0xABCD1234)
    _, _, pos, _ = VR.decode(vis)
    second = cov & (rec["m_InstanceConstIdx"][lst[pos] >> 5] == 1)
    assert second.any() and (cov & ~second).any()
    if seed % 2:
        assert np.all(g[second] == 0xABCD1234) and np.all(mot[second] == 0), "an out-of-range material index leaves both targets"
        same(mot[~second], mot2[~second], "motion shader's words")
    else:
        assert np.all(g[cov][:, 3] == 0xFF)
        same(mot, mot2, "motion shader's words")


def test_degenerate_world_matrix_gives_nan_normals(dev, vr, gr):
    """A wall whose instance scales x and y by 1e-30 (the positions carry the inverse): the adjugate's products underflow, the
    normal's length is 0 and the normalisation divides by it.  NaN and infinite normals pack as the reference packs them."""
    sc, v, vid, tri, rec, lst = wall(0x2FF7FDFF, scale=(1e-30, 2e-30, 1.0), axis=(0.0, 0.0, 1.0), angle=0.3)
    v["m_Position"][:, :2] *= np.float32(1e30)
    render = (320, 200)
    k = consts(synth.make_view(render=render))
    mats = synth.materials(3, 4)
    vis, g, mot, mot2, _ = _direct(dev, k, sc, v, vid, tri, rec, lst, render, mats)
    rvis, rg, rmot = _reference(vr, gr, k, sc, v, vid, tri, rec, lst, render, mats)
    same(vis, rvis, "texels"); same(g, rg, "GBufferA"); same(mot, rmot, "motion"); same(mot2, mot, "motion shader's words")
    cov = vis != 0
    assert cov.sum() > 1000
    n = GR.vertex_normal(gr, 0x2FF7FDFF, sc["instances"]["m_WorldMatrix"][0])
    assert not np.all(np.isfinite(n)), "the case must produce a non-finite vertex normal"


def test_wall_normals_on_the_gpu(dev, vr, gr):
    """The CPU file's wall (one packed normal, rotated instance, scale ratio 4): the GPU's words equal the reference's, and
    decode to the float64 normal within 1e-4 (bound derived in tests/test_gbuffer_ref.py)."""
    word = 0x2FF7FDFF
    sc, v, vid, tri, rec, lst = wall(word)
    render = (320, 200)
    k = consts(synth.make_view(render=render))
    mats = synth.materials(1, 4)
    vis, g, mot, mot2, _ = _direct(dev, k, sc, v, vid, tri, rec, lst, render, mats)
    rvis, rg, rmot = _reference(vr, gr, k, sc, v, vid, tri, rec, lst, render, mats)
    same(vis, rvis, "texels"); same(g, rg, "GBufferA"); same(mot, rmot, "motion")
    cov = vis != 0
    u = np.array([(word >> 20) & 0x3FF, (word >> 10) & 0x3FF, word & 0x3FF], np.float64) / 1023.0 * 2.0 - 1.0
    Wm = sc["instances"]["m_WorldMatrix"][0].astype(np.float64)[:3, :3]
    want = u @ np.stack([np.cross(Wm[1], Wm[2]), np.cross(Wm[2], Wm[0]), np.cross(Wm[0], Wm[1])])
    want /= np.linalg.norm(want)
    assert cov.sum() > 2000 and np.linalg.norm(GR.decode_oct(g[cov][:, 1]) - want, axis=1).max() <= 1e-4


def test_animated_frames_with_alpha_mask_slots(dev, oracle, vr, gr, tmp_path):
    """Four frames: the camera and every instance move (m_PrevWorldMatrix = last frame's), through all four slots."""
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    assert len(s.alphaMaskIds) > 0
    v, sc, mats = with_normals_and_materials(s, sc)
    inst0 = sc["instances"].copy()
    gs = gpu_scene(dev, s, inst0, v, mats)
    cam = s.cameras[0]
    render = (640, 360)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V0 = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    view = synth.View(V0, V0.copy(), P, float(np.float32(cam.znear)), *render)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, gbuffer=True, debug_mode=3)
    geo_v = (v, s.meshletVertexIds, s.meshletTriangles)
    hzb = oracle.HzbTexture(*view.hzb_dims)
    depth = np.zeros((render[1], render[0]), np.float32)
    prevV, prevW = V0, inst0["m_WorldMatrix"].copy()
    slots_seen = set()
    try:
        for f in range(4):
            V = synth.world_to_view((0.1 * f, 0.02 * f, -0.15 * f), cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            inst = inst0.copy()
            inst["m_WorldMatrix"][:, 3, 0] += np.float32(0.03 * f) * (1 + np.arange(len(inst)) % 3)
            inst["m_PrevWorldMatrix"] = prevW
            prevV, prevW = V, inst["m_WorldMatrix"].copy()
            gs.instances.upload(inst)
            scf = dict(sc); scf["instances"] = inst
            drv.view = view
            drv.record(); drv.run(); drv.results()
            ref = oracle.frame(scf, view.as_dict(), hzb, depth, cullingFlags=7, record_capacity=4096, raster=(I.world_to_clip(V, P), *geo_v))
            k = consts(view)
            geo = VR.Geometry(scf, *geo_v)
            vis_ref, _ = VR.frame_visibility(vr, k, geo, ref, *render)
            same(drv.visibility.download_mip(0), vis_ref, f"frame {f}: texels")
            g_ref, m_ref = GR.frame_gbuffer(gr, k, geo, ref, vis_ref, mats, 3)
            same(drv.gbufferA.download_mip(0), g_ref, f"frame {f}: GBufferA")
            m = drv.motion.download_mip(0).view(np.uint16)
            same(m, VR.to_half_bits(m_ref), f"frame {f}: motion")
            slots_seen |= set(np.unique(VR.decode(vis_ref[vis_ref != 0])[1]).tolist())
            if f > 0:
                assert np.count_nonzero(m) > 0.2 * vis_ref.size
        assert {0, 2} <= slots_seen, slots_seen
    finally:
        drv.release(); gs.release()


def test_lists_without_the_feature_record_the_same_ops(dev, oracle, tmp_path):
    """visibility=True alone and raster_depth=True alone record what they recorded before this shader existed: no op of
    "basepass_PS_Main_GBuffer", one "basepass_PS_Main_motion" (or none); gbuffer=True records the visibility=True list with the
    one resolve swapped."""
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    v, sc, mats = with_normals_and_materials(s, sc)
    gs = gpu_scene(dev, s, sc["instances"], v, mats)
    view = gltf_lite.view_of(s.cameras[0], (320, 180))
    out = {}
    try:
        for name, kw in (("depth", dict(raster_depth=True)), ("visibility", dict(visibility=True)), ("gbuffer", dict(gbuffer=True))):
            drv = FrameDriver(dev, gs, view, record_capacity=4096, **kw)
            try:
                out[name] = op_counts(dev, drv)
            finally:
                drv.release()
    finally:
        gs.release()
    print(json.dumps(out, indent=1))
    cull = {f"{n} LATE_CULL={late}#{k}": 2 for late in (0, 1) for n, ks in (("gpuculling_CS_GPUCulling", ("instance_cache", "fused")), ("basepass_AS_Main", ("cull", "compact")))
            for k in ks}
    hzb = {"ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1#depth_tile": 2, "ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1#tail": 2}
    # the per-op launch counts of the lists as they were before this shader existed (opaque + alpha-mask, early + late)
    assert out["depth"] == {**cull, **hzb, "basepass_MS_Main_depth#main": 4, "basepass_MS_Main_depth#tiles": 4}
    assert out["visibility"] == {**cull, **hzb, "basepass_MS_Main_visibility#main": 4, "basepass_MS_Main_visibility#tiles": 4, "basepass_PS_Main_motion#main": 1}
    swapped = dict(out["visibility"])
    swapped["basepass_PS_Main_GBuffer#main"] = swapped.pop("basepass_PS_Main_motion#main")
    assert out["gbuffer"] == swapped


def test_cornell_walls_through_the_driver_and_the_facade(dev, oracle, vr, gr):
    """FrameDriver(gbuffer=True) on the cornell fixture: GBufferA equals the reference, its albedo shows the white, red and
    green walls, and the host mirror's trhost_download_gbuffer_a returns the same words."""
    from toyrenderer_amd import host
    from toyrenderer_amd.frame import FrameDriver
    s, inst, _, mats, camera = lit_cornell(oracle)
    with open(os.path.join(ROOT, "tests", "golden", "cornell_materials.json")) as f:
        cm = json.load(f)
    sc = dict(s.as_oracle()); sc["instances"] = inst
    render = (320, 180)
    view = gltf_lite.view_of(camera, render)
    gs = gpu_scene(dev, s, inst, s.vertices, mats)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, gbuffer=True)
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    try:
        drv.record(); drv.run(); drv.results()
        ref = oracle.frame(sc, view.as_dict(), oracle.HzbTexture(*view.hzb_dims), np.zeros((render[1], render[0]), np.float32), cullingFlags=7,
                           record_capacity=4096, raster=(I.world_to_clip(view.worldToView, view.viewToClip), *geo_v))
        k = consts(view)
        geo = VR.Geometry(sc, *geo_v)
        vis_ref, _ = VR.frame_visibility(vr, k, geo, ref, *render)
        g_ref, _ = GR.frame_gbuffer(gr, k, geo, ref, vis_ref, mats)
        g = drv.gbufferA.download_mip(0)
        same(drv.visibility.download_mip(0), vis_ref, "texels"); same(g, g_ref, "GBufferA")
    finally:
        drv.release(); gs.release()
    cov = vis_ref != 0
    colours = [tuple(int(x) for x in (np.asarray(c[:3], np.float32) * np.float32(255)).astype(np.uint32)) for c in cm["baseColorFactor"]]
    got = GR.albedo_bytes(g[cov][:, 0])
    counts = [int(np.count_nonzero(np.all(got == np.array(c), axis=1))) for c in colours]
    assert sum(counts) == int(cov.sum()) and all(c > 1000 for c in counts), counts
    with host_renderer(s, gltf_lite.apply_materials(s), geo_v, mats, render=render, max_groups=4096) as r:
        r.set_gbuffer(True)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        r.set_camera(view)
        r.frame(); r.results()
        same(r.download_visibility(), vis_ref, "host: texels")
        same(r.download_gbuffer_a(), g, "host: GBufferA")


def test_host_path_with_animated_nodes(oracle, vr, gr, tmp_path):
    """The C++ host mirror (trhost_set_gbuffer): five frames with animated node transforms, a moving camera and a debug view
    mode that changes between frames.  GBufferA equals the reference computed from Renderer.instances() and each frame's
    view; motion too from the second frame on (the first frame's previous projection is the host's initial one)."""
    from toyrenderer_amd import host
    s, sc0 = city(tmp_path, oracle)
    v, sc0, mats = with_normals_and_materials(s, sc0)
    cam = s.cameras[0]
    render = (640, 360)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    hzb = oracle.HzbTexture(*I.hzb_dims(*render))
    depth = np.zeros((render[1], render[0]), np.float32)
    geo_v = (v, s.meshletVertexIds, s.meshletTriangles)
    inst_in = s.instances.copy()
    inst_in["m_MaterialDataIdx"] = sc0["instances"]["m_MaterialDataIdx"]
    with host_renderer(s, inst_in, geo_v, render=render, max_groups=4096) as r:
        with pytest.raises(host.HostError, match="trhost_load_materials"):
            r.set_gbuffer(True)
        textured = mats.copy(); textured["m_MaterialFlags"][5] = I.MaterialFlag_UseNormalTexture
        with pytest.raises(host.HostError, match="texture"):
            r.load_materials(textured)
        r.load_materials(mats)
        r.set_gbuffer(True)
        r.set_culling(7)
        prevV = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
        for f, mode in enumerate((0, 2, 3, 12, 3)):
            V = synth.world_to_view((0.1 * f, 0.02 * f, -0.15 * f), cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            prevV = V
            nodes = s.nodes.copy()
            nodes["m_Position"][:, 0] += np.float32(0.04 * f) * (1 + np.arange(len(nodes)) % 3)
            r.set_node_transforms(nodes)
            r.set_camera(view)
            r.set_debug_view_mode(mode)
            r.frame()
            got = r.results()
            inst = r.instances(len(s.instances))
            assert np.array_equal(inst["m_MaterialDataIdx"], inst_in["m_MaterialDataIdx"])
            sc = dict(s.as_oracle()); sc["instances"] = inst
            ref = oracle.frame(sc, view.as_dict(), hzb, depth, cullingFlags=7, record_capacity=4096, maxGroups=4096,
                               raster=(I.world_to_clip(V, P), *geo_v))
            compare_frame(got, ref)
            k = consts(view)
            geo = VR.Geometry(sc, *geo_v)
            vis_ref, _ = VR.frame_visibility(vr, k, geo, ref, *render)
            same(r.download_visibility(), vis_ref, f"frame {f}: texels")
            g_ref, m_ref = GR.frame_gbuffer(gr, k, geo, ref, vis_ref, mats, mode)
            g = r.download_gbuffer_a()
            same(g, g_ref, f"frame {f} (debug view {mode}): GBufferA")
            assert np.count_nonzero(g[..., 3]) > 0.2 * vis_ref.size
            if f > 0:
                same(r.download_motion().view(np.uint16), VR.to_half_bits(m_ref), f"frame {f}: motion")
        with pytest.raises(host.HostError, match="per rank"):
            host._check(host.load().trhost_exchange_create(ctypes.byref(host.ExchangeDesc())))


def test_misuse_is_refused(dev, oracle, tmp_path):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver
    from toyrenderer_amd.rhi import CB, SRV, TEX_SRV, TEX_UAV
    sc, v, vid, tri, rec, lst = hostile_soup(0)
    W, H = 64, 32
    k = consts(synth.make_view(render=(W, H)))
    bufs = [dev.buffer_from(sc["instances"], "inst", uav=False), dev.buffer_from(v, "v", uav=False), dev.buffer_from(sc["meshData"], "md", uav=False),
            dev.buffer_from(sc["meshlets"], "ml", uav=False), dev.buffer_from(vid, "vid", uav=False), dev.buffer_from(tri, "tri", uav=False),
            dev.buffer_from(rec, "rec"), dev.buffer_from(lst, "lst"), dev.buffer_from(synth.materials(0, 4), "materials", uav=False)]
    args = dev.create_buffer(12, "args", stride=12, indirect=True)
    args.upload(np.array([8, 4, 1], np.uint32))
    vis = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "vis")
    mot = dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, "motion")
    gba = dev.create_texture(W, H, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA")
    small = dev.create_texture(W // 2, H, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA small")
    wrong = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "GBufferA RG32")
    cl = dev.create_command_list()
    groups = ((W + 7) // 8, (H + 7) // 8, 1)
    try:
        cl.open()
        cb = cl.constant_buffer(k, "BasePassConstants")
        base = [CB(0, cb), SRV(0, bufs[0]), SRV(1, bufs[1]), SRV(2, bufs[2]), SRV(4, bufs[3]), SRV(5, bufs[4]), SRV(6, bufs[5]), TEX_SRV(18, vis)]
        for s in range(4):
            base += [SRV(10 + s, bufs[6]), SRV(14 + s, bufs[7])]
        mat, u0, u1 = [SRV(3, bufs[8])], [TEX_UAV(0, gba, 0)], [TEX_UAV(1, mot, 0)]
        cases = [("u0 wrong format", base + mat + [TEX_UAV(0, wrong, 0)] + u1, groups, "RGBA32_UINT"),
                 ("u0 is the motion target", base + mat + [TEX_UAV(0, mot, 0)] + u1, groups, "RGBA32_UINT"),
                 ("u0 wrong size", base + mat + [TEX_UAV(0, small, 0)] + u1, groups, "m_OutputResolution"),
                 ("u0 missing", base + mat + u1, groups, "u0"),
                 ("u1 missing", base + mat + u0, groups, "u1"),
                 ("t3 missing", base + u0 + u1, groups, "t3"),
                 ("grid too small", base + mat + u0 + u1, (groups[0] - 1, groups[1], 1), "covering")]
        for what, b, grp, text in cases:
            with pytest.raises(rhi.TrhipError, match=text):
                cl.dispatch("basepass_PS_Main_GBuffer", b, grp)
        with pytest.raises(rhi.TrhipError, match="direct dispatch"):
            cl.dispatch_indirect("basepass_PS_Main_GBuffer", base + mat + u0 + u1, args)
        cl.dispatch("basepass_PS_Main_GBuffer", base + mat + u0 + u1, groups)                       # the good one records
        with pytest.raises(rhi.TrhipError, match="clear_texture_u32"):
            cl.clear_texture_f32(gba, 0.0)
        cl.clear_texture_u32(gba, 7)
        cl.close()
        dev.execute(cl); dev.wait_idle()
        assert np.all(gba.download_mip(0) == 7) and gba.download_mip(0).shape == (H, W, 4)
        up = np.arange(W * H * 4, dtype=np.uint32).reshape(H, W, 4)
        gba.upload_mip(0, up)
        assert np.array_equal(gba.download_mip(0), up)
        gba.mark_written()
        w_, h_, off = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        assert rhi.load().trhip_texture_mip_info(gba.h, 0, ctypes.byref(w_), ctypes.byref(h_), ctypes.byref(off)) == 0
        assert (w_.value, h_.value, off.value) == (W, H, 0) and rhi.load().trhip_texture_size(gba.h) >= W * H * 16
    finally:
        cl.release(); vis.release(); mot.release(); gba.release(); small.release(); wrong.release(); args.release()
        for b in bufs:
            b.release()
    with pytest.raises(rhi.TrhipError, match="one mip"):
        dev.create_texture(W, H, 2, rhi.FORMAT_RGBA32_UINT, "two mips")
    s, scc = city(tmp_path, oracle)
    v2, scc, mats = with_normals_and_materials(s, scc)
    gs = gpu_scene(dev, s, scc["instances"], v2, None)
    view = gltf_lite.view_of(s.cameras[0], (64, 32))
    try:
        with pytest.raises(ValueError, match="set_materials"):
            FrameDriver(dev, gs, view, record_capacity=64, gbuffer=True)
        textured = mats.copy(); textured["m_MaterialFlags"][0] = I.MaterialFlag_UseAlbedoTexture
        with pytest.raises(ValueError, match="texture"):
            gs.set_materials(textured)
        gs.set_materials(mats)
        with pytest.raises(ValueError, match="shard"):
            FrameDriver(dev, gs, view, record_capacity=64, gbuffer=True, shard_late=lambda *a: None)
    finally:
        gs.release()
