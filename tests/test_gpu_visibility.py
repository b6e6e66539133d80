"""The visibility buffer ("basepass_MS_Main_visibility", csrc/k_raster.hip) and the motion resolve
("basepass_PS_Main_motion", csrc/k_motion.hip) on the GPU, word for word against tests/visibility_ref.c: through
FrameDriver(visibility=True) under all culling flags, through direct dispatches on a near wall (tile launch, exact depth
ties) and a hostile triangle soup, over animated frames, with pipeline statistics, and misuse."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from suite_support import compare_frame, dev, gpu_scene, host_renderer, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from toyrenderer_amd import gltf_lite, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import city, consts, hostile_soup, inside_view, with_duplicates  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_buffers(drv, vr, k, geo, ref, W, H, what):
    vis_ref, _ = VR.frame_visibility(vr, k, geo, ref, W, H)
    vis = drv.visibility.download_mip(0)
    depth = drv.depth.download_mip(0)
    assert np.array_equal(vis, vis_ref), f"{what}: visibility buffer differs in {int(np.count_nonzero(vis != vis_ref))} texels"
    assert np.array_equal((vis >> np.uint64(32)).astype(np.uint32), depth.view(np.uint32)), f"{what}: high words != depth"
    m_ref = VR.to_half_bits(VR.frame_motion(vr, k, geo, ref, vis_ref))
    m = drv.motion.download_mip(0).view(np.uint16)
    assert np.array_equal(m, m_ref), f"{what}: motion differs in {int(np.count_nonzero(m != m_ref))} words"
    return vis, m


@pytest.mark.parametrize("flags", range(8))
def test_frames_match_the_reference_under_every_flag(dev, oracle, vr, tmp_path, flags):
    """Two frames of a moving camera: visibility buffer and motion equal the reference; depth, HZB and every cull output
    are bit-identical to a raster_depth=True run without the visibility buffer."""
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    gs = gpu_scene(dev, s, sc["instances"])
    cam = s.cameras[0]
    render = (640, 360)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V0 = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    view = synth.View(V0, V0.copy(), P, float(np.float32(cam.znear)), *render)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=flags, visibility=True)
    base = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=flags, raster_depth=True)
    geo = VR.Geometry(sc, s.vertices, s.meshletVertexIds, s.meshletTriangles)
    hzb = oracle.HzbTexture(*view.hzb_dims)
    depth = np.zeros((render[1], render[0]), np.float32)
    prevV = V0
    try:
        for f, eye in enumerate([(0.0, 0.0, 0.0), (0.4, 0.1, -0.3)]):
            V = synth.world_to_view(eye, cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            prevV = V
            for d in (drv, base):
                d.view = view
                d.record(); d.run()
            got, got_base = drv.results(), base.results()
            ref = oracle.frame(sc, view.as_dict(), hzb, depth, cullingFlags=flags, record_capacity=4096,
                               raster=(I.world_to_clip(V, P), s.vertices, s.meshletVertexIds, s.meshletTriangles))
            compare_frame(got, ref)
            compare_frame(got_base, ref)
            assert np.array_equal(drv.depth.download_mip(0).view(np.uint32), base.depth.download_mip(0).view(np.uint32))
            assert np.array_equal(drv.depth.download_mip(0).view(np.uint32), depth.view(np.uint32))
            assert np.array_equal(drv.hzb.download_chain(), base.hzb.download_chain())
            if flags & 2:                                                                # the late buffers exist for occlusion only
                assert got["lateCount"] == got_base["lateCount"] and np.array_equal(got["lateArgs"], got_base["lateArgs"])
            vis, m = _check_buffers(drv, vr, consts(view), geo, ref, *render, f"flags {flags} frame {f}")
            assert np.count_nonzero(vis) > 0.2 * vis.size
            if f == 1:
                assert np.count_nonzero(m) > 0.2 * vis.size, "a moving camera moves pixels"
    finally:
        drv.release(); base.release(); gs.release()


def _direct(dev, k, sc, v, vid, tri, rec, lst, render, slot=0, profile=False):
    """One direct visibility dispatch (after clears) and one motion resolve of its texels: (depth, vis, motion, profile)."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, PUSH, SRV, TEX_SRV, TEX_UAV
    W, H = render
    bufs = [dev.buffer_from(sc["instances"], "inst", uav=False), dev.buffer_from(v, "v", uav=False, min_bytes=20),
            dev.buffer_from(sc["meshData"], "md", uav=False), dev.buffer_from(sc["meshlets"], "ml", uav=False, min_bytes=32),
            dev.buffer_from(vid, "vid", uav=False), dev.buffer_from(tri, "tri", uav=False), dev.buffer_from(rec, "rec", min_bytes=12),
            dev.buffer_from(lst, "lst")]
    empty = dev.create_buffer(16, "empty")
    args = dev.create_buffer(12, "drawArgs", stride=12, indirect=True)
    args.upload(np.array([len(lst), 1, 1], np.uint32))
    depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
    vis = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "VisibilityBuffer")
    mot = dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, "GBufferMotion")
    cl = dev.create_command_list()
    prof = None
    try:
        cl.open()
        cl.clear_texture_f32(depth, 0.0); cl.clear_texture_u32(vis, 0); cl.clear_texture_f32(mot, 0.0)
        cb = cl.constant_buffer(k, "BasePassConstants")
        geo = [CB(0, cb), SRV(0, bufs[0]), SRV(1, bufs[1]), SRV(2, bufs[2]), SRV(4, bufs[3]), SRV(5, bufs[4]), SRV(6, bufs[5])]
        cl.dispatch_indirect("basepass_MS_Main_visibility", geo + [SRV(7, bufs[6]), SRV(9, bufs[7]), TEX_UAV(0, depth, 0), TEX_UAV(1, vis, 0), PUSH(1)],
                             args, push=np.array([slot], np.uint32))
        slots = []
        for s in range(4):
            slots += [SRV(10 + s, bufs[6] if s == slot else empty), SRV(14 + s, bufs[7] if s == slot else empty)]
        cl.dispatch("basepass_PS_Main_motion", geo + slots + [TEX_SRV(18, vis), TEX_UAV(0, mot, 0)], ((W + 7) // 8, (H + 7) // 8, 1))
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
        return depth.download_mip(0), vis.download_mip(0), mot.download_mip(0).view(np.uint16), prof
    finally:
        cl.release(); depth.release(); vis.release(); mot.release(); args.release(); empty.release()
        for b in bufs:
            b.release()


def _reference(vr, k, sc, v, vid, tri, rec, lst, render, slot=0):
    W, H = render
    geo = VR.Geometry(sc, v, vid, tri)
    depth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
    VR.raster(vr, k, geo, rec, lst, slot, depth, vis)
    recs = [rec if s == slot else None for s in range(4)]
    lsts = [lst if s == slot else None for s in range(4)]
    return depth, vis, VR.to_half_bits(VR.motion(vr, k, geo, recs, lsts, vis))


def test_near_wall_goes_through_both_launches_and_ties_take_the_larger_payload(dev, oracle, vr, tmp_path):
    """The camera inside the city's wall: triangles far larger than kSmallBox (1024 px) go through "tiles", small ones
    through "main".  Every instance is duplicated with the identical matrix: every sample ties exactly, and the
    duplicate (larger list position) must win through both launches."""
    s, sc = city(tmp_path, oracle)
    sc, rec, lst, n = with_duplicates(s, sc, len(sc["instances"]))
    render = (1280, 720)
    view = inside_view(s.cameras[0], render)
    k = consts(view)
    depth, vis, mot, prof = _direct(dev, k, sc, s.vertices, s.meshletVertexIds, s.meshletTriangles, rec, lst, render, slot=2, profile=True)
    rdepth, rvis, rmot = _reference(vr, k, sc, s.vertices, s.meshletVertexIds, s.meshletTriangles, rec, lst, render, slot=2)
    assert np.array_equal(depth.view(np.uint32), rdepth.view(np.uint32))
    assert np.array_equal(vis, rvis)
    assert np.array_equal(mot, rmot)
    # the op names of the two launches and the resolve (launch counts only: "tiles" launches whether or not anything was
    # queued; the evidence that queued triangles were drawn is the payload coverage below)
    assert set(k for k in prof if k.startswith("basepass_")) == {"basepass_MS_Main_visibility#main", "basepass_MS_Main_visibility#tiles",
                                                                  "basepass_PS_Main_motion#main"}
    _, slot, pos, _ = VR.decode(vis[vis != 0])
    assert np.all(slot == 2)
    owners = rec["m_InstanceConstIdx"][lst[pos] >> 5]
    assert np.all(owners >= n), "an exact tie went to the smaller payload"
    # both launches produced texels: a payload covering more than kSmallBox (1024) pixels has a larger bounding box, so it
    # was queued and drawn by "tiles"; payloads of a few pixels were drawn in place by "main"
    _, counts = np.unique(vis[vis != 0] & np.uint64(0xFFFFFFFF), return_counts=True)
    assert counts.max() > 4096 and counts.min() < 64
    assert np.count_nonzero(vis) > 0.3 * vis.size


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hostile_soup(dev, oracle, vr, seed):
    """NaN / inf / 1e30 vertices, near-plane crossings, degenerate triangles, indices past the vertex count and meshlets
    with more than 128 triangles (depth only): depth, texels and motion exact, instance 1 moved since the last frame."""
    sc, v, vid, tri, rec, lst = hostile_soup(seed)
    render = (320, 200)
    view = synth.make_view(render=render)
    k = consts(view)
    depth, vis, mot, _ = _direct(dev, k, sc, v, vid, tri, rec, lst, render, slot=3)
    rdepth, rvis, rmot = _reference(vr, k, sc, v, vid, tri, rec, lst, render, slot=3)
    oref = np.zeros((render[1], render[0]), np.float32)
    oracle.raster_depth(k, sc, v, vid, tri, rec, lst, oref)
    assert np.array_equal(depth.view(np.uint32), oref.view(np.uint32))
    assert np.array_equal(vis, rvis)
    assert np.array_equal(mot, rmot)
    assert np.count_nonzero(mot) > 0


def test_animated_frames_with_alpha_mask_slots(dev, oracle, vr, tmp_path):
    """Four frames: the camera moves and every instance's world matrix moves (m_PrevWorldMatrix = last frame's), through
    all four slots.  Motion and texels equal the reference each frame."""
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    assert len(s.alphaMaskIds) > 0
    inst0 = sc["instances"].copy()
    gs = gpu_scene(dev, s, inst0)
    cam = s.cameras[0]
    render = (640, 360)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V0 = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    view = synth.View(V0, V0.copy(), P, float(np.float32(cam.znear)), *render)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, visibility=True)
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
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
            drv.record(); drv.run()
            drv.results()
            ref = oracle.frame(scf, view.as_dict(), hzb, depth, cullingFlags=7, record_capacity=4096, raster=(I.world_to_clip(V, P), *geo_v))
            vis, m = _check_buffers(drv, vr, consts(view), VR.Geometry(scf, *geo_v), ref, *render, f"frame {f}")
            slots_seen |= set(np.unique(VR.decode(vis[vis != 0])[1]).tolist())
            if f > 0:
                assert np.count_nonzero(m) > 0.2 * vis.size
        assert {0, 2} <= slots_seen, slots_seen                                         # opaque and alpha-mask texels
    finally:
        drv.release(); gs.release()


def test_pipeline_statistics_are_unchanged(dev, oracle, tmp_path):
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    gs = gpu_scene(dev, s, sc["instances"])
    view = gltf_lite.view_of(s.cameras[0], (640, 360))
    out = []
    try:
        for vis in (False, True):
            drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, raster_depth=True, visibility=vis)
            q = dev.create_pipeline_stats()
            try:
                drv.record(q); drv.run(); drv.results()
                out.append(q.get())
            finally:
                q.release(); drv.release()
    finally:
        gs.release()
    assert out[0] == out[1] and out[0]["MSInvocations"] > 0


def test_misuse_is_refused(dev, oracle, tmp_path):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver
    from toyrenderer_amd.rhi import CB, PUSH, SRV, TEX_UAV
    sc, v, vid, tri, rec, lst = hostile_soup(0)
    W, H = 64, 32
    k = consts(synth.make_view(render=(W, H)))
    bufs = [dev.buffer_from(sc["instances"], "inst", uav=False), dev.buffer_from(v, "v", uav=False), dev.buffer_from(sc["meshData"], "md", uav=False),
            dev.buffer_from(sc["meshlets"], "ml", uav=False), dev.buffer_from(vid, "vid", uav=False), dev.buffer_from(tri, "tri", uav=False),
            dev.buffer_from(rec, "rec"), dev.buffer_from(lst, "lst"), dev.create_buffer(4 * ((1 << 23) + 1), "huge list")]
    args = dev.create_buffer(12, "drawArgs", stride=12, indirect=True)
    args.upload(np.array([len(lst), 1, 1], np.uint32))
    depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "depth")
    good = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "vis")
    small = dev.create_texture(W // 2, H, 1, rhi.FORMAT_RG32_UINT, "vis small")
    wrong = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "vis R32F")
    cl = dev.create_command_list()
    slot0 = np.array([0], np.uint32)
    try:
        cl.open()
        cb = cl.constant_buffer(k, "BasePassConstants")
        base = [CB(0, cb), SRV(0, bufs[0]), SRV(1, bufs[1]), SRV(2, bufs[2]), SRV(4, bufs[3]), SRV(5, bufs[4]), SRV(6, bufs[5]), SRV(7, bufs[6]),
                TEX_UAV(0, depth, 0)]
        cases = [("u1 missing", base + [SRV(9, bufs[7]), PUSH(1)], slot0, "u1"),
                 ("u1 wrong format", base + [SRV(9, bufs[7]), TEX_UAV(1, wrong, 0), PUSH(1)], slot0, "RG32_UINT"),
                 ("u1 wrong size", base + [SRV(9, bufs[7]), TEX_UAV(1, small, 0), PUSH(1)], slot0, "does not match"),
                 ("no push constant", base + [SRV(9, bufs[7]), TEX_UAV(1, good, 0)], None, "push constants"),
                 ("slot 4", base + [SRV(9, bufs[7]), TEX_UAV(1, good, 0), PUSH(1)], np.array([4], np.uint32), "pass slot 4"),
                 ("list above 2^23", base + [SRV(9, bufs[8]), TEX_UAV(1, good, 0), PUSH(1)], slot0, "8388609 entries")]
        for what, b, push, text in cases:
            with pytest.raises(rhi.TrhipError, match=text):
                cl.dispatch_indirect("basepass_MS_Main_visibility", b, args, push=push)
        cl.dispatch_indirect("basepass_MS_Main_visibility", base + [SRV(9, bufs[7]), TEX_UAV(1, good, 0), PUSH(1)], args, push=slot0)   # the good one records
        with pytest.raises(rhi.TrhipError, match="clear_texture_u32"):
            cl.clear_texture_f32(good, 0.0)
        with pytest.raises(rhi.TrhipError, match="RG32_UINT"):
            cl.clear_texture_u32(depth, 0)
        cl.close()
    finally:
        cl.release(); depth.release(); good.release(); small.release(); wrong.release(); args.release()
        for b in bufs:
            b.release()
    with pytest.raises(rhi.TrhipError, match="one mip"):
        dev.create_texture(W, H, 2, rhi.FORMAT_RG32_UINT, "two mips")
    # a shard exchange with the visibility buffer fails loudly: list positions are per rank
    s, scc = city(tmp_path, oracle)
    gs = gpu_scene(dev, s, scc["instances"])
    try:
        with pytest.raises(ValueError, match="shard"):
            FrameDriver(dev, gs, gltf_lite.view_of(s.cameras[0], (64, 32)), record_capacity=64, visibility=True,
                        shard_late=lambda *a: None)
    finally:
        gs.release()


def test_depth_only_list_records_the_same_ops(dev, oracle, tmp_path):
    """Without the switch the frame still dispatches basepass_MS_Main_depth (main, tiles) and nothing new."""
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    gs = gpu_scene(dev, s, sc["instances"])
    drv = FrameDriver(dev, gs, gltf_lite.view_of(s.cameras[0], (320, 180)), record_capacity=4096, raster_depth=True)
    try:
        dev.profile_reset(); dev.profile_enable(True)
        try:
            drv.record(); drv.run(); drv.results()
            prof = dev.profile()
        finally:
            dev.profile_enable(False)
    finally:
        drv.release(); gs.release()
    names = {n for n in prof if n.startswith("basepass_MS") or n.startswith("basepass_PS")}
    assert names == {"basepass_MS_Main_depth#main", "basepass_MS_Main_depth#tiles"}, names


def test_out_of_contract_triangle_in_front_inside_tiles(dev, vr):
    """A large triangle with index 128 (out of contract: depth, no texel) lies in front of large in-contract triangles, all
    queued for "tiles".  The texels must still come from the triangles behind it: the tile's far-depth early-out reads the
    texel words, so the triangles behind are not skipped once the depth tile is full.  The out-of-contract meshlet comes
    first in the list and the 64 meshlets behind it follow, so it is queued early and the early-out is taken often."""
    W, H = 256, 192
    view = synth.make_view(render=(W, H))
    k = consts(view)
    near = [(-3.0, -3.0, -2.0), (3.0, -3.0, -2.0), (0.0, 3.0, -2.0)]          # covers the screen centre, depth ~0.05
    far = [(-30.0, -30.0, -10.0), (30.0, -30.0, -10.0), (0.0, 30.0, -10.0)]    # behind it, everywhere
    v = np.zeros(6, I.RawVertexFormat)
    v["m_Position"] = np.array(near + far, np.float32)
    n_far = 64
    meshlets = np.zeros(1 + n_far, I.MeshletData)
    tris = [3 | (4 << 8) | (5 << 16)] * 128 + [0 | (1 << 8) | (2 << 16)]         # 0..127: far (texels), 128: near (depth only)
    meshlets[0]["m_VertexAndTriangleCount"] = 6 | (129 << 8)
    for m in range(1, 1 + n_far):                                                # far triangles again, in contract
        meshlets[m]["m_MeshletIndexIDsBufferIdx"] = len(tris)
        meshlets[m]["m_VertexAndTriangleCount"] = 6 | (1 << 8)
        tris.append(3 | (4 << 8) | (5 << 16))
    tri = np.array(tris, np.uint32)
    vid = np.arange(6, dtype=np.uint32)
    inst = np.zeros(1, I.BasePassInstanceConstants)
    inst["m_WorldMatrix"][0] = np.eye(4, dtype=np.float32)
    inst["m_PrevWorldMatrix"][0] = np.eye(4, dtype=np.float32)
    md = np.zeros(1, I.MeshData)
    md["m_NumLODs"] = 1
    md["m_MeshLODDatas"]["m_NumMeshlets"][0][0] = len(meshlets)
    sc = dict(instances=inst, meshData=md, meshlets=meshlets)
    rec = np.zeros(3, I.MeshletAmplificationData)
    rec["m_MeshletGroupOffset"] = [0, 32, 64]
    lst = np.array([(g << 5) | lane for g in range(3) for lane in range(32 if g < 2 else 1)], np.uint32)
    depth, vis, mot, _ = _direct(dev, k, sc, v, vid, tri, rec, lst, (W, H), slot=1)
    rdepth, rvis, rmot = _reference(vr, k, sc, v, vid, tri, rec, lst, (W, H), slot=1)
    assert np.array_equal(depth.view(np.uint32), rdepth.view(np.uint32))
    assert np.array_equal(vis, rvis)
    assert np.array_equal(mot, rmot)
    hidden = (vis >> np.uint64(32)).astype(np.uint32) < depth.view(np.uint32)
    assert hidden.sum() > 0.2 * hidden.size, "the near triangle must hide the texels' triangles over a large area"
    assert np.all(vis[hidden] != 0), "a texel behind the out-of-contract triangle was lost"
    assert np.all(vis != 0)


def test_host_path_with_animated_nodes(oracle, vr, tmp_path):
    """The C++ host mirror (trhost_set_visibility_buffer): five frames with animated node transforms and a moving camera.
    Texels equal the reference computed from Renderer.instances() and each frame's view; motion too from the second
    frame on (the first frame's previous projection is the host's initial one, not the test's).  Then the refusals."""
    from toyrenderer_amd import host
    s, _ = city(tmp_path, oracle)
    cam = s.cameras[0]
    render = (640, 360)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    hzb = oracle.HzbTexture(*I.hzb_dims(*render))
    depth = np.zeros((render[1], render[0]), np.float32)
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    with host_renderer(s, s.instances, geo_v, render=render, max_groups=4096) as r:
        r.set_visibility_buffer(True)
        r.set_culling(7)
        prevV = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
        slots = set()
        for f in range(5):
            V = synth.world_to_view((0.1 * f, 0.02 * f, -0.15 * f), cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            prevV = V
            nodes = s.nodes.copy()
            nodes["m_Position"][:, 0] += np.float32(0.04 * f) * (1 + np.arange(len(nodes)) % 3)
            r.set_node_transforms(nodes)
            r.set_camera(view)
            r.frame()
            got = r.results()
            inst = r.instances(len(s.instances))
            sc = dict(s.as_oracle()); sc["instances"] = inst
            ref = oracle.frame(sc, view.as_dict(), hzb, depth, cullingFlags=7, record_capacity=4096, maxGroups=4096,
                               raster=(I.world_to_clip(V, P), *geo_v))
            compare_frame(got, ref)
            k = consts(view)
            g = VR.Geometry(sc, *geo_v)
            vis_ref, _ = VR.frame_visibility(vr, k, g, ref, *render)
            vis = r.download_visibility()
            assert np.array_equal(vis, vis_ref), f"frame {f}: visibility differs in {int(np.count_nonzero(vis != vis_ref))} texels"
            assert np.array_equal((vis >> np.uint64(32)).astype(np.uint32), r.download_depth().view(np.uint32))
            slots |= set(np.unique(VR.decode(vis[vis != 0])[1]).tolist())
            if f > 0:
                assert not np.array_equal(inst["m_WorldMatrix"], inst["m_PrevWorldMatrix"]), "the nodes must move"
                m_ref = VR.to_half_bits(VR.frame_motion(vr, k, g, ref, vis_ref))
                m = r.download_motion().view(np.uint16)
                assert np.array_equal(m, m_ref), f"frame {f}: motion differs in {int(np.count_nonzero(m != m_ref))} words"
                assert np.count_nonzero(m) > 0.2 * m.size
        assert {0, 2} <= slots, slots
        # refusals with the visibility buffer on: more than 2^18 groups, a shard exchange
        with pytest.raises(host.HostError, match="2\\^18"):
            host._check(host.load().trhost_set_limits(1 << 19, 0))
        with pytest.raises(host.HostError, match="per rank"):
            host._check(host.load().trhost_exchange_create(ctypes.byref(host.ExchangeDesc())))


def test_host_path_refuses_a_shard_exchange_and_large_limits(oracle, tmp_path):
    from toyrenderer_amd import host
    s, _ = city(tmp_path, oracle)
    r = host.Renderer(render=(64, 32), max_groups=1 << 19)
    try:
        r.load_scene(s.instances, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
        r.load_geometry(s.vertices, s.meshletVertexIds, s.meshletTriangles)
        with pytest.raises(host.HostError, match="2\\^18"):
            r.set_visibility_buffer(True)
    finally:
        r.shutdown()
