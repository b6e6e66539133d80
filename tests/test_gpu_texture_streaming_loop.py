"""Texture streaming on the GPU, the host loop: FrameDriver(gbuffer=True, streaming=...) over GpuScene.set_textures(...,
streaming=...) (toyrenderer_amd/streaming.py).  A static camera converges to the plain textured frame within the frame count derived
from the design (ceil(T / textures_per_frame) + LATENCY + 1), under poison, with the reference's feedback and the rule's maps in every
transient frame; a camera move brings new tiles and unmaps the old ones after exactly evict_after rounds; round-robin; misuse.
The same static-camera scene through the C++ host mirror (host.Renderer, trhost_set_texture_streaming) converges to the same words."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import alpha_test_scenes as A  # noqa: E402
import bc_blocks as B  # noqa: E402
import bc_ref  # noqa: E402
import material_texture_scenes as S  # noqa: E402
import texture_streaming_ref as TS  # noqa: E402
import texture_streaming_scenes as X  # noqa: E402
from suite_support import dev, host_renderer, ref_library, same, vr  # noqa: E402, F401
from toyrenderer_amd import streaming as ST  # noqa: E402
from visibility_scenes import consts  # noqa: E402

pytestmark = pytest.mark.gpu
ts = ref_library(TS)
POISON = 0xFF00FFFF


@pytest.fixture(scope="module")
def bc(tmp_path_factory):
    return bc_ref.load(tmp_path_factory.mktemp("bc_ref"))


def _scene(dev, quads, textures, mats, streaming):
    """A GpuScene of the quads (all opaque) with the textures of a tests/texture_streaming_scenes.py list, streamed or plain."""
    from toyrenderer_amd.frame import GpuScene
    sc = A.build([(q, "opaque") for q in quads], mats, [(t[1], t[2]) for t in textures])
    gs = GpuScene(dev, sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
    gs.set_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
    gs.set_textures(sc["textures"], streaming=streaming)
    gs.set_materials(sc["materials"])
    return gs


def _driver(dev, gs, view, **kw):
    from toyrenderer_amd.frame import FrameDriver
    return FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=1, gbuffer=True, **kw)


def _frame(drv):
    drv.record(); drv.run(); drv.results()
    return drv.gbufferA.download_mip(0)


def _plain(dev, quads, textures, mats, view):
    gs = _scene(dev, quads, textures, mats, None)
    drv = _driver(dev, gs, view)
    try:
        return _frame(drv)
    finally:
        drv.release(); gs.release()


def _ref_feedback(vr, ts, bc, quads, textures, mats, view):
    """{texture index: decoded bytes} of the reference for one frame: feedback does not depend on residency."""
    table, where = X.with_maps(textures)
    _, _, _, fb = X.reference(vr, ts, bc, consts(view), S.build(quads), mats(where), table)
    return {i: fb[where[i][1]] for i in where}


def _rule(ts, textures):
    return {i: TS.Residency(ts, *X.size_of(t[1]), len(t[1]), t[3], t[3][0] * t[3][1] * 4 if not hasattr(t[1], "width") else t[3][0] * t[3][1] // 16 * B.BLOCK_BYTES[t[2]])
            for i, t in enumerate(textures)}


def test_a_static_camera_converges_within_the_derived_frame_count(dev, vr, ts, bc):
    """T = 3 textures (sRGBA8, RGBA8, and BC1 in place of the third), textures_per_frame = 3: ceil(3 / 3) + LATENCY + 1 = 3 frames.  In every
    frame the device's feedback is the reference's and the min-mip maps are the rule's; the first frame shows the tail and the poison;
    the last equals the plain textured frame and its maps are the frame before's."""
    quads, textures, mats = X.loop_scene("three")
    textures[2] = X.texture(23, 16, 64, B.BC1)
    view = S.view()
    plain = _plain(dev, quads, textures, mats({}), view)
    want_fb = _ref_feedback(vr, ts, bc, quads, textures, mats, view)
    rule = _rule(ts, textures)
    gs = _scene(dev, quads, textures, mats({}), dict(region=X.REGION, poison=POISON))
    drv = _driver(dev, gs, view, streaming=dict(textures_per_frame=3, evict_after=2, poison=True))
    try:
        frames = math.ceil(len(textures) / 3) + ST.LATENCY + 1
        assert frames == 3 and [s.index for s in gs.streams] == [0, 1, 2]
        images, maps, uploaded = [], [], []
        for f in range(frames):
            images.append(_frame(drv))
            maps.append([drv.download_min_mip(i) for i in range(3)])
            uploaded.append(drv.streaming_stats["tilesUploaded"])
            for i in range(3):
                same(drv.download_feedback(i), want_fb[i], f"frame {f}: feedback of texture {i}")
                same(maps[f][i], rule[i].min_mip, f"frame {f}: min-mip map of texture {i}")
            for i in range(3):                                             # the next frame applies this frame's feedback
                rule[i].round(want_fb[i], 2)
        assert not np.array_equal(images[0], plain), "tail-only residency (and poison) shows in the first frame"
        same(images[-1], plain, "the converged frame against the plain textured frame")
        for i in range(3):
            same(maps[-1][i], maps[-2][i], f"the maps have stopped changing (texture {i})")
        assert uploaded[0] == 0 and uploaded[1] > 0 and uploaded[2] == 0, uploaded
        total = sum(r.total for r in rule.values())
        assert drv.streaming_stats["tilesTotal"] == total and 0 < drv.streaming_stats["tilesResident"] < total
        assert drv.streaming_stats["tilesResident"] == sum(int(r.resident[:r.total].sum()) for r in rule.values())
    finally:
        drv.release(); gs.release()


def test_a_camera_move_maps_new_tiles_and_unmaps_the_old_after_evict_after_rounds(dev, vr, ts, bc):
    """Two quads 40 units apart, each with its own texture; the camera looks at the first, then moves in front of the second.  The
    test runs the rule beside the driver on the feedback the driver itself read back: maps and statistics agree in every frame,
    the first quad's tiles leave in exactly the evict_after-th round that does not ask for them, and the image converges again."""
    evict_after = 3
    quads = [S.facing(z=-3.0, half=0.9, uv_lo=0.0, uv_hi=1.0, material=0, centre=(0.0, 0.0), world=X.turn()),
             S.facing(z=-3.0, half=0.9, uv_lo=-0.5, uv_hi=1.5, material=1, centre=(40.0, 0.1))]
    textures = [X.texture(71, 32, 32, S.SRGBA8), X.texture(72, 64, 32, B.BC3)]

    def mats(where):
        return np.concatenate([X.material(where, S.ALBEDO, (0, S.NONE, S.NONE, S.NONE)), X.material(where, S.ALBEDO | S.MR, (1, S.NONE, 1, S.NONE), wrap=(1, 1, 0, 1))])
    here, there = S.view(), S.view(eye=(40.0, 0.0, 0.0), prev_eye=(40.0, 0.0, 0.0))
    plain_there = _plain(dev, quads, textures, mats({}), there)
    rule = _rule(ts, textures)
    gs = _scene(dev, quads, textures, mats({}), dict(region=X.REGION, poison=POISON))
    drv = _driver(dev, gs, here, streaming=dict(textures_per_frame=2, evict_after=evict_after, poison=True))
    try:
        resident0 = []
        for f in range(3 + evict_after + 2):
            if f == 3:
                drv.view = there
            g = _frame(drv)
            seen = drv.streaming_history[-1]
            stats = [rule[i].round(seen[i], evict_after)[2] for i in sorted(seen)]
            for i in range(2):
                same(drv.download_min_mip(i), rule[i].min_mip, f"frame {f}: min-mip map of texture {i}")
            assert drv.streaming_stats["tilesUploaded"] == sum(s["tilesMapped"] for s in stats), f
            assert drv.streaming_stats["bytesUploaded"] == sum(s["bytesUploaded"] for s in stats), f
            assert drv.streaming_stats["tilesResident"] == sum(int(r.resident[:r.total].sum()) for r in rule.values()), f
            resident0.append(int(rule[0].resident[:rule[0].total].sum()))
        # frame 3 is the first that does not ask for texture 0; frame 4 applies it (round 1), so round evict_after is applied by frame 3 + evict_after
        assert all(n > 0 for n in resident0[1:3 + evict_after]) and resident0[3 + evict_after] == 0, resident0
        assert rule[1].resident[:rule[1].total].sum() > 0
        same(g, plain_there, "converged again after the move")
        assert np.all(drv.download_min_mip(0) == rule[0].S), "the first texture is back to its tail"
    finally:
        drv.release(); gs.release()


def test_round_robin_processes_every_texture(dev, vr, ts, bc):
    """textures_per_frame = 1 and three textures: each frame's read-back holds one texture, in turn, and the image converges within
    ceil(3 / 1) + LATENCY + 1 = 5 frames."""
    quads, textures, mats = X.loop_scene("three")
    view = S.view()
    plain = _plain(dev, quads, textures, mats({}), view)
    gs = _scene(dev, quads, textures, mats({}), dict(region=X.REGION, poison=POISON))
    drv = _driver(dev, gs, view, streaming=dict(textures_per_frame=1, evict_after=8, poison=True))
    try:
        frames = math.ceil(3 / 1) + ST.LATENCY + 1
        for f in range(frames):
            g = _frame(drv)
        assert [sorted(s) for s in drv.streaming_history] == [[], [0], [1], [2], [0]]
        same(g, plain, "converged")
    finally:
        drv.release(); gs.release()


def test_misuse_is_refused_by_name(dev):
    from toyrenderer_amd.frame import FrameDriver
    quads, textures, mats = X.loop_scene("floor")
    gs = _scene(dev, quads, textures, mats({}), dict(region=X.REGION))
    try:
        where = {s.index: (s.min_mip_index, s.feedback_index) for s in gs.streams}
        crossed = mats(where)
        crossed["m_AlbedoTexture"]["m_MinMapTextureDescriptorIndex"][0] = where[1][0]     # another texture's map
        with pytest.raises(ValueError, match="texture"):
            gs.set_materials(crossed)
        gs.set_materials(mats(where))                                                    # its own maps, named by the caller: accepted
        with pytest.raises(ValueError, match="alpha_test"):
            FrameDriver(dev, gs, S.view(), record_capacity=4096, culling_flags=1, gbuffer=True, alpha_test=True, streaming=dict(textures_per_frame=1))
        with pytest.raises(ValueError, match="gbuffer"):
            FrameDriver(dev, gs, S.view(), record_capacity=4096, culling_flags=1, visibility=True, streaming=dict(textures_per_frame=1))
    finally:
        gs.release()
    plain = _scene(dev, quads, textures, mats({}), None)
    try:
        with pytest.raises(ValueError, match="streamable"):
            _driver(dev, plain, S.view(), streaming=dict(textures_per_frame=1))
        with pytest.raises(ValueError, match="no multiple of the streaming region"):
            plain.set_textures([(t[1], t[2]) for t in textures], streaming=dict(region=(128, 8)))
    finally:
        plain.release()


def test_the_host_mirror_converges_to_the_same_words(dev, oracle):
    """tests/material_texture_scenes.py's glTF with images of 32 x 32, 64 x 32 and 16 x 16 (five textures, regions of 8 x 8) under its
    own static camera: host.Renderer with trhost_set_texture_streaming shows tail and poison in its first frame and, within
    ceil(T / textures_per_frame) + LATENCY + 1 frames, the plain textured frame of FrameDriver, word for word; its min-mip maps
    and resident tiles are those of the streamed Python driver; and the mirror's refusals name their cause."""
    from toyrenderer_amd import gltf_lite, host
    g, blobs, _ = S.textured_gltf()
    r8 = np.random.default_rng(77)
    images = [r8.integers(0, 256, (h, w, 4), dtype=np.uint16).astype(np.uint8) for w, h in ((32, 32), (64, 32), (16, 16))]
    images[0][..., :2] = 70 + images[0][..., :2] % 116                      # also read as a normal map
    s = gltf_lite.load(g, blobs, lods=False, images=images)
    inst = gltf_lite.apply_materials(s)
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    view = gltf_lite.view_of(s.cameras[0], S.RENDER)
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    T = len(s.textures)
    frames = math.ceil(T / T) + ST.LATENCY + 1

    def python_driver(streaming):
        from toyrenderer_amd.frame import FrameDriver, GpuScene
        gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
        gs.set_geometry(*geo_v)
        gs.set_textures(s.textures, streaming=dict(region=X.REGION, poison=POISON) if streaming else None)
        gs.set_materials(s.materials)
        drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, gbuffer=True,
                          **(dict(streaming=dict(textures_per_frame=T, evict_after=2, poison=True)) if streaming else {}))
        try:
            for _ in range(frames if streaming else 1):
                g = _frame(drv)
            return g, ([drv.download_min_mip(i) for i in range(T)], drv.streaming_stats) if streaming else None
        finally:
            drv.release(); gs.release()
    want, _ = python_driver(False)
    streamed, (maps, stats) = python_driver(True)
    same(streamed, want, "the Python driver, streamed, against its plain frame")
    assert (want[..., 0] != 0).sum() > 1200
    with host_renderer(s, inst, geo_v, render=S.RENDER, max_groups=4096) as r:
        r.set_texture_streaming(True, textures_per_frame=T, evict_after=2, poison=True, region=X.REGION)
        assert r.load_textures(s.textures) == list(range(T))
        crossed = s.materials.copy(); crossed["m_AlbedoTexture"]["m_MinMapTextureDescriptorIndex"][0] = 1
        with pytest.raises(host.HostError, match="texture"):
            r.load_materials(crossed)                                    # index 1 is a texture, not the map of texture 0
        r.load_materials(s.materials)
        r.set_gbuffer(True)
        with pytest.raises(host.HostError, match="streaming"):
            r.set_alpha_test(True)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        r.set_camera(view)
        got = []
        for f in range(frames):
            r.frame(); r.results()
            got.append(r.download_gbuffer_a())
        assert not np.array_equal(got[0], want), "tail-only residency (and poison) shows in the first frame"
        same(got[-1], want, "host mirror: the converged frame against the plain textured frame")
        for i in range(T):
            same(r.download_min_mip(i), maps[i], f"host mirror: min-mip map of texture {i} against the Python driver's")
        hs = r.streaming_stats
        assert hs["tilesTotal"] == stats["tilesTotal"] and hs["tilesResident"] == stats["tilesResident"] and 0 < hs["tilesResident"] < hs["tilesTotal"], (hs, stats)
        assert hs["tilesUploaded"] == 0 and hs["texturesProcessed"] == T, hs
    with host_renderer(s, inst, geo_v, render=S.RENDER, max_groups=4096) as r:
        r.set_texture_streaming(True, textures_per_frame=1, evict_after=2, region=(128, 8))
        with pytest.raises(host.HostError, match="no multiple of the streaming region"):
            r.load_textures(s.textures)
