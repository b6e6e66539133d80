"""The probe visualisation on the GPU ("giprobevisualization_CS_LoadGIProbes", "giprobevisualization_PS_VisualizeGIProbes";
csrc/k_giprobedraw.hip), every word against tests/ddgi_probe_draw_ref.c: LoadGIProbes dispatched alone on volumes of 1, 2, 3, 33 and
3 x 2 x 4 probes under each combination of the two flags, the draw dispatched alone on the scenes of tests/ddgi_probe_draw_scenes.py at
two sizes, three whole frames on the Cornell fixture through FrameDriver(probes=...) and two through the host mirror, what is recorded
with the option off, and misuse."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_placement_scenes as PS  # noqa: E402
import ddgi_probe_draw_ref as PD  # noqa: E402
import ddgi_probe_draw_scenes as S  # noqa: E402
import ddgi_update_scenes as US  # noqa: E402
import shadow_scenes as SS  # noqa: E402
from suite_support import dev, gpu_scene, recorded, ref_library, same  # noqa: E402, F401
from toyrenderer_amd import ddgi, gltf_lite  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
pd = ref_library(PD)
LOAD, CULL, DRAW = "giprobevisualization_CS_LoadGIProbes", "giprobevisualization_CS_VisualizeGIProbesCulling", "giprobevisualization_PS_VisualizeGIProbes"
GUARD = 0xA5A5A5A5


def _desc_cb(cl, vol):
    return cl.constant_buffer(np.frombuffer(vol.desc().tobytes(), np.uint8), "DDGIVolumeDesc")


# ---- 1. LoadGIProbes, dispatched alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", PS.RAGGED_COUNTS + [(3, 2, 4)], ids=lambda c: f"{int(np.prod(c))} probes")
def test_loaded_probes_match_the_reference(dev, pd, counts):
    """Positions and states word for word under each combination of the relocation and classification flags, from seeded non-zero
    offsets and states; 33 probes is the ragged last group.  The words behind the last probe keep their guard."""
    from toyrenderer_amd.rhi import CB, SRV, TEX_SRV, UAV
    n = int(np.prod(counts))
    for relocation in (False, True):
        for classification in (False, True):
            vol = S.volume(seed=n, counts=counts, relocation=relocation, classification=classification)
            assert np.any(vol.data[..., :3] != 0) and (n < 3 or np.any(vol.data[..., 3] == 1))
            desc, data, irr, dist = vol.upload(dev)
            positions, states = dev.create_buffer(12 * n + 16, "positions", stride=4), dev.create_buffer(4 * n + 16, "states")
            positions.upload(np.full(3 * n + 4, GUARD, np.uint32)); states.upload(np.full(n + 4, GUARD, np.uint32))
            cl = dev.create_command_list()
            try:
                cl.open()
                cl.dispatch(LOAD, [CB(0, _desc_cb(cl, vol)), SRV(0, desc), TEX_SRV(1, data), UAV(0, positions), UAV(1, states)], ((n + 31) // 32, 1, 1))
                cl.close()
                dev.execute(cl); dev.wait_idle()
                want_pos, want_states = PD.load_probes(pd, vol)
                what = f"{counts}, relocation {relocation}, classification {classification}"
                same(positions.download(np.uint32), np.r_[want_pos.view(np.uint32).reshape(-1), [GUARD] * 4], what + ": positions")
                same(states.download(np.uint32), np.r_[want_states.view(np.uint32), [GUARD] * 4], what + ": states")
            finally:
                cl.release()
                for r in (desc, data, irr, dist, positions, states):
                    r.release()


# ---- 2. the draw, dispatched alone --------------------------------------------------------------------------------------------------------
class Draw:
    """One scene's device resources and the draw through rhi bindings.  capacity: entries of t0 and t5."""

    def __init__(self, dev, s, capacity=None, sphere=None):
        from toyrenderer_amd import rhi
        self.dev, self.s, vol = dev, s, s["vol"]
        H, W = s["depth"].shape
        self.desc, self.data, self.irr, self.dist = vol.upload(dev)
        n = len(s["positions"]) if capacity is None else capacity
        self.positions = dev.buffer_from(np.ascontiguousarray(s["positions"][:n], F), "culled positions", uav=False)
        self.to_probe = dev.buffer_from(np.ascontiguousarray(s["to_probe"][:n], np.uint32), "instance to probe", uav=False)
        self.args = dev.buffer_from(np.array([I.kUnitSphereIndices, s["count"], 0, 0, 0], np.uint32), "draw args", uav=False)
        v, ix = ddgi.unit_sphere() if sphere is None else sphere
        self.vertices, self.indices = dev.buffer_from(v, "sphere vertices", uav=False), dev.buffer_from(ix, "sphere indices", uav=False)
        self.depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
        self.color = dev.create_texture(W, H, 1, rhi.FORMAT_RGBA8_UNORM, "Back Buffer")
        self.winners = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "Probe Draw Winners")
        self.cl = dev.create_command_list()
        self.k = PD.consts(s["world_to_clip"], s["radius"], s["near"])

    def block(self, cl, k=None, desc=None):
        return cl.constant_buffer(np.frombuffer((self.k if k is None else k).tobytes() + (self.s["vol"].desc() if desc is None else desc).tobytes(), np.uint8), "GIProbeVisualizationConsts")

    def bindings(self, cb, winners=True):
        from toyrenderer_amd.rhi import CB, SRV, TEX_SRV, TEX_UAV
        b = [CB(0, cb), SRV(0, self.positions), TEX_SRV(1, self.data), TEX_SRV(2, self.irr), TEX_SRV(3, self.dist), SRV(4, self.desc), SRV(5, self.to_probe), SRV(6, self.args),
             SRV(7, self.vertices), SRV(8, self.indices), TEX_UAV(0, self.depth, 0), TEX_UAV(1, self.color, 0)]
        return b + ([TEX_UAV(2, self.winners, 0)] if winners else [])

    def run(self, winners=True):
        self.depth.upload_mip(0, self.s["depth"]); self.color.upload_mip(0, self.s["color"])
        self.winners.upload_mip(0, np.full(self.s["depth"].shape, 0xFFFFFFFFFFFFFFFF, np.uint64))     # the pass clears them itself
        self.cl.open()
        self.cl.dispatch(DRAW, self.bindings(self.block(self.cl), winners), (1, 1, 1))
        self.cl.close()
        self.dev.execute(self.cl); self.dev.wait_idle()
        return self.winners.download_mip(0), self.color.download_mip(0), self.depth.download_mip(0)

    def release(self):
        self.cl.release()
        for r in (self.desc, self.data, self.irr, self.dist, self.positions, self.to_probe, self.args, self.vertices, self.indices, self.depth, self.color, self.winners):
            r.release()


def _reference(pd, s, count=None, capacity=None):
    n = len(s["positions"]) if capacity is None else capacity
    return PD.draw(pd, PD.consts(s["world_to_clip"], s["radius"], s["near"]), s["vol"], s["positions"][:n], s["to_probe"][:n], s["count"] if count is None else count,
                   s["depth"], s["color"])


DRAWS = [(name, size, S.GAMMAS[0]) for name in S.SCENES for size in S.SIZES] + [(name, S.SIZES[1], S.GAMMAS[1]) for name in ("one", "two coincident", "everything")]


@pytest.mark.parametrize("name,size,gamma", DRAWS, ids=lambda x: x if isinstance(x, str) else f"{x[0]}x{x[1]}" if isinstance(x, tuple) else f"gamma {x}")
def test_the_draw_matches_the_reference(dev, pd, name, size, gamma):
    """The winner words, the back buffer and the depth buffer, every word: a seeded volume with filled borders, a seeded back buffer,
    the scene's depth buffer (none, a plane, or a plane and a step).  Texels without a winner keep the seeded colour and the scene's
    depth, which the comparison with the reference covers and the last line states again.  "large" covers most of the screen and
    "below half a pixel" nothing: the draw has no size switch, both take its one path."""
    s = S.scene(name, size, gamma)
    winners, color, depth, n = _reference(pd, s)
    assert all(n[c] for c in s["shows"]), (name, n)
    d = Draw(dev, s)
    try:
        got_winners, got_color, got_depth = d.run()
        same(got_winners, winners, f"{name} {size}: winner words")
        same(got_color, color, f"{name} {size}: back buffer")
        same(got_depth.view(np.uint32), depth.view(np.uint32), f"{name} {size}: depth")
        if name == "everything":                                      # without u2 the words live in scratch: the same image
            _, again_color, again_depth = d.run(winners=False)
            same(again_color, color, "no u2: back buffer"); same(again_depth.view(np.uint32), depth.view(np.uint32), "no u2: depth")
        none = got_winners == 0
        assert np.array_equal(got_color[none], s["color"][none]) and np.array_equal(got_depth[none], s["depth"][none])
    finally:
        d.release()


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_sample_at_exactly_the_scene_depth_survives(dev, pd, size):
    """The depth buffer holds the sphere's own depth where the sphere lies: every sample ties the scene and GREATER_OR_EQUAL keeps
    every winner (where two triangles share an edge through a pixel centre, the one with the smaller depth loses as it did before),
    so the image is the one over an empty depth buffer."""
    s = S.on_its_own_depth(lambda sc: _reference(pd, sc), size)
    winners, color, depth, n = _reference(pd, s)
    assert n["won"] == _reference(pd, S.scene("one", size))[3]["won"] > 0 and np.array_equal(depth, s["depth"])
    d = Draw(dev, s)
    try:
        got_winners, got_color, got_depth = d.run()
        same(got_winners, winners, f"{size}: winner words")
        same(got_color, color, f"{size}: back buffer")
        same(got_depth.view(np.uint32), depth.view(np.uint32), f"{size}: depth")
    finally:
        d.release()


def test_an_instance_count_above_the_capacity_is_clamped(dev, pd):
    """m_InstanceCount = 1000 over a t0 and a t5 of a few entries: the image is the reference's of as many instances as the smaller
    of the two holds, so the entries the larger one has beyond that (they would draw more spheres) are not read as instances and
    nothing past either buffer is read at all; no winner word names an instance at or above the capacity."""
    s = S.scene("everything", S.SIZES[0])
    s["count"] = 1000
    for cap_positions, cap_index in ((5, 5), (5, 3), (4, 6)):
        cap = min(cap_positions, cap_index)
        winners, color, depth, n = _reference(pd, s, count=cap, capacity=cap)
        assert n["won"] > 0
        d = Draw(dev, s, capacity=cap)
        try:
            d.positions.release(); d.to_probe.release()
            d.positions = dev.buffer_from(np.ascontiguousarray(s["positions"][:cap_positions], F), "culled positions", uav=False)
            d.to_probe = dev.buffer_from(np.ascontiguousarray(s["to_probe"][:cap_index], np.uint32), "instance to probe", uav=False)
            got_winners, got_color, got_depth = d.run()
            same(got_winners, winners, f"capacity {cap}: winner words")
            same(got_color, color, f"capacity {cap}: back buffer")
            same(got_depth.view(np.uint32), depth.view(np.uint32), f"capacity {cap}: depth")
            assert int((got_winners >> np.uint64(8) & np.uint64(0xFFFFFF)).max()) < cap
        finally:
            d.release()


# ---- 3. whole frames ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell(dev, oracle):
    sc = SS.cornell()
    s = sc["loaded"]
    inst = sc["instances"].copy()
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    sc["instances"] = inst
    s.meshData = sc["meshData"]
    gs = gpu_scene(dev, s, inst, s.vertices, sc["materials"])
    gs.set_raytracing(sc["indices"], sc["cached"].meshSpecific)
    yield sc, gs
    gs.release()


RENDER = (64, 36)
RADIUS = 0.06
HIDING_RADIUS = 0.3                                # see test_three_frames_through_the_driver
UPDATE = dict(seed=13, relocate=True, classify=True, min_frontface_distance=0.1)


def _frame_reference(oracle, pd, vol, k_cull, k_draw, hzb_texels, view, depth, color):
    """(positions, states, culled positions, draw args, instance -> probe, winners, colour, depth, counters) of one frame's three passes
    from the volume as the update left it, the frame's HZB and what the frame held in front of the draw."""
    pos, states = PD.load_probes(pd, vol)
    hzb = oracle.HzbTexture(*view.hzb_dims)
    hzb.texels[:] = hzb_texels
    out_pos, args, out_idx = oracle.gi_probe_cull(k_cull, pos, states, hzb, draw_args=np.array([I.kUnitSphereIndices, 0, 0, 0, 0], np.uint32))
    n = len(pos)
    full_pos, full_idx = np.zeros((n, 3), F), np.zeros(n, np.uint32)
    full_pos[:len(out_idx)], full_idx[:len(out_idx)] = out_pos.reshape(-1, 3), out_idx
    return (pos, states, out_pos.reshape(-1, 3), args, out_idx) + PD.draw(pd, k_draw, vol, full_pos, full_idx, int(args[1]), depth, color)


def test_three_frames_through_the_driver(dev, oracle, pd, cornell):
    """Cornell at 64 x 36 through FrameDriver(lighting, post, ddgi, ddgi_update with relocation and classification, probes): after each of
    three frames the loaded positions and states, the cull's three outputs, the winner words, the back buffer and the depth equal the
    reference fed the volume as downloaded after that frame.  What the frame held in front of the draw comes from a twin driver
    without probes=, whose frames are the same bit for bit.  The spheres move with relocation.  A third driver hides the inactive
    probes, with a radius at which the switched-off probes inside the blocks and above the ceiling reach out of what occludes
    them: it matches the reference too, and draws fewer spheres than the same cull keeps with the switch off."""
    from toyrenderer_amd.frame import FrameDriver
    sc, gs = cornell
    cam = sc["camera"]
    view = gltf_lite.view_of(cam, RENDER)
    common = dict(record_capacity=4096, culling_flags=7, lighting=True, post=True, dir_light=US.LIGHT, camera_origin=tuple(float(x) for x in cam.position), ddgi_update=UPDATE)
    drv = FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), probes=dict(radius=RADIUS), **common)
    hiding = FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), probes=dict(radius=HIDING_RADIUS, hide_inactive=True), **common)
    twin = FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), **common)
    try:
        last, moved, dropped = PS.tight_volume().probe_positions_and_states()[0], 0, 0
        for f in range(3):
            for d in (drv, hiding, twin):
                d.record(); d.run(); d.results()
            vol = drv.download_ddgi()
            before_color, before_depth = twin.back_buffer.download_mip(0), twin.depth.download_mip(0)
            pos, states, culled, args, to_probe, winners, color, depth, n = _frame_reference(oracle, pd, vol, drv.probe_cull_consts, drv.probe_draw_consts, drv.hzb.download_chain(),
                                                                                              view, before_depth, before_color)
            same(drv.probe_positions.download(np.uint32), pos.view(np.uint32).reshape(-1), f"frame {f}: positions")
            same(drv.probe_states.download(np.uint32), states.view(np.uint32), f"frame {f}: states")
            same(drv.probe_draw_args.download(np.uint32, 5), args, f"frame {f}: draw arguments")
            count, got_culled, got_to_probe = drv.download_probes()
            assert count == int(args[1]) > 0 and int(args[0]) == 468
            same(got_to_probe, to_probe, f"frame {f}: instance -> probe"); same(got_culled.view(np.uint32), culled.view(np.uint32), f"frame {f}: culled positions")
            same(drv.download_probe_winners(), winners, f"frame {f}: winner words")
            same(drv.back_buffer.download_mip(0), color, f"frame {f}: back buffer")
            same(drv.depth.download_mip(0).view(np.uint32), depth.view(np.uint32), f"frame {f}: depth")
            assert n["won"] > 0 and n["lost_to_scene"] > 0, n
            moved += int(np.any(pos != last, axis=1).sum())
            last = pos
            hidden = _frame_reference(oracle, pd, vol, hiding.probe_cull_consts, hiding.probe_draw_consts, hiding.hzb.download_chain(), view, before_depth, before_color)
            shown = hiding.probe_cull_consts.copy()
            shown["m_bHideInactiveProbes"] = 0
            kept = int(_frame_reference(oracle, pd, vol, shown, hiding.probe_draw_consts, hiding.hzb.download_chain(), view, before_depth, before_color)[3][1])
            assert np.any(states == 1.0) and hiding.download_probes()[0] == int(hidden[3][1]) <= kept, (int(hidden[3][1]), kept)
            dropped += kept - int(hidden[3][1])
            same(hiding.back_buffer.download_mip(0), hidden[6], f"frame {f}, inactive hidden: back buffer")
        assert moved > 0, "relocation moved no probe"
        assert dropped > 0, "hiding the inactive probes hid none that the cull keeps"
        assert drv.probe_draw_consts.tobytes()[76:84] == F(RADIUS).tobytes() + F(view.nearPlane).tobytes()
    finally:
        for d in (drv, hiding, twin):
            d.release()


def test_two_frames_through_the_host_mirror(oracle, pd):
    """The same through host.Renderer with trhost_set_ddgi_probe_visualization: two frames' cull outputs against the reference fed the
    downloaded volume, under the block trhost_get_ddgi_probe_visualization_consts shows; without a volume or without post-processing
    the next frame says which is missing; switched off again, the frame has the passes it had."""
    from suite_support import host_renderer
    from toyrenderer_amd import host
    sc = SS.cornell()
    s = sc["loaded"]
    s.meshData = sc["meshData"]
    view = gltf_lite.view_of(sc["camera"], RENDER)
    vol = PS.tight_volume()
    with host_renderer(s, gltf_lite.apply_materials(s), (s.vertices, s.meshletVertexIds, s.meshletTriangles), sc["materials"], render=RENDER, max_groups=4096) as r:
        r.set_deferred_lighting(True)
        r.set_directional_light(*US.LIGHT)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        r.set_camera(view)
        r.frame(); r.results()
        plain = r.render_graph_stats()["passes"]
        r.set_ddgi_probe_visualization(True, RADIUS, False)
        with pytest.raises(host.HostError, match="probe visualisation.*no DDGI volume"):
            r.frame()
        r.upload_ddgi_volume(vol)
        r.set_ddgi(True)
        with pytest.raises(host.HostError, match="probe visualisation.*post-processing is off"):
            r.frame()
        r.set_ddgi_probe_visualization(False, RADIUS, False)
        r.set_post_process(True)
        r.load_raytracing(sc["indices"], sc["cached"].meshSpecific)
        r.set_ddgi_update(True, seed=6)
        r.set_ddgi_probe_placement(True, True, 0.1, 0.25)
        r.frame(); r.results()
        off = r.render_graph_stats()["passes"]
        r.set_ddgi_probe_visualization(True, RADIUS, False)
        for f in range(2):
            r.frame(); r.results()
            assert r.render_graph_stats()["passes"] == off + 1
            k = r.ddgi_probe_visualization_consts()
            assert k["m_ProbeRadius"][0] == F(RADIUS) and k["m_NearPlane"][0] == F(view.nearPlane)
            same(k["m_WorldToClip"][0].view(np.uint32), I.world_to_clip(view.worldToView, view.viewToClip).view(np.uint32), "m_WorldToClip")
            got = r.download_ddgi_volume(vol)
            pos, states = PD.load_probes(pd, got)
            got_pos, got_args, got_idx = r.gi_probe_results()
            assert int(got_args[0]) == 468 and 0 < int(got_args[1]) <= len(pos)
            same(got_pos.view(np.uint32), pos[got_idx].view(np.uint32), f"host frame {f}: culled positions are the live volume's")
        r.set_ddgi_probe_visualization(False, RADIUS, False)
        r.frame(); r.results()
        assert r.render_graph_stats()["passes"] == off and off > plain


# ---- 4. option off ------------------------------------------------------------------------------------------------------------------------
def test_with_the_option_off_the_frame_records_what_it_did(dev, oracle, cornell):
    """probes absent and probes=None: the same commands and the same constant blocks; with it the three dispatches follow the post pass,
    in the order load, cull, draw.  probes= without ddgi= or without post= is refused."""
    from toyrenderer_amd.frame import FrameDriver
    sc, gs = cornell
    view = gltf_lite.view_of(sc["camera"], RENDER)
    common = dict(record_capacity=4096, culling_flags=7, lighting=True, post=True, dir_light=US.LIGHT, ddgi_update=dict(seed=4))
    made = [FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), **common), FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), probes=None, **common),
            FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), probes=dict(radius=RADIUS), **common)]
    try:
        absent, none, on = (recorded(d) for d in made)
        assert absent == none and on[:len(absent)] == absent and [shader for _, shader in on[len(absent):] if shader] == [LOAD, CULL, DRAW]
        assert absent[-1][1] == "postprocess_PS_PostProcess"
        for name in ("lighting_consts", "ddgi_update_consts"):
            assert getattr(made[0], name).tobytes() == getattr(made[1], name).tobytes() == getattr(made[2], name).tobytes()
        for a, b, c in zip(made[0].post_consts, made[1].post_consts, made[2].post_consts):
            assert (a is None and b is None and c is None) or a.tobytes() == b.tobytes() == c.tobytes()
        assert made[0].probes is None and made[1].probe_winners is None and made[1].probe_draw_consts is None
        with pytest.raises(ValueError, match="download_probes: the probe visualisation is off"):
            made[1].download_probes()
    finally:
        for d in made:
            d.release()
    with pytest.raises(ValueError, match="probes=... needs ddgi=ddgi.Volume"):
        FrameDriver(dev, gs, view, probes=dict(radius=RADIUS), record_capacity=4096, lighting=True, post=True)
    with pytest.raises(ValueError, match="probes=... needs post=True"):
        FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), probes=dict(radius=RADIUS), record_capacity=4096, lighting=True)
    with pytest.raises(ValueError, match="probes: unknown settings"):
        FrameDriver(dev, gs, view, ddgi=PS.tight_volume(), probes=dict(size=1), record_capacity=4096, lighting=True, post=True)


# ---- 5. misuse ----------------------------------------------------------------------------------------------------------------------------
def test_misuse_of_the_passes_is_refused(dev):
    """A short or missing block, a wrong group count, outputs too small for the probe count, a wrong array format at each new slot, an
    array texture at an undeclared slot, a wrong depth or back buffer format, a back buffer or winner texture of another size, and
    sphere buffers of no sphere: each is refused with the pass's name."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, SRV, TEX_SRV, TEX_UAV, UAV
    s = S.scene("one", S.SIZES[0])
    vol = s["vol"]
    n = int(np.prod(vol.counts))
    d = Draw(dev, s)
    made = []

    def keep(r):
        made.append(r)
        return r

    def swap(bindings, kind, slot, new):
        return [b for b in bindings if not (b.type == kind and b.slot == slot)] + ([new] if new is not None else [])

    cl = d.cl
    cl.open()
    try:
        positions, states = keep(dev.create_buffer(12 * n, "positions", stride=12)), keep(dev.create_buffer(4 * n, "states"))
        small_pos, small_states = keep(dev.create_buffer(12 * n - 12, "small positions", stride=12)), keep(dev.create_buffer(4 * n - 4, "small states"))
        rg = keep(dev.create_texture_array(3, 3, 2, rhi.FORMAT_RG16_FLOAT, "wrong format"))
        plain = keep(dev.create_texture(3, 3, 1, rhi.FORMAT_RGBA16_FLOAT, "plain"))
        W, H = S.SIZES[0]
        other_size = keep(dev.create_texture(W + 1, H, 1, rhi.FORMAT_RGBA8_UNORM, "other size"))
        other_winners = keep(dev.create_texture(W, H + 1, 1, rhi.FORMAT_RG32_UINT, "other winners"))
        half_depth = keep(dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, "half depth"))
        float_color = keep(dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "float colour"))
        odd_vertices, many_vertices = keep(dev.create_buffer(36, "odd vertices")), keep(dev.create_buffer(32 * 129, "129 vertices", stride=32))
        four_indices, many_indices = keep(dev.create_buffer(16, "four indices")), keep(dev.create_buffer(12 * 257, "257 triangles"))
        short_args = keep(dev.create_buffer(16, "short draw args"))
        load = [CB(0, _desc_cb(cl, vol)), SRV(0, d.desc), TEX_SRV(1, d.data), UAV(0, positions), UAV(1, states)]
        groups = ((n + 31) // 32, 1, 1)
        bad_desc = vol.desc().copy()
        bad_desc["probeCounts"] = (3, 0, 3)
        cases = [(LOAD, "64-byte DDGIVolumeDesc\\) missing or short", swap(load, rhi.BIND_CONSTANT_BUFFER, 0, None), groups),
                 (LOAD, "missing or short", swap(load, rhi.BIND_CONSTANT_BUFFER, 0, CB(0, cl.constant_buffer(np.zeros(60, np.uint8), "short"))), groups),
                 (LOAD, "not in 1..1024", swap(load, rhi.BIND_CONSTANT_BUFFER, 0, CB(0, cl.constant_buffer(np.frombuffer(bad_desc.tobytes(), np.uint8), "bad"))), groups),
                 (LOAD, "direct dispatch of", load, (groups[0] + 1, 1, 1)),
                 (LOAD, "t0 = the 64-byte DDGIVolumeDesc", swap(load, rhi.BIND_STRUCTURED_SRV, 0, None), groups),
                 (LOAD, "t1 = the RGBA16_FLOAT", swap(load, rhi.BIND_TEXTURE_SRV, 1, None), groups),
                 (LOAD, "not an array", swap(load, rhi.BIND_TEXTURE_SRV, 1, TEX_SRV(1, plain)), groups),
                 (LOAD, "declares an RGBA16_FLOAT array texture there", swap(load, rhi.BIND_TEXTURE_SRV, 1, TEX_SRV(1, rg)), groups),
                 (LOAD, "declares no array texture there", load + [TEX_SRV(2, d.irr)], groups),
                 (LOAD, "u0 = the probe positions", swap(load, rhi.BIND_STRUCTURED_UAV, 1, None), groups),
                 (LOAD, f"{n} probes need", swap(load, rhi.BIND_STRUCTURED_UAV, 0, UAV(0, small_pos)), groups),
                 (LOAD, f"{n} probes need", swap(load, rhi.BIND_STRUCTURED_UAV, 1, UAV(1, small_states)), groups)]
        draw = d.bindings(d.block(cl))
        one = (1, 1, 1)
        cases += [(DRAW, "160 bytes\\) missing or short", swap(draw, rhi.BIND_CONSTANT_BUFFER, 0, None), one),
                  (DRAW, "missing or short", swap(draw, rhi.BIND_CONSTANT_BUFFER, 0, CB(0, cl.constant_buffer(np.zeros(96, np.uint8), "short"))), one),
                  (DRAW, "not in 1..1024", swap(draw, rhi.BIND_CONSTANT_BUFFER, 0, CB(0, d.block(cl, desc=bad_desc))), one),
                  (DRAW, "t0 = the culled probe positions", swap(draw, rhi.BIND_STRUCTURED_SRV, 5, None), one),
                  (DRAW, "t4 = the 64-byte DDGIVolumeDesc", swap(draw, rhi.BIND_STRUCTURED_SRV, 4, None), one),
                  (DRAW, "t6 = the DrawIndexedIndirectArguments", swap(draw, rhi.BIND_STRUCTURED_SRV, 6, None), one),
                  (DRAW, "t6 = the DrawIndexedIndirectArguments", swap(draw, rhi.BIND_STRUCTURED_SRV, 6, SRV(6, short_args)), one),
                  (DRAW, "t7 = the unit sphere's vertices", swap(draw, rhi.BIND_STRUCTURED_SRV, 8, None), one),
                  (DRAW, "the sphere has 1..128 vertices", swap(draw, rhi.BIND_STRUCTURED_SRV, 7, SRV(7, odd_vertices)), one),
                  (DRAW, "the sphere has 1..128 vertices", swap(draw, rhi.BIND_STRUCTURED_SRV, 7, SRV(7, many_vertices)), one),
                  (DRAW, "the sphere has 1..256 triangles", swap(draw, rhi.BIND_STRUCTURED_SRV, 8, SRV(8, four_indices)), one),
                  (DRAW, "the sphere has 1..256 triangles", swap(draw, rhi.BIND_STRUCTURED_SRV, 8, SRV(8, many_indices)), one),
                  (DRAW, "declares an RGBA16_FLOAT array texture there", swap(draw, rhi.BIND_TEXTURE_SRV, 1, TEX_SRV(1, rg)), one),
                  (DRAW, "declares an R10G10B10A2_UNORM array texture there", swap(draw, rhi.BIND_TEXTURE_SRV, 2, TEX_SRV(2, rg)), one),
                  (DRAW, "declares an RG16_FLOAT array texture there", swap(draw, rhi.BIND_TEXTURE_SRV, 3, TEX_SRV(3, d.data)), one),
                  (DRAW, "t2 = the R10G10B10A2_UNORM", swap(draw, rhi.BIND_TEXTURE_SRV, 2, None), one),
                  (DRAW, "t3 = the RG16_FLOAT", swap(draw, rhi.BIND_TEXTURE_SRV, 3, None), one),
                  (DRAW, "not an array", swap(draw, rhi.BIND_TEXTURE_SRV, 1, TEX_SRV(1, plain)), one),
                  (DRAW, "declares no array texture there", draw + [TEX_SRV(9, d.irr)], one),
                  (DRAW, "u0 = the R32_FLOAT depth buffer", swap(draw, rhi.BIND_TEXTURE_UAV, 0, TEX_UAV(0, half_depth, 0)), one),
                  (DRAW, "u0 = the R32_FLOAT depth buffer", swap(draw, rhi.BIND_TEXTURE_UAV, 0, None), one),
                  (DRAW, "u1 = the RGBA8_UNORM back buffer", swap(draw, rhi.BIND_TEXTURE_UAV, 1, TEX_UAV(1, float_color, 0)), one),
                  (DRAW, f"the back buffer at u1 is {W + 1}x{H}, the depth buffer at u0 is {W}x{H}", swap(draw, rhi.BIND_TEXTURE_UAV, 1, TEX_UAV(1, other_size, 0)), one),
                  (DRAW, f"the winner words at u2 are {W}x{H + 1}", swap(draw, rhi.BIND_TEXTURE_UAV, 2, TEX_UAV(2, other_winners, 0)), one)]
        for name, match, b, g in cases:
            with pytest.raises(rhi.TrhipError, match=match) as e:
                cl.dispatch(name, b, g)
            assert name in str(e.value), (match, str(e.value))
    finally:
        cl.close()
        for r in made:
            r.release()
        d.release()


# ---- 6. what fails without this feature ---------------------------------------------------------------------------------------------------
def test_the_feature_is_there():
    from toyrenderer_amd import host, rhi
    names = rhi.shader_names()
    assert LOAD in names and DRAW in names and CULL in names
    for symbol in ("trhost_set_ddgi_probe_visualization", "trhost_get_ddgi_probe_visualization_consts"):
        assert symbol in host.HOST_SYMBOLS
