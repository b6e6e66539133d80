"""The ray-traced shadow mask on the GPU ("raytracing_CS_RefitTLAS" and "shadowmask_CS_ShadowMask", csrc/k_shadowmask.hip), every
word against brute force over every triangle (tests/shadowmask_ref.c): the cases of tests/shadow_scenes.py (sizes around the 8 x 8
tile, BLAS shapes around the leaf capacity, TLAS sizes, light directions with zero and -0 components, soft and hard, the frame
counter's wrap), the alpha test, far depth, animated instances and whole frames through FrameDriver(shadows=...), the recorded command
list, the C++ host mirror and misuse.  The mask and the linear view depth are pre-filled with sentinels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lighting_ref as LR  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from shadow_passes import REFIT, TRACE, Pass as _Pass  # noqa: E402
from suite_support import bare_gpu_scene as _gpu_scene, dev, gpu_scene, lr, op_counts, recorded, same, shadow_case_reference, sm  # noqa: E402, F401
from toyrenderer_amd import accel, cached_scene, gltf_lite, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
# ---- 1. the cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SS.CASES, ids=lambda c: c[0])
def test_cases_match_brute_force(dev, sm, case):
    """The refit's node boxes and matrices equal the shadow_case_reference's bit for bit; every texel of the mask and of the linear view depth
    equals brute force; far texels keep the mask's sentinel."""
    sc, acc, k, depth, g, noise, mask, lvd = shadow_case_reference(sm, case)
    W, H = case[2]
    gs = _gpu_scene(dev, sc)
    p = _Pass(dev, gs, W, H, noise)
    try:
        got_mask, got_lvd = p.run(k, depth, g)
        nodes, records = p.structure()
        want_nodes, want_records = SR.refit(sm, acc)
        assert nodes.tobytes() == want_nodes.tobytes(), f"{case[0]}: TLAS nodes after the refit"
        assert records.tobytes() == want_records.tobytes(), f"{case[0]}: TLAS instances after the refit"
        same(got_mask, mask, f"{case[0]}: mask")
        same(got_lvd, lvd, f"{case[0]}: linear view depth")
        assert np.all(got_mask[depth == 0] == SR.SENTINEL8)
    finally:
        p.release(); gs.release()


# ---- 2. the alpha test ----------------------------------------------------------------------------------------------------------------------
def test_alpha_test_of_the_candidates_instance(dev, sm):
    """A roof over everything.  In the alpha-mask list with alpha below its cutoff it casts nothing, at and above the cutoff it
    casts; in the opaque list it casts whatever its alpha.  A second, opaque instance with another material sits in front of
    it in the instance buffer, so reading another instance's material would show."""
    W, H = 33, 17
    depth, g = SS.images(W, H, 5)
    noise = SS.noise_image()
    k = SS.consts(W, H, SS.LIGHTS["up"], True, 2)
    roof = SS.world_matrix(scale=(60.0, 1.0, 60.0), position=(0.0, 30.0, 0.0))
    speck = SS.world_matrix(scale=(0.01, 0.01, 0.01), position=(0.0, -50.0, 0.0))
    for lst, alpha, cutoff, casts in (("alpha", 0.25, 0.5, False), ("alpha", 0.5, 0.5, True), ("alpha", 0.75, 0.5, True), ("opaque", 0.25, 0.5, True),
                                      ("alpha", 0.0, 0.0, True)):
        mats = SS.materials()
        mats["m_ConstAlbedo"][0, 3], mats["m_AlphaCutoff"][0] = 1.0 - alpha, 1.0 - cutoff + (0.25 if casts else -0.25)      # the speck's: the opposite verdict
        mats["m_ConstAlbedo"][1, 3], mats["m_AlphaCutoff"][1] = alpha, cutoff
        sc = SS.make_scene([SS.quad(1.0), SS.tetrahedron()], [(1, speck, 0, "opaque"), (0, roof, 1, lst)], mats)
        acc = SR.Accel(sc)
        want, want_lvd, _ = SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE)
        assert np.all(want[depth != 0] == (0 if casts else 255)), (lst, alpha, cutoff)
        gs = _gpu_scene(dev, sc)
        p = _Pass(dev, gs, W, H, noise)
        try:
            got, got_lvd = p.run(k, depth, g)
            same(got, want, f"{lst} alpha {alpha} cutoff {cutoff}: mask")
            same(got_lvd, want_lvd, "linear view depth")
        finally:
            p.release(); gs.release()


# ---- 3. far depth -----------------------------------------------------------------------------------------------------------------------------
def test_far_depth_and_distant_texels(dev, sm):
    """depth 0.0f and -0.0f: the mask's sentinel survives and the linear view depth is 0x7BFF; a depth so small that the texel is
    farther than 65520 from the camera overflows to the binary16 infinity, as round-to-nearest-even does; NaN and negative depths go
    through the arithmetic like any other."""
    W, H = 9, 9
    sc = SS.scattered(3)
    acc = SR.Accel(sc)
    depth, g = SS.images(W, H, 6, far_share=0.0)
    flat = depth.reshape(-1)
    flat[:12] = [0.0, -0.0, 1e-7, 1.8e-6, 1.52e-6, 1.53e-6, 1e-30, np.nan, -0.5, np.inf, 1e-45, 0.0]
    noise = SS.noise_image()
    k = SS.consts(W, H, SS.LIGHTS["generic"], True, 1)
    want, want_lvd, _ = SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE)
    w = want_lvd.reshape(-1)
    assert w[0] == w[1] == w[11] == 0x7BFF and want.reshape(-1)[0] == want.reshape(-1)[1] == SR.SENTINEL8
    assert w[2] == 0x7C00 and w[6] == 0x7C00 and 0x7800 < w[3] < 0x7C00 and w[7] == w[9] == 0x7E00, [hex(int(x)) for x in w[:12]]
    gs = _gpu_scene(dev, sc)
    p = _Pass(dev, gs, W, H, noise)
    try:
        got, got_lvd = p.run(k, depth, g)
        same(got_lvd, want_lvd, "linear view depth")
        same(got, want, "mask")
    finally:
        p.release(); gs.release()


# ---- 4. frames through FrameDriver --------------------------------------------------------------------------------------------------------------
def _cornell_gpu(dev, oracle):
    sc = SS.cornell()
    s = sc["loaded"]
    inst = sc["instances"].copy()
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)                   # the matrices the frames of the other tests use
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    sc["instances"] = inst
    s.meshData = sc["meshData"]                                                  # with m_GlobalIndexBufferIdx
    gs = gpu_scene(dev, s, inst, s.vertices, sc["materials"])
    gs.set_raytracing(sc["indices"], sc["cached"].meshSpecific)
    return sc, gs


def _frame_reference(sm, sc, drv, instances, frame):
    acc = SR.Accel(sc)                                                           # the topology of the rest transforms, as set_raytracing built it
    depth, g = drv.depth.download_mip(0), drv.gbufferA.download_mip(0)
    k = accel.shadow_consts(I.clip_to_world(drv.view.worldToView, drv.view.viewToClip), drv.dir_light[0], drv.camera_origin, drv.view.renderW, drv.view.renderH,
                            drv.shadows, frame)
    assert drv.shadow_consts.tobytes() == k.tobytes()
    mask, lvd, _ = SR.trace(sm, k, acc, depth, g, drv.shadows["noise"], SR.BRUTE, instances=instances)
    return k, depth, g, mask, lvd


@pytest.mark.parametrize("debug_mode", [0, 11])
def test_cornell_frames_with_animation(dev, oracle, sm, lr, debug_mode):
    """Two frames of FrameDriver(lighting=True, shadows=...) on the Cornell box next to a shadows=None driver, one wall moved inwards
    and the other far outside its rest box between them: everything in front of the pass equals the shadows=None run, the
    mask and the linear view depth equal brute force with the frame's own matrices, LightingOutput equals the lighting shadow_case_reference
    fed that mask, and debug view 11 shows it."""
    from toyrenderer_amd.frame import FrameDriver
    sc, gs = _cornell_gpu(dev, oracle)
    cam = sc["camera"]
    view = gltf_lite.view_of(cam, (160, 90))
    light = SS.unit((0.25, 0.45, 0.9))                                         # through the box's open side
    common = dict(record_capacity=4096, culling_flags=7, lighting=True, debug_mode=debug_mode, dir_light=(light, 3.0), camera_origin=tuple(float(x) for x in cam.position))
    settings = dict(noise=SS.noise_image(4), ray_start_offset=0.01, soft=True, sun_angular_diameter=2.0)
    base, drv = FrameDriver(dev, gs, view, **common), FrameDriver(dev, gs, view, shadows=settings, **common)
    H, W = view.renderH, view.renderW
    try:
        assert base.shadow_mask_texture is None and base.shadow_consts is None
        with pytest.raises(ValueError, match="shadows=None"):
            base.download_shadow_mask()
        instances = sc["instances"].copy()
        seen = []
        for f in range(2):
            if f == 1:                                                            # animation: new matrices in the instance buffer
                instances["m_PrevWorldMatrix"] = instances["m_WorldMatrix"]
                rest = instances["m_WorldMatrix"].astype(np.float64)
                # the left wall comes inwards; the right wall goes far outside its rest box, in front of the opening, into the light
                instances["m_WorldMatrix"][1] = (rest[1] @ SS.world_matrix(position=(0.7, 0.0, 0.0))).astype(F)
                instances["m_WorldMatrix"][2] = (rest[2] @ SS.world_matrix(axis=(0, 1, 0), angle=0.4, position=(-0.6, 0.4, 2.6))).astype(F)
                gs.instances.upload(instances)
            drv.shadow_mask_texture.upload_mip(0, np.full((H, W), SR.SENTINEL8, np.uint8))
            drv.linear_view_depth.upload_mip(0, np.full((H, W), SR.SENTINEL16, np.uint16))
            for d in (base, drv):
                d.frame_counter = f
                d.record(); d.run(); d.results()
            what = f"cornell view {debug_mode} frame {f}"
            for name in ("gbufferA", "visibility"):
                same(getattr(drv, name).download_mip(0), getattr(base, name).download_mip(0), what + ": " + name)
            k, depth, g, mask, lvd = _frame_reference(sm, sc, drv, instances, f)
            same(depth.view(np.uint32), base.depth.download_mip(0).view(np.uint32), what + ": depth")
            same(drv.download_shadow_mask(), mask, what + ": mask")
            same(drv.linear_view_depth.download_mip(0), lvd, what + ": linear view depth")
            assert np.any(mask == 0) and np.any(mask == 255)
            same(drv.lighting_output.download_mip(0), LR.lighting(lr, drv.lighting_consts, g, depth, shadow=mask, motion=drv.motion.download_mip(0)),
                  what + ": LightingOutput")
            same(base.lighting_output.download_mip(0), LR.lighting(lr, base.lighting_consts, g, depth, motion=base.motion.download_mip(0)), what + ": LightingOutput, shadows=None")
            assert np.count_nonzero(drv.lighting_output.download_mip(0) != base.lighting_output.download_mip(0)) > 50
            seen.append(mask)
        assert np.count_nonzero(seen[0] != seen[1]) > 20                          # the moved boxes moved their shadows
    finally:
        base.release(); drv.release(); gs.release()


def test_a_moved_instance_grows_its_ancestors(dev, sm):
    """The single passes on a scattered scene whose instance 5 is moved far outside its rest box after set_raytracing(): the refit
    arrays equal the shadow_case_reference's and the mask equals brute force with the new matrices."""
    sc = SS.scattered(65)
    acc = SR.Accel(sc)
    W, H = 67, 35
    depth, g = SS.images(W, H, 21)
    noise = SS.noise_image()
    k = SS.consts(W, H, SS.LIGHTS["up"], False, 0)
    moved = sc["instances"].copy()
    moved["m_WorldMatrix"][5] = SS.world_matrix(scale=(6.0, 0.3, 8.0), position=(0.5, 40.0, -6.0))
    gs = _gpu_scene(dev, sc)
    p = _Pass(dev, gs, W, H, noise)
    try:
        first, _ = p.run(k, depth, g)
        same(first, SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE)[0], "rest: mask")
        gs.instances.upload(moved)
        got, got_lvd = p.run(k, depth, g)
        want, want_lvd, _ = SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE, instances=moved)
        nodes, records = p.structure()
        want_nodes, want_records = SR.refit(sm, acc, moved)
        assert nodes.tobytes() == want_nodes.tobytes() and records.tobytes() == want_records.tobytes()
        same(got, want, "moved: mask")
        same(got_lvd, want_lvd, "moved: linear view depth")
        assert np.count_nonzero(got != first) > 100
    finally:
        p.release(); gs.release()


def test_city_frame(dev, oracle, sm, lr, tmp_path):
    """The generated city at 48 x 27 through FrameDriver(lighting=True, ao, shadows): mask, linear view depth and LightingOutput."""
    from gbuffer_scenes import with_normals_and_materials
    from toyrenderer_amd.frame import FrameDriver
    from visibility_scenes import city
    s, sc0 = city(tmp_path, oracle, lods=False)
    v, sc0, mats = with_normals_and_materials(s, sc0)
    c = cached_scene.from_scene(s)
    s.meshData = c.meshData
    gs = gpu_scene(dev, s, sc0["instances"], v, mats)
    gs.set_raytracing(c.indices, c.meshSpecific)
    sc = dict(vertices=v, indices=c.indices, meshData=c.meshData, index_counts=c.meshSpecific["m_NumIndices"], instances=sc0["instances"], opaqueIds=s.opaqueIds,
              alphaMaskIds=s.alphaMaskIds, materials=mats)
    view = gltf_lite.view_of(s.cameras[0], (48, 27))
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, lighting=True, dir_light=(SS.unit((0.2, 0.35, -0.9)), 2.5), ao=dict(quality=1),
                      shadows=dict(noise=SS.noise_image(9), ray_start_offset=0.1))
    try:
        drv.frame_counter = 300
        drv.shadow_mask_texture.upload_mip(0, np.full((view.renderH, view.renderW), SR.SENTINEL8, np.uint8))       # far texels keep what the mask held
        drv.linear_view_depth.upload_mip(0, np.full((view.renderH, view.renderW), SR.SENTINEL16, np.uint16))
        drv.record(); drv.run(); drv.results()
        k, depth, g, mask, lvd = _frame_reference(sm, sc, drv, sc0["instances"], 300)
        assert k["m_NoisePhase"][0] == F(300 & 0xFF) * F(1.61803398875)
        same(drv.download_shadow_mask(), mask, "city: mask")
        same(drv.linear_view_depth.download_mip(0), lvd, "city: linear view depth")
        assert np.any(mask == 0) and np.any(mask == 255)
        same(drv.lighting_output.download_mip(0), LR.lighting(lr, drv.lighting_consts, g, depth, shadow=mask, ssao=drv.download_ssao()), "city: LightingOutput")
    finally:
        drv.release(); gs.release()


# ---- 5. the recorded command list --------------------------------------------------------------------------------------------------------------
def test_shadows_add_two_dispatches_in_front_of_the_lighting_dispatch(dev, oracle):
    """shadows=None records the parent's list, command for command, and launches the same kernels; shadows=... adds exactly the refit
    and the trace between the AO passes and the lighting dispatch."""
    from toyrenderer_amd.frame import FrameDriver
    sc, gs = _cornell_gpu(dev, oracle)
    view = gltf_lite.view_of(sc["camera"], (64, 36))
    seen, counts = {}, {}
    settings = dict(noise=SS.noise_image())
    try:
        for name, extra in (("parent", {}), ("none", dict(shadows=None)), ("shadows", dict(shadows=settings)), ("ao", dict(ao={})), ("both", dict(ao={}, shadows=settings))):
            drv = FrameDriver(dev, gs, view, record_capacity=4096, lighting=True, **extra)
            try:
                counts[name] = op_counts(dev, drv)
                seen[name] = recorded(drv)
            finally:
                drv.release()
        drv = FrameDriver(dev, gs, view, record_capacity=4096, gbuffer=True, shadows=settings)                # the G-buffer alone is enough
        try:
            seen["gbuffer"] = recorded(drv)
        finally:
            drv.release()
    finally:
        gs.release()
    assert seen["none"] == seen["parent"] and counts["none"] == counts["parent"]
    added = [("dispatch", REFIT), ("dispatch", TRACE)]
    at = seen["parent"].index(("dispatch", "deferredlighting_PS_Main"))
    assert seen["shadows"] == seen["parent"][:at] + added + seen["parent"][at:]
    assert counts["shadows"] == {**counts["parent"], REFIT + "#main": 1, TRACE + "#main": 1}
    at = seen["ao"].index(("dispatch", "deferredlighting_PS_Main"))
    assert seen["both"] == seen["ao"][:at] + added + seen["ao"][at:]
    assert seen["gbuffer"][-2:] == added


# ---- 6. the host mirror ---------------------------------------------------------------------------------------------------------------------
def test_host_path_over_three_frames(oracle, sm, tmp_path):
    """The C++ host mirror with a moving camera: frame 0 soft shadows, frame 1 off, frame 2 hard shadows with another offset.
    trhost_get_shadow_mask_consts equals the Python block (the camera position is the mirror's own m_Eye), trhost_download_shadow_mask
    equals brute force fed the frame's own depth and GBufferA, and the refusals of the facade each raise."""
    from gbuffer_scenes import with_normals_and_materials
    from toyrenderer_amd import host
    from visibility_scenes import city
    s, sc0 = city(tmp_path, oracle, lods=False)
    v, sc0, mats = with_normals_and_materials(s, sc0)
    c = cached_scene.from_scene(s)
    cam = s.cameras[0]
    render = (48, 27)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    inst_in = s.instances.copy()
    inst_in["m_MaterialDataIdx"] = sc0["instances"]["m_MaterialDataIdx"]
    sc = dict(vertices=v, indices=c.indices, meshData=c.meshData, index_counts=c.meshSpecific["m_NumIndices"], instances=sc0["instances"], opaqueIds=s.opaqueIds,
              alphaMaskIds=s.alphaMaskIds, materials=mats)
    acc = SR.Accel(sc)
    noise = SS.noise_image(2)
    light = SS.unit((0.2, 0.35, -0.9))
    r = host.Renderer(render=render, max_groups=4096)
    try:
        r.load_scene(inst_in, c.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
        r.load_nodes(s.nodes, s.primToNode)
        r.load_geometry(v, s.meshletVertexIds, s.meshletTriangles)
        r.load_materials(mats)
        with pytest.raises(host.HostError, match="G-buffer is off"):
            r.set_shadow_mask(True)
        r.set_deferred_lighting(True)
        with pytest.raises(host.HostError, match="no acceleration structure"):
            r.set_shadow_mask(True)
        with pytest.raises(host.HostError, match="whole triangles"):
            r.load_raytracing(c.indices[:-1], c.meshSpecific)
        r.load_raytracing(c.indices, c.meshSpecific)
        with pytest.raises(host.HostError, match="no blue noise"):
            r.set_shadow_mask(True)
        with pytest.raises(host.HostError, match="65536 bytes"):
            r.upload_blue_noise(noise[:64])
        r.upload_blue_noise(noise)
        for bad, match in ((dict(sun_angular_diameter=-1.0), "diameter"), (dict(sun_angular_diameter=float("nan")), "diameter"), (dict(ray_start_offset=-0.1), "offset"),
                           (dict(ray_start_offset=float("inf")), "offset")):
            with pytest.raises(host.HostError, match=match):
                r.set_shadow_mask(True, **bad)
        r.upload_shadow_mask(np.full((render[1], render[0]), 255, np.uint8))
        with pytest.raises(host.HostError, match="was uploaded"):
            r.set_shadow_mask(True)
        r.upload_shadow_mask(None)
        with pytest.raises(host.HostError, match="did not run"):
            r.shadow_mask_consts()
        with pytest.raises(host.HostError, match="did not run"):
            r.download_shadow_mask()
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        prevV = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
        settings = [dict(soft=True, sun_angular_diameter=1.5, ray_start_offset=0.1), None, dict(soft=False, sun_angular_diameter=0.533, ray_start_offset=0.02)]
        for f, setting in enumerate(settings):
            V = synth.world_to_view((0.1 * f, 0.02 * f, -0.15 * f), cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            prevV = V
            r.set_camera(view)
            r.set_directional_light(light, 2.0)
            if setting is None:
                r.set_shadow_mask(False)
            else:
                r.set_shadow_mask(True, **setting)
            r.frame()
            r.results()
            if setting is None:
                with pytest.raises(host.HostError, match="did not run"):
                    r.shadow_mask_consts()
                with pytest.raises(host.HostError, match="did not run"):
                    r.download_shadow_mask()
                continue
            k = r.shadow_mask_consts()
            want_k = accel.shadow_consts(I.clip_to_world(V, P), light, k["m_CameraPosition"][0], *render, {**setting, "noise": noise}, f + 1)   # the frame is counted before it is recorded
            assert k.tobytes() == want_k.tobytes(), f
            assert np.allclose(k["m_CameraPosition"][0], (0.1 * f, 0.02 * f, -0.15 * f), atol=1e-5)
            depth = r.download_depth()
            got = r.download_shadow_mask()
            mask, _, _ = SR.trace(sm, k, acc, depth, r.download_gbuffer_a(), noise, SR.BRUTE, mask=got)   # far texels keep what the mirror's texture held
            same(got, mask, f"frame {f}: mask")
    finally:
        r.shutdown()


# ---- 7. misuse at the back end -------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused(dev, sm):
    """Each refusal happens while the command is recorded, so no kernel is launched; a good pass directly behind is correct."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, TEX_SRV, TEX_UAV
    W, H = 32, 16
    sc = SS.scattered(8)
    acc = SR.Accel(sc)
    gs = _gpu_scene(dev, sc)
    noise = SS.noise_image()
    p = _Pass(dev, gs, W, H, noise)
    mk = lambda w, h, fmt, name: dev.create_texture(w, h, 1, fmt, name)                                   # noqa: E731
    small8, r8uint, r32, noise64 = mk(W // 2, H, rhi.FORMAT_R8_UNORM, "small mask"), mk(W, H, rhi.FORMAT_R8_UINT, "R8_UINT"), mk(W, H, rhi.FORMAT_R32_FLOAT, "R32"), \
        mk(64, 64, rhi.FORMAT_RGBA8_UNORM, "small noise")
    lvd_mips = dev.create_texture(W, H, 2, rhi.FORMAT_R16_FLOAT, "two mips")
    args = dev.create_buffer(12, "args", stride=12, indirect=True)
    cl = dev.create_command_list()
    k = SS.consts(W, H, SS.LIGHTS["generic"], True, 0)
    denoise = k.copy(); denoise["m_bDoDenoising"] = 1
    try:
        dev.profile_reset(); dev.profile_enable(True)
        cl.open()
        cb = cl.constant_buffer(k, "ShadowMaskConsts")
        short = cl.constant_buffer(k.view(np.uint32).reshape(-1)[:27].copy(), "short")
        cbd = cl.constant_buffer(denoise, "denoise")
        good = p.trace_bindings(cb)

        def without(kind, slot):
            return [b for b in good if not (b.type == kind and b.slot == slot)]

        def swapped(kind, slot, new):
            return without(kind, slot) + [new]
        bad = [("112 bytes", good[1:], p.groups()), ("112 bytes", [CB(0, short), *good[1:]], p.groups()), ("m_bDoDenoising", [CB(0, cbd), *good[1:]], p.groups()),
               ("covering 32x16", good, (3, 2, 1)), ("covering 32x16", good, (4, 1, 1)),
               ("R32_FLOAT depth", without(rhi.BIND_TEXTURE_SRV, 0), p.groups()), ("R32_FLOAT depth", swapped(rhi.BIND_TEXTURE_SRV, 0, TEX_SRV(0, p.lvd)), p.groups()),
               ("GBufferA", without(rhi.BIND_TEXTURE_SRV, 2), p.groups()), ("GBufferA", swapped(rhi.BIND_TEXTURE_SRV, 2, TEX_SRV(2, r32)), p.groups()),
               ("blue noise", without(rhi.BIND_TEXTURE_SRV, 8), p.groups()), ("blue noise", swapped(rhi.BIND_TEXTURE_SRV, 8, TEX_SRV(8, noise64)), p.groups()),
               ("blue noise", swapped(rhi.BIND_TEXTURE_SRV, 8, TEX_SRV(8, r32)), p.groups()),
               ("shadow mask", without(rhi.BIND_TEXTURE_UAV, 0), p.groups()), ("shadow mask", swapped(rhi.BIND_TEXTURE_UAV, 0, TEX_UAV(0, r8uint, 0)), p.groups()),
               ("is 16x16", swapped(rhi.BIND_TEXTURE_UAV, 0, TEX_UAV(0, small8, 0)), p.groups()),
               ("linear view depth", without(rhi.BIND_TEXTURE_UAV, 1), p.groups()), ("linear view depth", swapped(rhi.BIND_TEXTURE_UAV, 1, TEX_UAV(1, lvd_mips, 0)), p.groups())]
        bad += [(what, without(rhi.BIND_STRUCTURED_SRV, slot), p.groups()) for slot, what in ((1, "TLAS nodes"), (3, "instances"), (4, "vertices"), (5, "materials"), (6, "indices"),
                                                                                         (7, "mesh data"), (9, "TLAS instances"), (10, "BLAS headers"), (11, "BLAS nodes"),
                                                                                         (12, "triangle order"))]
        for match, bindings, groups in bad:
            with pytest.raises(rhi.TrhipError, match=match):
                cl.dispatch(TRACE, bindings, groups)
        with pytest.raises(rhi.TrhipError, match="direct dispatch"):
            cl.dispatch_indirect(TRACE, good, args)
        rb, rp, rg = p.refit_bindings(), p.refit_push(), ((gs.numInstances + 63) // 64, 1, 1)
        too_many = rp.copy(); too_many["m_NumInstances"] = 1000
        too_many_nodes = rp.copy(); too_many_nodes["m_NumNodes"] = 1000
        for match, bindings, groups, push in (("12 bytes", rb[1:], rg, None), ("12 bytes", rb, rg, np.zeros(2, np.uint32)), ("needs SRVs", rb[:3] + rb[4:], rg, rp),
                                              ("needs SRVs", rb[:-1], rg, rp), ("exceed the instance buffer", rb, (16, 1, 1), too_many),
                                              ("exceed the TLAS node buffer", rb, rg, too_many_nodes), ("zero group count", rb, (0, 1, 1), rp)):
            with pytest.raises(rhi.TrhipError, match=match):
                cl.dispatch(REFIT, bindings, groups, push=push)
        with pytest.raises(rhi.TrhipError, match="direct dispatch"):
            cl.dispatch_indirect(REFIT, rb, args, push=rp)
        cl.close()
        dev.execute(cl); dev.wait_idle()
        assert not any(n.startswith(("shadowmask_", "raytracing_")) for n in dev.profile()), dev.profile()        # nothing was launched
        dev.profile_enable(False)
        depth, g = SS.images(W, H, 12)
        want, want_lvd, _ = SR.trace(sm, k, acc, depth, g, noise, SR.BRUTE)
        got, got_lvd = p.run(k, depth, g)
        same(got, want, "a good pass after the refusals: mask")
        same(got_lvd, want_lvd, "its linear view depth")
    finally:
        dev.profile_enable(False)
        cl.release(); args.release(); p.release(); gs.release()
        for t in (small8, r8uint, r32, noise64, lvd_mips):
            t.release()
