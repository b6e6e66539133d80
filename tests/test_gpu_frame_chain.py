"""The everything-on frame against tests/frame_chain_ref.py, the chain that runs on the CPU from the scene to the back buffer and takes
nothing from the device: three frames of FrameDriver, then of the C++ host mirror, on the chain's scene (an alpha-mask cut-out with a
BC3 texture over a BC1 / BC5 textured floor under open sky, a box that moves, a probe volume round it) with every option on, the
camera moving.  After each frame every download and every constant block equals the chain's, word for word, nothing excluded.
tests/test_frame_chain_ref.py shows that no pass of that frame is vacuous; profiles/frame/mutations.txt that a swapped binding or
matrix fails here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_chain_ref as FC  # noqa: E402
import sigma_ref as SG  # noqa: E402
from suite_support import compare_frame, dev, same  # noqa: E402, F401
from toyrenderer_amd import accel, gtao  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = FC.RENDER
F = np.float32


@pytest.fixture(scope="module")
def libraries(tmp_path_factory):
    return FC.Libraries(tmp_path_factory.mktemp("frame_chain"))


def _block(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.tobytes() == want.tobytes(), (what, got, want)


def _words(a, dtype=np.uint32):
    return np.ascontiguousarray(a).view(dtype)


def _compare_volume(got, want, what):
    same(got.irradiance, want.irradiance, what + ": irradiance")
    same(_words(got.distance, np.uint16), _words(want.distance, np.uint16), what + ": distance")
    same(_words(got.data, np.uint16), _words(want.data, np.uint16), what + ": probe data")


# ---- 1. FrameDriver -------------------------------------------------------------------------------------------------------------------------
def _gpu_scene(dev, sc):
    from toyrenderer_amd.frame import GpuScene
    gs = GpuScene(dev, sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
    gs.set_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
    gs.set_textures(sc["textures"])
    gs.set_materials(sc["materials"])
    gs.set_raytracing(sc["indices"], sc["index_counts"])
    return gs


def _prefill(drv):
    """The targets the frame does not clear and its passes do not write everywhere, filled with the references' sentinels."""
    drv.shadow_mask_texture.upload_mip(0, np.full((H, W), SG.SENTINEL8, np.uint8))
    drv.linear_view_depth.upload_mip(0, np.full((H, W), SG.SENTINEL16, np.uint16))
    drv.shadow_penumbra.upload_mip(0, np.full((H, W), SG.SENTINEL16, np.uint16))
    drv.shadow_history[1 - drv.shadow_history_written].upload_mip(0, np.full((H, W), SG.SENTINEL16, np.uint16))
    drv.shadow_tiles.upload_mip(0, np.full(accel.sigma_tiles(W, H)[::-1], SG.SENTINEL8, np.uint8))
    drv.normal_roughness.upload_mip(0, np.full((H, W), SG.SENTINEL32, np.uint32))


def _compare_driver(drv, want, what):
    same(drv.visibility.download_mip(0), want["vis"], what + ": visibility")
    same(_words(drv.motion.download_mip(0)).reshape(H, W), want["motion"], what + ": motion")
    same(drv.gbufferA.download_mip(0), want["gbuffer"], what + ": GBufferA")
    same(drv.hzb.download_chain(), want["hzb"], what + ": HZB")
    compare_frame(drv.results(), want["cull"])
    same(np.concatenate([drv.ao_depth.download_mip(m).ravel() for m in range(gtao.DEPTH_MIP_LEVELS)]), want["ao_chain"], what + ": AO working depth chain")
    same(drv.ao_edges.download_mip(0), want["ao_edges"], what + ": AO edges")
    same(drv.ao_working.download_mip(0), want["ao_working"], what + ": working AO term")
    same(drv.download_ssao(), want["ssao"], what + ": SSAO")
    same(drv.download_shadow_penumbra(), want["penumbra"], what + ": penumbra")
    same(drv.linear_view_depth.download_mip(0), want["linear_view_depth"], what + ": linear view depth")
    same(_words(drv.normal_roughness.download_mip(0)).reshape(H, W), want["normal_roughness"], what + ": normal and roughness")
    same(drv.download_shadow_tiles(), want["shadow_tiles"], what + ": shadow tiles")
    same(drv.download_shadow_history(), want["shadow_history"], what + ": shadow history")
    same(drv.download_shadow_mask(), want["shadow_mask"], what + ": shadow mask")
    same(_words(drv.download_ddgi_rays()), _words(want["ddgi_rays"]), what + ": DDGI rays")
    same(_words(drv.download_ddgi_fixed_rays()), _words(want["ddgi_fixed_rays"]), what + ": DDGI fixed rays")
    same(_words(drv.download_ddgi_variability()), _words(want["ddgi_variability"]), what + ": DDGI variability")
    _compare_volume(drv.download_ddgi(), want["volume"], what)
    same(drv.lighting_output.download_mip(0), want["lighting_output"], what + ": LightingOutput")
    for mip in range(FC.BLOOM_MIPS):
        same(drv.download_bloom(mip), want["bloom"][mip], what + f": bloom mip {mip}")
    same(drv.histogram.download(np.uint32, 256), want["histogram"], what + ": luminance histogram")
    same(_words(drv.luminance.download(np.float32, 1)), _words(np.array([want["luminance"]], F)), what + ": adapted luminance")
    same(_words(drv.exposure_texture.download_mip(0)).reshape(-1), _words(np.array([want["exposure"]], F)), what + ": exposure")
    same(drv.download_anti_aliased_output(), want["anti_aliased_output"], what + ": AntiAliasedLightingOutput")
    same(_words(drv.download_taa_history(), np.uint16), want["taa_history"], what + ": TAA history")
    same(drv.back_buffer.download_mip(0), want["back_buffer"], what + ": back buffer")
    same(_words(drv.depth.download_mip(0)), _words(want["depth_after_probes"]), what + ": depth")
    same(drv.probe_positions.download(np.uint32), _words(want["probe_positions"]).reshape(-1), what + ": probe positions")
    same(drv.probe_states.download(np.uint32), _words(want["probe_states"]), what + ": probe states")
    same(drv.probe_draw_args.download(np.uint32, 5), want["probe_draw_args"], what + ": probe draw arguments")
    count, culled, to_probe = drv.download_probes()
    assert count == int(want["probe_draw_args"][1]), (what, count)
    same(_words(culled), _words(want["probe_culled_positions"]), what + ": culled probe positions")
    same(to_probe, want["probe_instance_to_probe"], what + ": instance -> probe")
    same(drv.download_probe_winners(), want["probe_winners"], what + ": probe winner words")
    # every constant block the driver keeps
    seen = {name for name in dir(drv) if name.endswith("_consts") and not name.startswith("_") and not callable(getattr(drv, name))}
    assert seen == {"lighting_consts", "gtao_consts", "shadow_consts", "sigma_consts", "ddgi_update_consts", "sky_consts", "bloom_consts", "taa_consts", "post_consts",
                    "probe_cull_consts", "probe_draw_consts"}, seen
    for name in sorted(seen - {"post_consts"}):
        _block(getattr(drv, name), want[name], what + ": " + name)
    for got, block, name in zip(drv.post_consts, want["post_consts"], ("histogram", "adapt", "post")):
        _block(got, block, what + ": post_consts, " + name)
    _block(drv.taa_prev_world_to_clip, want["prev_world_to_clip"], what + ": m_PrevWorldToClip")
    _block(drv.taa_view.viewToClip, want["view"].viewToClip, what + ": the jittered projection")


def test_three_frames_through_the_driver(dev, oracle, libraries):
    """FrameDriver with FC.driver_settings() (the everything configuration), the view, the eye and the frame number of each frame
    set as the TAA and sigma frame tests set them, the box moved by an upload of the instance buffer in front of frame 1."""
    from toyrenderer_amd.frame import FrameDriver
    chain = FC.Chain(libraries, oracle)
    sc = chain.sc
    gs = _gpu_scene(dev, sc)
    view, eye = FC.view_at(0)
    drv = FrameDriver(dev, gs, view, camera_origin=eye, **FC.driver_settings())
    try:
        for f in range(FC.FRAMES):
            gs.instances.upload(FC.instances_at(sc, f))
            drv.view, drv.camera_origin = FC.view_at(f)
            drv.frame_counter = f
            _prefill(drv)
            dev.profile_reset(); dev.profile_enable(True)
            try:
                drv.record(); drv.run(); drv.results()
                names = set(dev.profile())
            finally:
                dev.profile_enable(False)
            _compare_driver(drv, chain.frame(f), f"frame {f}")
            assert "basepass_PS_Main_GBuffer#textured" in names, names
            assert any(n.startswith("basepass_MS_Main_visibility ALPHA_MASK_MODE=1#") for n in names), names
            assert {n.split("#")[1] for n in names if n.startswith("shadowmask_CS_ShadowMask")} == {"textured_penumbra"}, names
            assert drv.ddgi_updates == f + 1 and drv.ddgi_updates_skipped == 0
    finally:
        drv.release(); gs.release()


# ---- 2. the host mirror ---------------------------------------------------------------------------------------------------------------------
def _host_textures(r, sc):
    """The cut-out's texture through the DDS reader, the others as block bytes; the descriptor indices are the scene's."""
    import bc_blocks as B
    (cut, cut_format), rest = sc["textures"][0], sc["textures"][1:]
    assert cut_format == B.BC3
    got = [r.create_material_texture_dds(B.make_dds(cut.width, cut.height, list(cut), fourcc=b"DXT5"), False)]
    got += [r.create_material_texture(mips, fmt) for mips, fmt in rest]
    assert got == list(range(len(sc["textures"]))), got


def _compare_host(r, vol, want, what):
    same(r.download_visibility(), want["vis"], what + ": visibility")
    same(_words(r.download_motion()).reshape(H, W), want["motion"], what + ": motion")
    same(r.download_gbuffer_a(), want["gbuffer"], what + ": GBufferA")
    same(r.download_hzb(), want["hzb"], what + ": HZB")
    compare_frame(r.results(), want["cull"])
    same(r.download_ssao(), want["ssao"], what + ": SSAO")
    same(r.download_shadow_penumbra(), want["penumbra"], what + ": penumbra")
    same(r.download_shadow_tiles(), want["shadow_tiles"], what + ": shadow tiles")
    same(r.download_shadow_history(), want["shadow_history"], what + ": shadow history")
    same(r.download_shadow_mask(), want["shadow_mask"], what + ": shadow mask")
    same(_words(r.download_ddgi_variability(vol)), _words(want["ddgi_variability"]), what + ": DDGI variability")
    _compare_volume(r.download_ddgi_volume(vol), want["volume"], what)
    same(r.download_lighting_output(), want["lighting_output"], what + ": LightingOutput")
    for mip in range(FC.BLOOM_MIPS):
        same(r.download_bloom(mip), want["bloom"][mip], what + f": bloom mip {mip}")
    luminance, exposure = r.scene_luminance()
    same(_words(np.array([luminance, exposure], F)), _words(np.array([want["luminance"], want["exposure"]], F)), what + ": adapted luminance and exposure")
    same(r.download_anti_aliased_output(), want["anti_aliased_output"], what + ": AntiAliasedLightingOutput")
    same(_words(r.download_taa_history(), np.uint16), want["taa_history"], what + ": TAA history")
    same(r.download_back_buffer(), want["back_buffer"], what + ": back buffer")
    same(_words(r.download_depth()), _words(want["depth_after_probes"]), what + ": depth")
    culled, args, to_probe = r.gi_probe_results()
    same(args, want["probe_draw_args"], what + ": probe draw arguments")
    same(_words(culled), _words(want["probe_culled_positions"]), what + ": culled probe positions")
    same(to_probe, want["probe_instance_to_probe"], what + ": instance -> probe")
    _block(r.deferred_lighting_consts(), want["lighting_consts"], what + ": DeferredLightingConsts")
    _block(r.gtao_consts(), want["gtao_consts"], what + ": GTAOConstants")
    _block(r.shadow_mask_consts(), want["shadow_consts"], what + ": ShadowMaskConsts")
    _block(r.sigma_consts(), want["sigma_consts"], what + ": SigmaConsts")
    _block(r.sky_consts(), want["sky_consts"], what + ": SkyPassParameters")
    k, current, previous = r.taa_consts()
    _block(k, want["taa_consts"], what + ": TAAConsts")
    _block(np.concatenate([current, previous]), np.array([*want["jitter"][0], *want["jitter"][1]], F), what + ": the jitter offsets")
    _block(r.bloom_consts(2 * (FC.BLOOM_MIPS - 1)), want["bloom_consts"], what + ": BloomConsts")
    for got, block, name in zip(r.post_process_consts(), want["post_consts"], ("histogram", "adapt", "post")):
        _block(got, block, what + ": post-processing, " + name)
    _block(r.ddgi_update_consts(), want["ddgi_update_consts"], what + ": DDGIUpdateConsts")
    _block(r.ddgi_probe_visualization_consts(), want["probe_draw_consts"], what + ": GIProbeVisualizationConsts")


def test_three_frames_through_the_host_mirror(oracle, libraries):
    """The same three frames through host.Renderer with every trhost_set_* option on.  The mirror counts its frame before it records
    (frame f runs with m_FrameCounter f + 1: jitter, NoiseIndex, m_NoisePhase, m_FrameIndex), derives m_Eye from the matrix it is
    handed, moves the box through its node transforms and draws the probe rays' rotation from its own generator: the chain takes
    the rotation, and nothing else, from trhost_get_ddgi_update_consts."""
    from toyrenderer_amd import host
    r = host.Renderer(render=FC.RENDER, max_groups=FC.RECORD_CAPACITY)
    try:
        def consts_of(update):
            k = FC.ddgi_consts(update)
            k["rayRotation"] = r.ddgi_update_consts()["rayRotation"]
            return k
        chain = FC.Chain(libraries, oracle, consts_of=consts_of, frame_number=lambda f: f + 1, eye_of=FC.host_eye)
        sc, n = chain.sc, len(chain.sc["instances"])
        vol = FC.volume()
        r.load_scene(sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
        r.load_nodes(FC.nodes_at(sc, 0), np.arange(n, dtype=np.uint32))
        r.load_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
        _host_textures(r, sc)
        r.load_materials(sc["materials"])
        r.set_post_process(True)
        r.set_alpha_test(True)
        r.set_directional_light(*FC.LIGHT)
        r.set_ambient_occlusion(True)
        r.load_raytracing(sc["indices"], sc["index_counts"])
        r.upload_blue_noise(chain.noise)
        r.set_shadow_mask(True)
        r.set_shadow_denoising(True)
        r.upload_ddgi_volume(vol)
        r.set_ddgi(True)
        r.set_ddgi_update(True, seed=FC.UPDATE["seed"])
        r.set_ddgi_probe_placement(True, True, FC.UPDATE["min_frontface_distance"], 0.25)
        r.set_ddgi_probe_variability(True, FC.UPDATE["variability_threshold"])
        r.load_sky_dataset(FC.SK.dataset())
        r.set_sky(True, *FC.SKY)
        r.set_bloom(True, FC.BLOOM_MIPS, FC.BLOOM_RADIUS, FC.BLOOM_STRENGTH)
        r.set_auto_exposure(FC.AUTO_EXPOSURE[0], FC.AUTO_EXPOSURE[1], 0.0025)
        r.set_frame_time_ms(16.0)                                                         # 0.0025 per ms x 16 ms: FrameDriver's speed of one frame, 0.04
        r.set_taa(True)
        r.set_ddgi_probe_visualization(True, FC.PROBE_RADIUS, True)
        r.set_culling(FC.FLAGS)
        for f in range(FC.FRAMES):
            r.set_node_transforms(FC.nodes_at(sc, f))
            r.set_camera(FC.view_at(f)[0])
            r.frame(); r.results()
            chain.penumbra_init = r.download_shadow_penumbra()                            # the trace leaves the sky's texels as they were; the mirror's cannot be pre-filled
            want = chain.frame(f)
            got = r.instances(n)
            same(_words(got["m_WorldMatrix"]), _words(want["instances"]["m_WorldMatrix"]), f"host frame {f}: world matrices")
            same(_words(got["m_PrevWorldMatrix"]), _words(want["instances"]["m_PrevWorldMatrix"]), f"host frame {f}: previous world matrices")
            _compare_host(r, vol, want, f"host frame {f}")
            v = r.ddgi_variability()
            assert not v["converged"] and v["samples"] == f + 1 and v["skipped"] == 0, v
    finally:
        r.shutdown()
