"""Auto exposure and tone mapping on the GPU ("adaptluminance_CS_GenerateLuminanceHistogram", "adaptluminance_CS_AdaptExposure",
"postprocess_PS_PostProcess", csrc/k_postprocess.hip), every word against tests/postprocess_ref.c: uploaded inputs at sizes with
partial vectors, trips, tiles and waves; constructed histograms; full frames through FrameDriver(post=True) over five frames with
the luminance carried along; and misuse.  Outputs are pre-filled so that a skipped texel or an overwritten count shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gbuffer_ref as GR  # noqa: E402
import lighting_ref as LR  # noqa: E402
import lighting_scenes as LS  # noqa: E402
import postprocess_ref as PR  # noqa: E402
from suite_support import bits, compare_frame, dev, frame_reference, gpu_scene, gr, halves_to_words, host_renderer, kernel_constant, lit_cornell, lr, op_counts, post_chain_reference, pr, recorded_kinds, same, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from gbuffer_scenes import with_normals_and_materials  # noqa: E402
from toyrenderer_amd import gltf_lite, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import city  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENTINEL = 0x12345678
HIST_INIT = (np.arange(256, dtype=np.uint32) * np.uint32(7) + np.uint32(3))


# ---- 1. the histogram ---------------------------------------------------------------------------------------------------------
def _two_trip_size(dev):
    """The smallest image at which every workgroup of the histogram kernel takes at least two trips and the last trip is partial.
    The kernel runs min(ceil(vectors / kBlock), kHistGroupsPerCU * CUs) workgroups of kBlock lanes; lane t of workgroup b takes the
    16-byte vectors b * kBlock + t + j * grid * kBlock.  With the grid at its cap G, workgroup G - 1 starts its second trip at
    vector G * kBlock + (G - 1) * kBlock, so vectors = (2 G - 1) * kBlock + 1 is the smallest count at which its lane 0 (and so a
    lane of every workgroup) takes two trips; that trip has one lane of kBlock, the most partial it can be.  Three more texels
    make W * H mod 4 = 3, so the tail path runs as well.  The count is laid out as 5 rows when it divides, else one row."""
    block, per_cu, per_lane = kernel_constant("k_postprocess.hip", "kBlock"), kernel_constant("k_postprocess.hip", "kHistGroupsPerCU"), kernel_constant("k_postprocess.hip", "kHistTexelsPerLane")
    grid = per_cu * dev.compute_units
    texels = ((2 * grid - 1) * block + 1) * per_lane + (per_lane - 1)
    return (texels // 5, 5) if texels % 5 == 0 else (texels, 1)


def _histogram_contents(pr, n, seed):
    """name -> n words: seeded over the whole format; one value (the worst LDS contention: a lost add shows); black; luminances
    on both sides of 0.005; values above max_luminance; the NaN and infinity patterns among ordinary texels."""
    seeded = PR.seeded_words(n, seed)
    tile = lambda w: np.resize(np.asarray(w, np.uint32), n)                                            # noqa: E731
    above = np.array([PR.grey(c) for c in range(19 << 6, 31 << 6, 5)], np.uint32)                      # 16 and up: above 12.0
    mixed = seeded.copy()
    mixed[:min(n, len(PR.SPECIAL_WORDS))] = PR.SPECIAL_WORDS[:n]
    return {"seeded": seeded, "one value": tile([PR.grey(14 << 6)]), "black": np.zeros(n, np.uint32), "straddling 0.005": tile(PR.straddling_words(pr)),
            "above the maximum": tile(above), "NaN and infinity": mixed}


HIST_SIZES = [(1, 1), (16, 16), (17, 17), (67, 35), (129, 3), (640, 360), "two trips"]


@pytest.mark.parametrize("size", HIST_SIZES, ids=str)
def test_histogram_matches_the_reference(dev, pr, size):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import PUSH, TEX_SRV, UAV
    W, H = _two_trip_size(dev) if size == "two trips" else size
    if size == "two trips":
        print(f"two-trip size with {dev.compute_units} CUs: {W}x{H} = {W * H} texels, W*H mod 4 = {W * H % 4}")
    assert {(67, 35): 1, (129, 3): 3}.get((W, H), W * H % 4) == W * H % 4
    tex = dev.create_texture(W, H, 1, rhi.FORMAT_R11G11B10_FLOAT, "Lighting Output")
    hist = dev.create_buffer(1024, "Luminance Histogram")
    cl = dev.create_command_list()
    k = PR.histogram_params((W, H))
    try:
        for name, words in _histogram_contents(pr, W * H, 50 + W).items():
            tex.upload_mip(0, words.reshape(H, W))
            hist.upload(HIST_INIT)
            cl.open()
            cl.dispatch("adaptluminance_CS_GenerateLuminanceHistogram", [PUSH(0), TEX_SRV(0, tex), UAV(0, hist)], ((W + 15) // 16, (H + 15) // 16, 1), push=k)
            cl.close()
            dev.execute(cl); dev.wait_idle()
            got = hist.download(np.uint32, 256)
            same(got, PR.histogram(pr, words, k, HIST_INIT), f"{W}x{H} {name}")
            assert int((got - HIST_INIT).astype(np.uint64).sum()) == W * H, "the kernel adds to u0, and the counts sum to W * H"
            if name == "one value":
                assert np.count_nonzero(got != HIST_INIT) == 1
            if name == "black":
                assert got[0] - HIST_INIT[0] == W * H
            if name == "above the maximum":
                assert got[255] - HIST_INIT[255] == W * H
    finally:
        cl.release(); hist.release(); tex.release()


# ---- 2. CS_AdaptExposure ------------------------------------------------------------------------------------------------------
def test_adapt_exposure_matches_the_reference(dev, pr):
    """The constructed histograms of the CPU tests, uploaded; speeds 0, 0.04 and 1; three starting luminances; then 20 steps of
    the recurrence on the GPU's own state.  The luminance buffer and the exposure texel are compared bit for bit."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import PUSH, SRV, TEX_UAV, UAV
    hist = dev.create_buffer(1024, "Luminance Histogram")
    lum = dev.create_buffer(4, "Exposure Buffer")
    exposure = dev.create_texture(1, 1, 1, rhi.FORMAT_R32_FLOAT, "Exposure Texture")
    cl = dev.create_command_list()

    def step(k):
        cl.open()
        cl.dispatch("adaptluminance_CS_AdaptExposure", [PUSH(0), SRV(0, hist), UAV(0, lum), TEX_UAV(1, exposure, 0)], (1, 1, 1), push=k)
        cl.close()
        dev.execute(cl); dev.wait_idle()
        return lum.download(F, 1)[0], exposure.download_mip(0)[0, 0]
    try:
        for name, (h, n) in PR.ADAPT_HISTOGRAMS.items():
            hist.upload(h)
            for speed in (0.0, 0.04, 1.0):
                k = PR.adapt_params(n, speed)
                for last in (1.0, 0.004, 12.0):
                    lum.upload(np.array([last], F))
                    exposure.upload_mip(0, np.array([[-1.0]], F))
                    got = step(k)
                    want = PR.adapt_exposure(pr, k, h, last)
                    assert bits(got).tolist() == bits(want).tolist(), (name, speed, last, got, want)
        h, n = PR.ADAPT_HISTOGRAMS["mid bins"]
        hist.upload(h)
        k = PR.adapt_params(n, 0.04)
        lum.upload(np.array([1.0], F))
        want_lum = F(1.0)
        for i in range(20):
            got = step(k)
            want_lum, want_exp = PR.adapt_exposure(pr, k, h, want_lum)
            assert bits(got).tolist() == bits((want_lum, want_exp)).tolist(), i
        assert want_lum != F(1.0)
    finally:
        cl.release(); hist.release(); lum.release(); exposure.release()


# ---- 3. PS_PostProcess --------------------------------------------------------------------------------------------------------
def _post_image(W, H, seed, ramp=False):
    """Colour words [H, W]: seeded over the whole format with the special patterns among the first texels; or the grey ramp over
    every 11-bit code (ramp: 2048 codes along the rows of a 256-wide image, then seeded finite words)."""
    if ramp:
        w = PR.seeded_finite_words(W * H, seed)
        w[:2048] = [PR.grey(c) for c in range(2048)]
        return w.reshape(H, W)
    w = np.where(np.random.default_rng(seed).random(W * H) < 0.5, PR.seeded_words(W * H, seed), PR.seeded_finite_words(W * H, seed + 1))
    k = min(len(PR.SPECIAL_WORDS), max(W * H - 1, 0))
    w[1:1 + k] = PR.SPECIAL_WORDS[:k]
    return w.reshape(H, W).astype(np.uint32)


POST_SIZES = list(LS.SIZES) + [(256, 256)]


@pytest.mark.parametrize("size", POST_SIZES, ids=str)
def test_post_process_matches_the_reference(dev, pr, size):
    """The lighting test's sizes (partial tiles and waves on both axes) and a 256 x 256 grey ramp; bloom bound and unbound at
    strengths 0, 0.1 and 1; manual exposures and the luminance buffer; constants through push constants and through b0.  u0 is
    pre-filled with a sentinel: every texel is overwritten, alpha 255."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, PUSH, SAMPLER, SRV, TEX_SRV, TEX_UAV
    W, H = size
    colour, bloom = _post_image(W, H, 60 + W, ramp=size == (256, 256)), _post_image(W, H, 61 + W)
    t_colour = dev.create_texture(W, H, 1, rhi.FORMAT_R11G11B10_FLOAT, "Lighting Output")
    t_bloom = dev.create_texture(W, H, 1, rhi.FORMAT_R11G11B10_FLOAT, "Bloom")
    t_out = dev.create_texture(W, H, 1, rhi.FORMAT_RGBA8_UNORM, "Back Buffer")
    lum = dev.create_buffer(4, "Exposure Buffer")
    cl = dev.create_command_list()
    t_colour.upload_mip(0, colour); t_bloom.upload_mip(0, bloom)
    groups = ((W + 7) // 8, (H + 7) // 8, 1)
    cases = [(manual, 1.0, None, 0.0) for manual in (0.05, 1.0, 20.0)] + [(0.0, l, None, 0.0) for l in (0.004, 1.0, 12.0, 0.0)]
    cases += [(1.0, 1.0, bloom, s) for s in (0.0, 0.1, 1.0)] + [(0.0, 0.37, bloom, 0.1), (0.0, 0.37, None, 0.5)]
    try:
        for i, (manual, luminance, b, strength) in enumerate(cases):
            k = PR.post_params((W, H), manual=manual, bloom_strength=strength)
            t_out.upload_mip(0, np.full((H, W), SENTINEL, np.uint32))
            lum.upload(np.array([luminance], F))
            cl.open()
            bind = [TEX_SRV(0, t_colour), TEX_UAV(0, t_out, 0), SAMPLER(0)] + ([TEX_SRV(2, t_bloom)] if b is not None else [])
            bind += [SRV(1, lum)] if manual == 0.0 or i % 2 else []
            if i % 2:
                cl.dispatch("postprocess_PS_PostProcess", bind + [CB(0, cl.constant_buffer(k, "PostProcessParameters"))], groups)
            else:
                cl.dispatch("postprocess_PS_PostProcess", bind + [PUSH(0)], groups, push=k)
            cl.close()
            dev.execute(cl); dev.wait_idle()
            got = t_out.download_mip(0)
            what = f"{W}x{H} manual {manual} luminance {luminance} bloom {'bound' if b is not None else 'unbound'} strength {strength}"
            same(got, PR.post(pr, k, colour, bloom=b, luminance_in=luminance), what)
            assert np.all(got >> 24 == 255) and not np.any(got == SENTINEL), what
            if luminance == 0.0 and manual == 0.0:
                assert np.all(got == 0xFF000000), "a zero luminance stores black"
        if size == (256, 256):
            assert len(np.unique(got)) > 1000
    finally:
        cl.release(); lum.release(); t_colour.release(); t_bloom.release(); t_out.release()


# ---- 4. full frames -----------------------------------------------------------------------------------------------------------
def _check_post_frames(dev, pr, post, lighting_output, what, frames=5, bloom=None):
    """`frames` frames of a post=True driver against the reference chain, the luminance carried from frame to frame."""
    luminance = F(1.0)
    seen = []
    for f in range(frames):
        post.record(); post.run(); post.results()
        back, hist, luminance, exposure = post_chain_reference(pr, post, lighting_output, luminance, bloom)
        same(post.lighting_output.download_mip(0), lighting_output, f"{what} frame {f}: LightingOutput")
        same(post.back_buffer.download_mip(0), back, f"{what} frame {f}: back buffer")
        assert bits(post.luminance.download(F, 1)).tolist() == bits(luminance).tolist(), (what, f)
        if hist is not None:
            same(post.histogram.download(np.uint32, 256), hist, f"{what} frame {f}: histogram")
            assert bits(post.exposure_texture.download_mip(0)).tolist() == bits(exposure).tolist(), (what, f)
            assert int(hist.sum()) == lighting_output.size
        seen.append(float(luminance))
    return seen


@pytest.mark.parametrize("flags", [0, 7])
def test_frames_match_the_reference(dev, oracle, vr, gr, lr, pr, tmp_path, flags):
    """FrameDriver(post=True) on the generated city, debug modes 0 and 4, next to a lighting=True driver, five frames each: back
    buffer, histogram, luminance and exposure equal gr_gbuffer -> lighting reference -> post reference; depth, HZB, cull outputs,
    GBufferA, motion, LightingOutput and pipeline statistics equal the lighting=True run word for word."""
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    v, sc, mats = with_normals_and_materials(s, sc)
    gs = gpu_scene(dev, s, sc["instances"], v, mats)
    cam = s.cameras[0]
    render = (640, 360)
    eye = (0.4, 0.1, -0.3)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view(eye, cam.orientation)
    view = synth.View(V, synth.world_to_view((0.0, 0.0, 0.0), cam.orientation), P, float(np.float32(cam.znear)), *render)
    geo_v = (v, s.meshletVertexIds, s.meshletTriangles)
    light = (LS.LIGHTS[1][1], 2.5)
    drivers, queries = [], []
    try:
        for mode in (0, 4):
            kw = dict(record_capacity=4096, culling_flags=flags, debug_mode=mode, dir_light=light, camera_origin=eye)
            lit = FrameDriver(dev, gs, view, lighting=True, **kw)
            post = FrameDriver(dev, gs, view, post=True, **kw)
            ql, qp = dev.create_pipeline_stats(), dev.create_pipeline_stats()
            drivers += [lit, post]; queries += [ql, qp]
            for d, q in ((lit, ql), (post, qp)):
                d.record(q); d.run()
            got_lit, got = lit.results(), post.results()
            what = f"flags {flags} debug mode {mode}"
            assert post.lighting_consts.tobytes() == lit.lighting_consts.tobytes()
            ref, vis, depth, g, m, out = frame_reference(oracle, vr, gr, lr, sc, geo_v, view, mats, flags, mode, post.lighting_consts)
            compare_frame(got, ref); compare_frame(got_lit, ref)
            for name in ("gbufferA", "visibility", "lighting_output"):
                same(getattr(post, name).download_mip(0), getattr(lit, name).download_mip(0), what + ": " + name)
            same(post.motion.download_mip(0).view(np.uint16), lit.motion.download_mip(0).view(np.uint16), what + ": motion")
            same(post.depth.download_mip(0).view(np.uint32), lit.depth.download_mip(0).view(np.uint32), what + ": depth")
            same(post.hzb.download_chain(), lit.hzb.download_chain(), what + ": HZB")
            if flags & 2:
                assert got["lateCount"] == got_lit["lateCount"] and np.array_equal(got["lateArgs"], got_lit["lateArgs"])
            assert qp.get() == ql.get(), what + ": pipeline statistics"
            post.reset_exposure()                                                          # the first frame above moved it
            seen = _check_post_frames(dev, pr, post, out, what)
            steps = np.diff([1.0] + seen)
            assert np.all(steps < 0) or np.all(steps > 0), seen                            # it adapts, monotonically
            back = post.back_buffer.download_mip(0)
            cov = depth > 0
            assert cov.sum() > 0.2 * cov.size and np.all(back[~cov] == 0xFF000000) and len(np.unique(back[cov])) > {0: 50, 4: 8}[mode]   # view 4 shows the materials' few albedos
    finally:
        for q in queries:
            q.release()
        for d in drivers:
            d.release()
        gs.release()


def test_post_adds_one_clear_and_three_dispatches(dev, oracle, pr, tmp_path):
    """The op names and launch counts of a lighting=True driver are those of the parent commit; post=True adds exactly one buffer
    clear and three dispatches, and with a manual exposure one buffer write and one dispatch.  The manual frame's back buffer and
    luminance equal the reference's; exposure and bloom parameters reach the constants."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver
    s, sc = city(tmp_path, oracle)
    v, sc, mats = with_normals_and_materials(s, sc)
    gs = gpu_scene(dev, s, sc["instances"], v, mats)
    view = gltf_lite.view_of(s.cameras[0], (320, 180))
    bloom_words = _post_image(320, 180, 77)
    t_bloom = dev.create_texture(320, 180, 1, rhi.FORMAT_R11G11B10_FLOAT, "Bloom")
    t_bloom.upload_mip(0, bloom_words)
    out, kinds = {}, {}
    try:
        for name, kw in (("lighting", dict(lighting=True)), ("post", dict(post=True)), ("manual", dict(post=True, exposure=(2.5, 0.25), bloom=(t_bloom, 0.2)))):
            drv = FrameDriver(dev, gs, view, record_capacity=4096, **kw)
            try:
                out[name] = op_counts(dev, drv)
                kinds[name] = recorded_kinds(drv)
                if name == "manual":
                    hk, ak, pk = drv.post_consts
                    assert hk is None and ak is None and pk.tobytes() == PR.post_params((320, 180), manual=2.5, middle_gray=0.25, bloom_strength=0.2).tobytes()
                    _check_post_frames(dev, pr, drv, drv.lighting_output.download_mip(0), "manual exposure", frames=2, bloom=bloom_words)
                    assert drv.luminance.download(F, 1)[0] == F(2.5)
                if name == "post":
                    hk, ak, pk = drv.post_consts
                    assert hk.tobytes() == PR.histogram_params((320, 180)).tobytes() and ak.tobytes() == PR.adapt_params(320 * 180, 0.04).tobytes()
                    assert pk.tobytes() == PR.post_params((320, 180)).tobytes()
            finally:
                drv.release()
    finally:
        t_bloom.release(); gs.release()
    cull = {f"{n} LATE_CULL={late}#{k}": 2 for late in (0, 1) for n, ks in (("gpuculling_CS_GPUCulling", ("instance_cache", "fused")), ("basepass_AS_Main", ("cull", "compact")))
            for k in ks}
    hzb = {"ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1#depth_tile": 2, "ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1#tail": 2}
    parent = {**cull, **hzb, "basepass_MS_Main_visibility#main": 4, "basepass_MS_Main_visibility#tiles": 4, "basepass_PS_Main_GBuffer#main": 1,
              "deferredlighting_PS_Main#main": 1}
    assert out["lighting"] == parent                                                  # what tests/test_gpu_lighting.py pins for the parent
    assert out["post"] == {**parent, "adaptluminance_CS_GenerateLuminanceHistogram#main": 1, "adaptluminance_CS_AdaptExposure#main": 1, "postprocess_PS_PostProcess#main": 1}
    assert out["manual"] == {**parent, "postprocess_PS_PostProcess#main": 1}
    added = lambda a: {k: n - kinds["lighting"].get(k, 0) for k, n in kinds[a].items() if n != kinds["lighting"].get(k, 0)}   # noqa: E731
    assert added("post") == {"clear_buffer_u32": 1, "dispatch": 3}, added("post")
    assert added("manual") == {"write_buffer": 1, "dispatch": 1}, added("manual")


def test_cornell_through_the_driver(dev, oracle, vr, gr, lr, pr):
    """The cornell fixture with tests/golden/cornell_materials.json through FrameDriver(post=True), five frames: the reference
    chain's words; the lit red wall is red in the back buffer and the green wall green."""
    from toyrenderer_amd.frame import FrameDriver
    s, inst, _, mats, camera = lit_cornell(oracle)
    sc = dict(s.as_oracle()); sc["instances"] = inst
    render = (320, 180)
    view = gltf_lite.view_of(camera, render)
    eye = tuple(float(x) for x in camera.position)
    gs = gpu_scene(dev, s, inst, s.vertices, mats)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, post=True, dir_light=((0.3, -0.8, -0.52), 3.0), camera_origin=eye,
                      auto_exposure=(0.004, 12.0, 0.5))
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    try:
        drv.record()
        _, _, depth, g, _, out = frame_reference(oracle, vr, gr, lr, sc, geo_v, view, mats, 7, 0, drv.lighting_consts)
        _check_post_frames(dev, pr, drv, out, "cornell")
        back = drv.back_buffer.download_mip(0)
        albedo = GR.albedo_bytes(g[..., 0]).astype(np.int64)
        r8, g8 = (back & 0xFF).astype(np.int64), ((back >> 8) & 0xFF).astype(np.int64)
        lit = (depth > 0) & (np.maximum(r8, g8) >= 32)
        red, green = lit & (albedo[..., 0] > albedo[..., 1] + 60), lit & (albedo[..., 1] > albedo[..., 0] + 60)
        assert red.sum() + green.sum() > 500 and np.all(r8[red] > g8[red]) and np.all(g8[green] > r8[green])
    finally:
        drv.release(); gs.release()


# ---- 5. the host mirror -------------------------------------------------------------------------------------------------------
def test_host_path_over_five_frames(oracle, vr, gr, lr, pr, tmp_path):
    """The C++ host mirror (trhost_set_post_process): five frames with a moving camera and a changing light, a bloom upload in
    frame 1, a manual exposure switched on in frame 3 and off again in frame 4.  The back buffer equals gr_gbuffer -> lighting
    reference -> post reference fed the structs of trhost_get_post_process_consts, the luminance carried from frame to frame;
    trhost_get_scene_luminance is compared bit for bit; trhost_reset_exposure returns the state to 1.0; misuse at the facade."""
    from toyrenderer_amd import host
    from visibility_scenes import consts
    s, sc0 = city(tmp_path, oracle)
    v, sc0, mats = with_normals_and_materials(s, sc0)
    cam = s.cameras[0]
    render = (640, 360)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    hzb = oracle.HzbTexture(*I.hzb_dims(*render))
    depth0 = np.zeros((render[1], render[0]), np.float32)
    geo_v = (v, s.meshletVertexIds, s.meshletTriangles)
    inst_in = s.instances.copy()
    inst_in["m_MaterialDataIdx"] = sc0["instances"]["m_MaterialDataIdx"]
    bloom = PR.seeded_finite_words(render[0] * render[1], 91).reshape(render[1], render[0])
    with host_renderer(s, inst_in, geo_v, render=render, max_groups=4096) as r:
        with pytest.raises(host.HostError, match="trhost_load_materials"):
            r.set_post_process(True)
        for call in (r.download_back_buffer, r.post_process_consts, r.scene_luminance):
            with pytest.raises(host.HostError, match="post-processing"):
                call()
        r.load_materials(mats)
        r.set_debug_view_mode(10)
        with pytest.raises(host.HostError, match="Ambient"):
            r.set_post_process(True)
        r.set_debug_view_mode(0)
        r.set_post_process(True)
        r.set_auto_exposure(0.004, 12.0, 0.0025)
        r.set_frame_time_ms(16.0)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        prevV = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
        luminance = F(1.0)
        for f in range(5):
            eye = (0.1 * f, 0.02 * f, -0.15 * f)
            V = synth.world_to_view(eye, cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            prevV = V
            manual = 1.75 if f == 3 else 0.0
            r.set_camera(view)
            r.set_directional_light((0.2 * f - 0.4, -1.0, 0.3), 1.0 + f)
            r.set_exposure(manual, 0.18 + 0.01 * f)
            if f == 1:
                r.upload_bloom(bloom, 0.25)
            if f == 4:
                r.upload_bloom(None)
            r.frame()
            r.results()
            sc = dict(s.as_oracle()); sc["instances"] = r.instances(len(s.instances))
            ref = oracle.frame(sc, view.as_dict(), hzb, depth0, cullingFlags=7, record_capacity=4096, maxGroups=4096, raster=(I.world_to_clip(V, P), *geo_v))
            kb = consts(view)
            geo = VR.Geometry(sc, *geo_v)
            vis_ref, depth = VR.frame_visibility(vr, kb, geo, ref, *render)
            g_ref, m_ref = GR.frame_gbuffer(gr, kb, geo, ref, vis_ref, mats, 0)
            lit = LR.lighting(lr, r.deferred_lighting_consts(), g_ref, depth, motion=halves_to_words(VR.to_half_bits(m_ref)))
            same(r.download_lighting_output(), lit, f"frame {f}: LightingOutput")
            hk, ak, pk = r.post_process_consts()
            want_bloom = bloom if 1 <= f < 4 else None
            assert pk.tobytes() == PR.post_params(render, manual=manual, middle_gray=0.18 + 0.01 * f, bloom_strength=0.25 if want_bloom is not None else 0.0).tobytes()
            if manual > 0:
                assert hk is None and ak is None
                luminance, exposure = F(manual), None
            else:
                assert hk.tobytes() == PR.histogram_params(render).tobytes()
                assert ak.tobytes() == PR.adapt_params(render[0] * render[1], F(0.0025) * F(16.0), middle_gray=0.18 + 0.01 * f).tobytes()
                luminance, exposure = PR.adapt_exposure(pr, ak, PR.histogram(pr, lit, hk), luminance)
            same(r.download_back_buffer(), PR.post(pr, pk, lit, bloom=want_bloom, luminance_in=luminance), f"frame {f}: back buffer")
            got_lum, got_exp = r.scene_luminance()
            assert bits(got_lum).tolist() == bits(luminance).tolist(), f
            if exposure is not None:
                assert bits(got_exp).tolist() == bits(exposure).tolist(), f
        assert luminance != F(1.0)
        r.reset_exposure()
        assert bits(r.scene_luminance()).tolist() == bits((1.0, 1.0)).tolist()


# ---- 6. misuse ----------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused(dev, oracle, tmp_path):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    from toyrenderer_amd.rhi import PUSH, SRV, TEX_SRV, TEX_UAV, UAV
    W, H = 64, 32
    mk = lambda w, h, fmt, name: dev.create_texture(w, h, 1, fmt, name)                                 # noqa: E731
    colour, bloom, back = mk(W, H, rhi.FORMAT_R11G11B10_FLOAT, "colour"), mk(W, H, rhi.FORMAT_R11G11B10_FLOAT, "bloom"), mk(W, H, rhi.FORMAT_RGBA8_UNORM, "back")
    back2 = mk(W, H, rhi.FORMAT_RGBA8_UNORM, "back 2")
    small, small_back, r32 = mk(W // 2, H, rhi.FORMAT_R11G11B10_FLOAT, "small"), mk(W // 2, H, rhi.FORMAT_RGBA8_UNORM, "small back"), mk(W, H, rhi.FORMAT_R32_FLOAT, "R32")
    exposure, exposure2 = mk(1, 1, rhi.FORMAT_R32_FLOAT, "exposure"), mk(2, 1, rhi.FORMAT_R32_FLOAT, "2x1 exposure")
    hist, short, lum = dev.create_buffer(1024, "histogram"), dev.create_buffer(1020, "short histogram"), dev.create_buffer(4, "luminance")
    args = dev.create_buffer(12, "args", stride=12, indirect=True)
    args.upload(np.array([8, 4, 1], np.uint32))
    cl = dev.create_command_list()
    everything = [colour, bloom, back, back2, small, small_back, r32, exposure, exposure2, hist, short, lum, args]
    try:
        cl.open()
        # the histogram
        name, g16 = "adaptluminance_CS_GenerateLuminanceHistogram", ((W + 15) // 16, (H + 15) // 16, 1)
        hk = PR.histogram_params((W, H))
        t0, u0 = TEX_SRV(0, colour), UAV(0, hist)
        cases = [("push missing", [t0, u0], g16, None, "push constants"), ("push too short", [PUSH(0), t0, u0], g16, hk.view(np.uint32)[:3], "push constants"),
                 ("t0 missing", [PUSH(0), u0], g16, hk, "t0"), ("t0 wrong format", [PUSH(0), TEX_SRV(0, r32), u0], g16, hk, "R11G11B10_FLOAT"),
                 ("t0 wrong size", [PUSH(0), TEX_SRV(0, small), u0], g16, hk, "m_SrcColorDims"), ("dims differ", [PUSH(0), t0, u0], g16, PR.histogram_params((W // 2, H)), "m_SrcColorDims"),
                 ("u0 missing", [PUSH(0), t0], g16, hk, "u0"), ("u0 short", [PUSH(0), t0, UAV(0, short)], g16, hk, "256 uint32"),
                 ("grid too small", [PUSH(0), t0, u0], (g16[0] - 1, g16[1], 1), hk, "covering"), ("grid too small in y", [PUSH(0), t0, u0], (g16[0], g16[1] - 1, 1), hk, "covering"),
                 ("empty", [PUSH(0), t0, u0], g16, PR.histogram_params((0, H)), "empty")]
        for what, b, grp, push, text in cases:
            with pytest.raises(rhi.TrhipError, match=text) as e:
                cl.dispatch(name, b, grp, push=push)
            assert name in str(e.value), (what, str(e.value))
        with pytest.raises(rhi.TrhipError, match="direct dispatch") as e:
            cl.dispatch_indirect(name, [PUSH(0), t0, u0], args, push=hk)
        assert name in str(e.value)
        cl.dispatch(name, [PUSH(0), t0, u0], g16, push=hk)
        # the adapt pass
        name = "adaptluminance_CS_AdaptExposure"
        ak = PR.adapt_params(W * H, 0.04)
        t0, u0, u1 = SRV(0, hist), UAV(0, lum), TEX_UAV(1, exposure, 0)
        cases = [("push missing", [t0, u0, u1], (1, 1, 1), None, "push constants"), ("push too short", [PUSH(0), t0, u0, u1], (1, 1, 1), ak.view(np.uint32)[:4], "push constants"),
                 ("t0 missing", [PUSH(0), u0, u1], (1, 1, 1), ak, "t0"), ("t0 short", [PUSH(0), SRV(0, short), u0, u1], (1, 1, 1), ak, "256 uint32"),
                 ("u0 missing", [PUSH(0), t0, u1], (1, 1, 1), ak, "u0"), ("u1 missing", [PUSH(0), t0, u0], (1, 1, 1), ak, "u1"),
                 ("u1 wrong format", [PUSH(0), t0, u0, TEX_UAV(1, back, 0)], (1, 1, 1), ak, "R32_FLOAT"), ("u1 wrong size", [PUSH(0), t0, u0, TEX_UAV(1, exposure2, 0)], (1, 1, 1), ak, "1x1"),
                 ("two groups", [PUSH(0), t0, u0, u1], (2, 1, 1), ak, r"\(1, 1, 1\)")]
        for what, b, grp, push, text in cases:
            with pytest.raises(rhi.TrhipError, match=text) as e:
                cl.dispatch(name, b, grp, push=push)
            assert name in str(e.value), (what, str(e.value))
        with pytest.raises(rhi.TrhipError, match=r"\(1, 1, 1\)") as e:
            cl.dispatch_indirect(name, [PUSH(0), t0, u0, u1], args, push=ak)
        assert name in str(e.value)
        cl.dispatch(name, [PUSH(0), t0, u0, u1], (1, 1, 1), push=ak)
        # the post pass
        name, g8 = "postprocess_PS_PostProcess", ((W + 7) // 8, (H + 7) // 8, 1)
        pk, pm = PR.post_params((W, H)), PR.post_params((W, H), manual=1.5)
        t0, t1, t2, u0 = TEX_SRV(0, colour), SRV(1, lum), TEX_SRV(2, bloom), TEX_UAV(0, back, 0)
        cases = [("constants missing", [t0, t1, u0], g8, None, "PostProcessParameters"), ("t0 missing", [PUSH(0), t1, u0], g8, pk, "t0"),
                 ("t0 wrong format", [PUSH(0), TEX_SRV(0, r32), t1, u0], g8, pk, "R11G11B10_FLOAT"), ("t0 wrong size", [PUSH(0), TEX_SRV(0, small), t1, u0], g8, pk, "m_OutputDims"),
                 ("t1 missing with manual 0", [PUSH(0), t0, u0], g8, pk, "t1"), ("t2 wrong format", [PUSH(0), t0, t1, TEX_SRV(2, back2), u0], g8, pk, "bloom"),
                 ("t2 wrong size", [PUSH(0), t0, t1, TEX_SRV(2, small), u0], g8, pk, "m_OutputDims"), ("u0 missing", [PUSH(0), t0, t1], g8, pk, "u0"),
                 ("u0 wrong format", [PUSH(0), t0, t1, TEX_UAV(0, bloom, 0)], g8, pk, "RGBA8_UNORM"), ("u0 wrong size", [PUSH(0), t0, t1, TEX_UAV(0, small_back, 0)], g8, pk, "m_OutputDims"),
                 ("dims differ", [PUSH(0), t0, t1, u0], g8, PR.post_params((W // 2, H)), "m_OutputDims"), ("empty", [PUSH(0), t0, t1, u0], g8, PR.post_params((W, 0)), "empty"),
                 ("grid too small", [PUSH(0), t0, t1, u0], (g8[0] - 1, g8[1], 1), pk, "covering"), ("grid too small in y", [PUSH(0), t0, t1, u0], (g8[0], g8[1] - 1, 1), pk, "covering")]
        for what, b, grp, push, text in cases:
            with pytest.raises(rhi.TrhipError, match=text) as e:
                cl.dispatch(name, b, grp, push=push)
            assert name in str(e.value), (what, str(e.value))
        with pytest.raises(rhi.TrhipError, match="direct dispatch") as e:
            cl.dispatch_indirect(name, [PUSH(0), t0, t1, u0], args, push=pk)
        assert name in str(e.value)
        cl.dispatch(name, [PUSH(0), t0, u0], g8, push=pm)                                  # a manual exposure needs no t1
        cl.dispatch(name, [PUSH(0), t0, t1, t2, u0], g8, push=pk)
        # the new format: no clear, by name; copies between equal descriptions
        for clear in (lambda: cl.clear_texture_f32(back, 0.5), lambda: cl.clear_texture_u32(back, 1)):
            with pytest.raises(rhi.TrhipError, match="RGBA8_UNORM"):
                clear()
        cl.copy_texture(back2, back)
        with pytest.raises(rhi.TrhipError, match="differ"):
            cl.copy_texture(small_back, back)
        with pytest.raises(rhi.TrhipError, match="differ"):
            cl.copy_texture(bloom, back)
        cl.close()
        back.upload_mip(0, np.arange(W * H, dtype=np.uint32).reshape(H, W))                # upload, copy and download keep the words
        colour.upload_mip(0, np.zeros((H, W), np.uint32)); bloom.upload_mip(0, np.zeros((H, W), np.uint32))
        cl.open(); cl.copy_texture(back2, back); cl.close()
        dev.execute(cl); dev.wait_idle()
        got = back2.download_mip(0)
        assert got.dtype == np.uint32 and got.shape == (H, W) and np.array_equal(got.ravel(), np.arange(W * H, dtype=np.uint32))
    finally:
        cl.release()
        for r in everything:
            r.release()
    with pytest.raises(rhi.TrhipError, match="one mip"):
        dev.create_texture(W, H, 2, rhi.FORMAT_RGBA8_UNORM, "two mips")
    with pytest.raises(rhi.TrhipError, match="unsupported format"):
        dev.create_texture(W, H, 1, 9, "format 9")
    assert rhi.FORMAT_RGBA8_UNORM == 10
    s, scc = city(tmp_path, oracle)
    v2, scc, mats = with_normals_and_materials(s, scc)
    gs = GpuScene(dev, scc["instances"], s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(v2, s.meshletVertexIds, s.meshletTriangles)
    view = gltf_lite.view_of(s.cameras[0], (64, 32))
    try:
        with pytest.raises(ValueError, match="post=True needs GpuScene.set_materials"):
            FrameDriver(dev, gs, view, record_capacity=64, post=True)
        gs.set_materials(mats)
        with pytest.raises(ValueError, match="post-processing with a shard exchange"):
            FrameDriver(dev, gs, view, record_capacity=64, post=True, shard_late=lambda *a: None)
        with pytest.raises(ValueError, match="Ambient"):
            FrameDriver(dev, gs, view, record_capacity=64, post=True, debug_mode=10)
    finally:
        gs.release()
