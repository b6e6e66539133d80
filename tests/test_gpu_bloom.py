"""BloomRenderer's mip chain on the GPU ("bloom_PS_Downsample", "bloom_PS_Upsample", csrc/k_bloom.hip), every word against
tests/bloom_ref.c: single passes through rhi bindings at sizes around every tile edge, constants through push constants and b0,
sources and destinations at non-zero mips, whole chains through FrameDriver(post=True, bloom_mips=...) and the C++ host mirror
with the existing post reference behind them, and misuse.  Destinations are pre-filled so that a skipped texel shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bloom_ref as BR  # noqa: E402
import postprocess_ref as PR  # noqa: E402
from gbuffer_scenes import with_normals_and_materials  # noqa: E402
from suite_support import bits, bl, dev, gpu_scene, host_renderer, kernel_constant, lit_city, lit_cornell, op_counts, post_chain_reference, pr, recorded, same  # noqa: E402, F401
from toyrenderer_amd import gltf_lite, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import city  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0x12345678
RADII = (0.001, 0.005, 0.1)


def _consts(kind, src_dims, radius):
    k = np.zeros(1, I.BloomConsts)
    if kind == "up":
        k["m_FilterRadius"] = radius
    else:
        k["m_InvSourceResolution"] = (F(1.0) / F(src_dims[0]), F(1.0) / F(src_dims[1]))
        k["m_bIsFirstDownsample"] = int(kind == "first")
    return k


def _dispatch(cl, kind, k, src, src_mip, dst, dst_mip, dst_dims, via="push"):
    from toyrenderer_amd.rhi import CB, PUSH, SAMPLER, TEX_SRV, TEX_UAV
    groups = ((dst_dims[0] + 7) // 8, (dst_dims[1] + 7) // 8, 1)
    name = "bloom_PS_Upsample" if kind == "up" else "bloom_PS_Downsample"
    b = [TEX_SRV(0, src, src_mip), TEX_UAV(0, dst, dst_mip), SAMPLER(0)]
    if via == "push":
        cl.dispatch(name, [PUSH(0)] + b, groups, push=k)
    else:
        cl.dispatch(name, [CB(0, cl.constant_buffer(k, "BloomConsts"))] + b, groups)


def _reference(bl, kind, words, dst_dims, radius):
    if kind == "up":
        return BR.upsample(bl, words, radius, dst_dims)
    return BR.downsample(bl, words, kind == "first", dest=dst_dims)


def _contents(W, H, seed):
    """name -> (H, W) words: seeded over the whole format (NaN and infinity codes included), seeded finite, one value, and the
    special patterns of the CPU tests."""
    out = {"seeded": BR.seeded_words(W, H, seed), "seeded finite": BR.seeded_finite_words(W, H, seed + 1),
           "one value": np.full((H, W), PR.grey(14 << 6 | 37), np.uint32)}
    out.update(BR.special_images(W, H))
    return out


# ---- 1. single passes -----------------------------------------------------------------------------------------------------------
def _tile_edge_sizes():
    """Destination sizes one below, at and one above each edge of the kernels' tile, in both axes, two tiles included (more than
    one workgroup in each axis)."""
    tw, th = kernel_constant("k_bloom.hip", "kBloomTileW"), kernel_constant("k_bloom.hip", "kBloomTileH")
    return [(tw - 1, th - 1), (tw, th), (tw + 1, th + 1), (2 * tw - 1, 2 * th + 1), (2 * tw + 1, 2 * th - 1)]


# the finer level of each pair: a downsample reads it and writes (W >> 1, H >> 1) (at least 1); an upsample writes it from that size
LEVELS = [(2, 2), (16, 16), (17, 17), (67, 35), (129, 3), (270, 135)]
KINDS = [("down", None), ("first", None)] + [("up", r) for r in RADII]


def _single_pass_cases():
    cases = [("level", s) for s in LEVELS]
    for dw, dh in _tile_edge_sizes():
        cases += [("dest even", (dw, dh)), ("dest odd", (dw, dh))]
    return cases


@pytest.mark.parametrize("case", _single_pass_cases(), ids=lambda c: f"{c[0]} {c[1][0]}x{c[1][1]}")
def test_single_passes_match_the_reference(dev, bl, case):
    """Every kind of pass on every content.  "level": the sizes of the issue's list.  "dest even" / "dest odd": the DESTINATION has
    the tile-edge size; the downsample's source is twice that (plus one: the ratio is not 2), the upsample's half of it."""
    from toyrenderer_amd import rhi
    how, (W, H) = case
    half = (max(W >> 1, 1), max(H >> 1, 1))
    if how == "level":
        down, up = ((W, H), half), (half, (W, H))
    else:
        extra = 1 if how == "dest odd" else 0
        down, up = ((2 * W + extra, 2 * H + extra), (W, H)), (half, (W, H))
    cl = dev.create_command_list()
    textures = {}

    def tex(dims, name):
        if (dims, name) not in textures:
            textures[(dims, name)] = dev.create_texture(dims[0], dims[1], 1, rhi.FORMAT_R11G11B10_FLOAT, name)
        return textures[(dims, name)]
    try:
        for kind, radius in KINDS:
            src_dims, dst_dims = up if kind == "up" else down
            src, dst = tex(src_dims, "source"), tex(dst_dims, "destination")
            for name, words in _contents(src_dims[0], src_dims[1], 7 * W + H).items():
                src.upload_mip(0, words)
                dst.upload_mip(0, np.full((dst_dims[1], dst_dims[0]), SENTINEL, np.uint32))
                cl.open()
                _dispatch(cl, kind, _consts(kind, src_dims, radius), src, 0, dst, 0, dst_dims)
                cl.close()
                dev.execute(cl); dev.wait_idle()
                same(dst.download_mip(0), _reference(bl, kind, words, dst_dims, radius), f"{kind} {radius} {src_dims} -> {dst_dims} {name}")
    finally:
        cl.release()
        for t in textures.values():
            t.release()


def test_decoupled_constants_and_large_radius(dev, bl):
    """m_InvSourceResolution is a constant, not derived from the bound source: a step of 3 texels and of 0 is honoured.  An upsample
    at radius 0.45 reads almost across the source (there is no tiled path with a limit: the taps read global memory)."""
    from toyrenderer_amd import rhi
    src_dims, dst_dims = (67, 35), (40, 9)
    words = BR.seeded_finite_words(*src_dims, 5)
    src = dev.create_texture(*src_dims, 1, rhi.FORMAT_R11G11B10_FLOAT, "source")
    dst = dev.create_texture(*dst_dims, 1, rhi.FORMAT_R11G11B10_FLOAT, "destination")
    cl = dev.create_command_list()
    try:
        src.upload_mip(0, words)
        for kind, inv, radius in (("down", (F(3) / F(67), F(3) / F(35)), None), ("first", (F(0), F(0)), None), ("up", None, 0.45), ("up", None, 0.0)):
            k = _consts(kind, src_dims, radius)
            if inv is not None:
                k["m_InvSourceResolution"] = inv
            dst.upload_mip(0, np.full((dst_dims[1], dst_dims[0]), SENTINEL, np.uint32))
            cl.open()
            _dispatch(cl, kind, k, src, 0, dst, 0, dst_dims)
            cl.close()
            dev.execute(cl); dev.wait_idle()
            want = BR.upsample(bl, words, radius, dst_dims) if kind == "up" else BR.downsample(bl, words, kind == "first", dest=dst_dims, inv=inv)
            same(dst.download_mip(0), want, f"{kind} inv {inv} radius {radius}")
    finally:
        cl.release(); src.release(); dst.release()


# ---- 2. constants and mips ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", ["push", "cb"])
def test_passes_between_mips_of_one_texture(dev, bl, via):
    """A source at a non-zero baseMip and a destination at a non-zero mip of the same render target; the other mips keep their
    sentinels.  67 x 35 with 4 mips: 67x35, 33x17, 16x8, 8x4."""
    from toyrenderer_amd import rhi
    W, H, mips = 67, 35, 4
    t = dev.create_texture(W, H, mips, rhi.FORMAT_R11G11B10_FLOAT, "chain", render_target=True)
    cl = dev.create_command_list()
    dims = BR.chain_dims(W, H, mips)
    assert dims == [(67, 35), (33, 17), (16, 8), (8, 4)]
    fill = [np.full((h, w), SENTINEL + k, np.uint32) for k, (w, h) in enumerate(dims)]
    try:
        for kind, s, d, radius in (("down", 1, 2, None), ("first", 2, 3, None), ("up", 3, 2, 0.005), ("up", 2, 1, 0.1), ("up", 1, 0, 0.001)):
            for k in range(mips):
                t.upload_mip(k, fill[k])
            words = BR.seeded_finite_words(*dims[s], 40 + s)
            t.upload_mip(s, words)
            cl.open()
            _dispatch(cl, kind, _consts(kind, dims[s], radius), t, s, t, d, dims[d], via)
            cl.close()
            dev.execute(cl); dev.wait_idle()
            for k in range(mips):
                want = words if k == s else _reference(bl, kind, words, dims[d], radius) if k == d else fill[k]
                same(t.download_mip(k), want, f"{via} {kind} mip {s} -> {d}: mip {k}")
    finally:
        cl.release(); t.release()


# ---- 3. whole chains through FrameDriver ---------------------------------------------------------------------------------------
def _cornell(oracle):
    *scene, camera = lit_cornell(oracle)
    return (*scene, camera, dict(dir_light=((0.3, -0.8, -0.52), 3.0), camera_origin=tuple(float(x) for x in camera.position), auto_exposure=(0.004, 12.0, 0.5)))


def _city(oracle, tmp_path):
    return (*lit_city(oracle, tmp_path), dict(dir_light=((0.2, -1.0, 0.3), 2.5)))


CHAINS = [("cornell", (320, 180), 6, 0.005, 0.1), ("city", (540, 270), 6, 0.005, 0.1), ("city", (67, 35), 2, 0.02, 0.5), ("city", (67, 35), 6, 0.1, 1.0)]


@pytest.mark.parametrize("scene,render,mips,radius,strength", CHAINS, ids=lambda v: str(v))
def test_frames_match_the_reference_chain(dev, oracle, bl, pr, tmp_path, scene, render, mips, radius, strength):
    """Three frames of FrameDriver(post=True, bloom_mips=mips) next to a bloom_mips=0 driver: every bloom mip equals bloom_chain of
    LightingOutput, the back buffer the existing post reference fed mip 0, the luminance carried; everything up to LightingOutput,
    the histogram, the luminance and the pipeline statistics equal the bloom_mips=0 run; the back buffers differ."""
    from toyrenderer_amd.frame import FrameDriver
    s, inst, vertices, mats, camera, kw = _cornell(oracle) if scene == "cornell" else _city(oracle, tmp_path)
    gs = gpu_scene(dev, s, inst, vertices, mats)
    view = gltf_lite.view_of(camera, render)
    base = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, post=True, **kw)
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, post=True, bloom_mips=mips, bloom_filter_radius=radius, bloom_strength=strength, **kw)
    qb, qd = dev.create_pipeline_stats(), dev.create_pipeline_stats()
    dims = BR.chain_dims(*render, mips)
    try:
        assert mips <= BR.max_mips(*render) and dims[-1][0] >= 1 and dims[-1][1] >= 1
        for k, (w, h) in enumerate(dims):                                    # a mip the chain does not write would keep this
            drv.bloom_texture.upload_mip(k, np.full((h, w), SENTINEL, np.uint32))
        luminance = F(1.0)
        for f in range(3):
            for d, q in ((base, qb), (drv, qd)):
                d.record(q); d.run(); d.results()
            what = f"{scene} {render} frame {f}"
            lit = base.lighting_output.download_mip(0)
            for name in ("gbufferA", "visibility", "lighting_output"):
                same(getattr(drv, name).download_mip(0), getattr(base, name).download_mip(0), what + ": " + name)
            same(drv.motion.download_mip(0).view(np.uint16), base.motion.download_mip(0).view(np.uint16), what + ": motion")
            same(drv.depth.download_mip(0).view(np.uint32), base.depth.download_mip(0).view(np.uint32), what + ": depth")
            same(drv.hzb.download_chain(), base.hzb.download_chain(), what + ": HZB")
            same(drv.histogram.download(np.uint32, 256), base.histogram.download(np.uint32, 256), what + ": histogram")
            assert qd.get() == qb.get(), what + ": pipeline statistics"
            assert drv.bloom_consts.tobytes() == BR.pass_consts(*render, mips, radius).tobytes()
            chain = BR.bloom_chain(bl, lit, *render, mips, radius)
            for k in range(mips):
                same(drv.download_bloom(k), chain[k], f"{what}: bloom mip {k}")
            assert drv.post_consts[2].tobytes() == PR.post_params(render, bloom_strength=strength).tobytes()
            back, _, luminance, _ = post_chain_reference(pr, drv, lit, luminance, bloom=chain[0])
            same(drv.back_buffer.download_mip(0), back, what + ": back buffer")
            assert bits(drv.luminance.download(F, 1)).tolist() == bits(luminance).tolist() == bits(base.luminance.download(F, 1)).tolist()
            assert np.count_nonzero(drv.back_buffer.download_mip(0) != base.back_buffer.download_mip(0)) > 0
    finally:
        qb.release(); qd.release(); drv.release(); base.release(); gs.release()


def test_bloom_adds_its_dispatches_between_lighting_and_the_histogram_clear(dev, oracle, tmp_path):
    """bloom_mips = 0 records the post=True list of the parent commit, command for command, and launches the same kernels;
    bloom_mips = m adds exactly m - 1 downsamples and m - 1 upsamples behind the lighting dispatch, in front of the histogram clear."""
    from toyrenderer_amd.frame import FrameDriver
    s, inst, vertices, mats, camera, kw = _city(oracle, tmp_path)
    gs = gpu_scene(dev, s, inst, vertices, mats)
    view = gltf_lite.view_of(camera, (320, 180))
    seen, counts = {}, {}
    try:
        for name, extra in (("post", {}), ("zero", dict(bloom_mips=0, bloom_filter_radius=0.3, bloom_strength=0.9)), ("five", dict(bloom_mips=5))):
            drv = FrameDriver(dev, gs, view, record_capacity=4096, post=True, **extra, **kw)
            try:
                counts[name] = op_counts(dev, drv)
                seen[name] = recorded(drv)
                if name == "zero":
                    assert drv.bloom_texture is None and drv.post_consts[2].tobytes() == PR.post_params((320, 180)).tobytes()
                    with pytest.raises(ValueError, match="bloom generation is off"):
                        drv.download_bloom(0)
            finally:
                drv.release()
    finally:
        gs.release()
    assert seen["zero"] == seen["post"] and counts["zero"] == counts["post"]
    assert counts["five"] == {**counts["post"], "bloom_PS_Downsample#main": 4, "bloom_PS_Upsample#main": 4}
    at = seen["post"].index(("dispatch", "deferredlighting_PS_Main")) + 1
    assert seen["post"][at] == ("clear_buffer_u32", None)                    # the histogram clear
    added = [("dispatch", "bloom_PS_Downsample")] * 4 + [("dispatch", "bloom_PS_Upsample")] * 4
    assert seen["five"] == seen["post"][:at] + added + seen["post"][at:]


# ---- 4. the host mirror ---------------------------------------------------------------------------------------------------------
def test_host_path_over_three_frames(oracle, bl, pr, tmp_path):
    """The C++ host mirror with a moving camera: frame 0 bloom on (6 mips), frame 1 off, frame 2 on with other parameters.
    trhost_download_bloom and the back buffer equal the reference chain of the frame's own LightingOutput, the luminance carried;
    trhost_get_bloom_consts is bit for bit; generation and an uploaded bloom texture refuse each other."""
    from toyrenderer_amd import host
    s, sc0 = city(tmp_path, oracle)
    v, sc0, mats = with_normals_and_materials(s, sc0)
    cam = s.cameras[0]
    render = (540, 270)
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    inst_in = s.instances.copy()
    inst_in["m_MaterialDataIdx"] = sc0["instances"]["m_MaterialDataIdx"]
    uploaded = PR.seeded_finite_words(render[0] * render[1], 91).reshape(render[1], render[0])
    with host_renderer(s, inst_in, (v, s.meshletVertexIds, s.meshletTriangles), mats, render=render, max_groups=4096) as r:
        with pytest.raises(host.HostError, match="post-processing is off"):
            r.set_bloom(True)
        r.set_post_process(True)
        for call in (r.download_bloom, lambda: r.bloom_consts(1)):
            with pytest.raises(host.HostError, match="bloom generation on"):
                call()
        for mips in (1, 10):                                                  # 270 = 2^8 + 14: at most 9 mips
            with pytest.raises(host.HostError, match="at most 9"):
                r.set_bloom(True, mips)
        for radius in (-0.01, float("inf"), float("nan")):
            with pytest.raises(host.HostError, match="finite"):
                r.set_bloom(True, 6, radius)
        r.set_bloom(True, 9)
        r.set_bloom(False)
        r.upload_bloom(uploaded, 0.25)
        with pytest.raises(host.HostError, match="uploaded bloom texture"):
            r.set_bloom(True)
        r.upload_bloom(None)
        r.set_auto_exposure(0.004, 12.0, 0.0025)
        r.set_frame_time_ms(16.0)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        prevV = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
        luminance = F(1.0)
        settings = [(6, 0.005, 0.1), None, (4, 0.03, 0.6)]
        for f, setting in enumerate(settings):
            V = synth.world_to_view((0.1 * f, 0.02 * f, -0.15 * f), cam.orientation)
            view = synth.View(V, prevV, P, float(np.float32(cam.znear)), *render)
            prevV = V
            r.set_camera(view)
            r.set_directional_light((0.2 * f - 0.4, -1.0, 0.3), 2.0 + f)
            if setting is None:
                r.set_bloom(False)
            else:
                r.set_bloom(True, *setting)
                with pytest.raises(host.HostError, match="bloom generation is on"):
                    r.upload_bloom(uploaded, 0.25)
            r.frame()
            r.results()
            lit = r.download_lighting_output()
            hk, ak, pk = r.post_process_consts()
            luminance, _ = PR.adapt_exposure(pr, ak, PR.histogram(pr, lit, hk), luminance)
            if setting is None:
                assert pk.tobytes() == PR.post_params(render).tobytes()
                same(r.download_back_buffer(), PR.post(pr, pk, lit, luminance_in=luminance), f"frame {f}: back buffer without bloom")
                with pytest.raises(host.HostError, match="did not run"):
                    r.bloom_consts(1)
            else:
                mips, radius, strength = setting
                assert pk.tobytes() == PR.post_params(render, bloom_strength=strength).tobytes()
                assert r.bloom_consts(2 * (mips - 1)).tobytes() == BR.pass_consts(*render, mips, radius).tobytes()
                with pytest.raises(host.HostError, match="did not run"):
                    r.bloom_consts(2 * (mips - 1) + 1)
                chain = BR.bloom_chain(bl, lit, *render, mips, radius)
                for k in range(mips):
                    same(r.download_bloom(k), chain[k], f"frame {f}: bloom mip {k}")
                same(r.download_back_buffer(), PR.post(pr, pk, lit, bloom=chain[0], luminance_in=luminance), f"frame {f}: back buffer")
            assert bits(r.scene_luminance()[0]).tolist() == bits(luminance).tolist(), f


# ---- 5. misuse at the back end --------------------------------------------------------------------------------------------------
def test_misuse_is_refused(dev, bl):
    """Each refusal happens while the command is recorded, so no kernel is launched; the device stays usable."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import PUSH, SAMPLER, TEX_SRV, TEX_UAV
    W, H = 32, 16
    mk = lambda w, h, fmt, name: dev.create_texture(w, h, 1, fmt, name)                                  # noqa: E731
    src, dst = mk(W, H, rhi.FORMAT_R11G11B10_FLOAT, "source"), mk(W // 2, H // 2, rhi.FORMAT_R11G11B10_FLOAT, "destination")
    r32, back = mk(W, H, rhi.FORMAT_R32_FLOAT, "R32"), mk(W // 2, H // 2, rhi.FORMAT_RGBA8_UNORM, "RGBA8")
    chain = dev.create_texture(W, H, 3, rhi.FORMAT_R11G11B10_FLOAT, "chain", render_target=True)
    args = dev.create_buffer(12, "args", stride=12, indirect=True)
    cl = dev.create_command_list()
    k = _consts("down", (W, H), None)
    groups = (2, 1, 1)
    try:
        with pytest.raises(rhi.TrhipError, match="one mip"):                 # a mip chain needs the render-target flag
            dev.create_texture(W, H, 3, rhi.FORMAT_R11G11B10_FLOAT, "no flag")
        with pytest.raises(rhi.TrhipError, match="one mip"):
            dev.create_texture(W, H, 3, rhi.FORMAT_RGBA8_UNORM, "another format", render_target=True)
        dev.profile_reset(); dev.profile_enable(True)
        cl.open()
        for name in ("bloom_PS_Downsample", "bloom_PS_Upsample"):
            bad = [
                ("R11G11B10_FLOAT source", [PUSH(0), TEX_SRV(0, r32), TEX_UAV(0, dst, 0)], groups, k),
                ("R11G11B10_FLOAT destination", [PUSH(0), TEX_SRV(0, src), TEX_UAV(0, back, 0)], groups, k),
                ("R11G11B10_FLOAT source", [PUSH(0), TEX_UAV(0, dst, 0)], groups, k),
                ("R11G11B10_FLOAT destination", [PUSH(0), TEX_SRV(0, src)], groups, k),
                ("BloomConsts, 16 bytes", [TEX_SRV(0, src), TEX_UAV(0, dst, 0)], groups, None),
                ("BloomConsts, 16 bytes", [PUSH(0), TEX_SRV(0, src), TEX_UAV(0, dst, 0)], groups, k.view(np.uint32)[:3]),
                ("same mip", [PUSH(0), TEX_SRV(0, chain, 1), TEX_UAV(0, chain, 1)], groups, k),
                ("same mip", [PUSH(0), TEX_SRV(0, src), TEX_UAV(0, src, 0)], (4, 2, 1), k),
                ("t0 mip 3 out of range", [PUSH(0), TEX_SRV(0, chain, 3), TEX_UAV(0, chain, 1)], groups, k),
                ("UAV mip 3 out of range", [PUSH(0), TEX_SRV(0, chain, 0), TEX_UAV(0, chain, 3)], groups, k),
                ("covering the 16x8 destination", [PUSH(0), TEX_SRV(0, src), TEX_UAV(0, dst, 0)], (1, 1, 1), k),
            ]
            for match, bindings, g, push in bad:
                with pytest.raises(rhi.TrhipError, match=match):
                    cl.dispatch(name, bindings, g, push=push)
            with pytest.raises(rhi.TrhipError, match="direct dispatch"):
                cl.dispatch_indirect(name, [PUSH(0), TEX_SRV(0, src), TEX_UAV(0, dst, 0)], args, push=k)
        cl.close()
        dev.execute(cl); dev.wait_idle()
        assert not any(n.startswith("bloom_") for n in dev.profile()), dev.profile()      # nothing was launched
        dev.profile_enable(False)
        # the device is still usable: a good pass right behind, samplers accepted and ignored
        words = BR.seeded_finite_words(W, H, 3)
        src.upload_mip(0, words)
        dst.upload_mip(0, np.full((H // 2, W // 2), SENTINEL, np.uint32))
        cl.open()
        cl.dispatch("bloom_PS_Downsample", [PUSH(0), TEX_SRV(0, src), TEX_UAV(0, dst, 0), SAMPLER(0), SAMPLER(3)], groups, push=k)
        cl.close()
        dev.execute(cl); dev.wait_idle()
        same(dst.download_mip(0), BR.downsample(bl, words, False), "a good pass after the refusals")
    finally:
        dev.profile_enable(False)
        cl.release(); args.release()
        for t in (src, dst, r32, back, chain):
            t.release()
