"""Temporal anti-aliasing on the GPU ("taa_CS_TemporalResolve", csrc/k_taa.hip), every word against tests/taa_ref.c: direct
dispatches on uploaded inputs at sizes with partial tiles and waves; the constructed cases of tests/test_taa_ref.py; six frames of
the lit Cornell fixture through FrameDriver(taa=...) under a camera that moves and turns, the history carried on both sides; the
driver with taa=None; a reset; and misuse.  Both outputs are pre-filled with a sentinel so that a skipped texel shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import postprocess_ref as PR  # noqa: E402
import taa_ref as TR  # noqa: E402
import taa_scenes as TS  # noqa: E402
from suite_support import bits, dev, gpu_scene, gr, host_renderer, kernel_constant, lit_cornell, lr, op_counts, pr, recorded, recorded_kinds, ref_library, same, vr  # noqa: E402, F401
from toyrenderer_amd import interop as I  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0x12345678
NAME = "taa_CS_TemporalResolve"
ta = ref_library(TR)

TILE = (kernel_constant("k_taa.hip", "kTaaTileW"), kernel_constant("k_taa.hip", "kTaaTileH"))
LDS_TILE = (kernel_constant("k_taa.hip", "kTaaLdsTileW"), kernel_constant("k_taa.hip", "kTaaLdsTileH"))
# one texel, every neighbour clamping, one 8 x 8 group, exactly one tile and one more in each axis, several tiles with partial
# ones on both axes, a partial wave per row; then where the LDS design's tile and its halo end
SIZES = [(1, 1), (2, 2), (8, 8), TILE, (TILE[0] + 1, TILE[1] + 1), (67, 35), (129, 3), LDS_TILE, (LDS_TILE[0] + 1, LDS_TILE[1] + 1), (2 * LDS_TILE[0] - 1, 2 * LDS_TILE[1] - 1)]


class Pass:
    """The pass's six textures at one size; run() uploads one set of inputs, dispatches and returns (history bits, colour words)."""

    def __init__(self, dev, W, H):
        from toyrenderer_amd import rhi
        self.dev, self.W, self.H = dev, W, H
        mk = lambda fmt, name: dev.create_texture(W, H, 1, fmt, name)                                 # noqa: E731
        self.colour, self.depth, self.motion = mk(rhi.FORMAT_R11G11B10_FLOAT, "Lighting Output"), mk(rhi.FORMAT_R32_FLOAT, "Depth Buffer"), mk(rhi.FORMAT_RG16_FLOAT, "GBufferMotion")
        self.history, self.new = mk(rhi.FORMAT_RGBA16_FLOAT, "TAA History 0"), mk(rhi.FORMAT_RGBA16_FLOAT, "TAA History 1")
        self.out = mk(rhi.FORMAT_R11G11B10_FLOAT, "Anti-Aliased Lighting Output")
        self.cl = dev.create_command_list()

    def bindings(self, **other):
        from toyrenderer_amd.rhi import TEX_SRV, TEX_UAV
        t = dict(t0=self.colour, t1=self.depth, t2=self.motion, t3=self.history, u0=self.new, u1=self.out)
        t.update(other)
        return [TEX_SRV(0, t["t0"]), TEX_SRV(1, t["t1"]), TEX_SRV(2, t["t2"]), TEX_SRV(3, t["t3"]), TEX_UAV(0, t["u0"], 0), TEX_UAV(1, t["u1"], 0)]

    def groups(self):
        return ((self.W + 7) // 8, (self.H + 7) // 8, 1)

    def run(self, k, colour, depth, motion, history, constant_buffer=False):
        from toyrenderer_amd.rhi import CB, PUSH
        W, H = self.W, self.H
        self.colour.upload_mip(0, np.ascontiguousarray(colour, np.uint32).reshape(H, W))
        self.depth.upload_mip(0, np.ascontiguousarray(depth, F).reshape(H, W))
        self.motion.upload_mip(0, np.ascontiguousarray(motion).view(np.float16).reshape(H, W, 2))
        self.history.upload_mip(0, np.ascontiguousarray(history).view(np.float16).reshape(H, W, 4))
        self.new.upload_mip(0, np.full((H, W, 4), 0x5555, np.uint16).view(np.float16))
        self.out.upload_mip(0, np.full((H, W), SENTINEL, np.uint32))
        cl = self.cl
        cl.open()
        if constant_buffer:
            cl.dispatch(NAME, self.bindings() + [CB(0, cl.constant_buffer(k, "TAAConsts"))], self.groups())
        else:
            cl.dispatch(NAME, self.bindings() + [PUSH(0)], self.groups(), push=k)
        cl.close()
        self.dev.execute(cl); self.dev.wait_idle()
        return self.new.download_mip(0).view(np.uint16), self.out.download_mip(0)

    def release(self):
        self.cl.release()
        for t in (self.colour, self.depth, self.motion, self.history, self.new, self.out):
            t.release()


def _compare(p, ta, k, inputs, what, **kw):
    new, out = p.run(k, *inputs, **kw)
    want_new, want_out, path = TR.resolve(ta, k, *inputs)
    same(out, want_out, what + ": AntiAliasedLightingOutput")
    same(new, want_new, what + ": history")
    return path


# ---- 1. direct dispatches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_resolve_matches_the_reference(dev, ta, size):
    """Seeded words over the whole of every format (the colour's and the history's NaN and infinity codes, negative history, NaN
    depths, depth ties), with and without a jitter delta, a reset, a low cap on the count; then the constructed cases where the
    size holds them."""
    W, H = size
    p = Pass(dev, W, H)
    try:
        seen = np.zeros((H, W), np.uint8)
        for i, (delta, finite, reset, cap) in enumerate((((0.0, 0.0), False, False, 64.0), ((0.25, -0.125), True, False, 64.0), ((-0.4375, 0.3125), True, False, 3.0),
                                                         ((0.25, -0.125), False, True, 64.0))):
            inputs = TR.seeded_inputs(W, H, 100 * i + W, finite_history=finite)
            k = TR.consts(W, H, jitter_delta=delta, reset=reset, max_sample_count=cap, min_blend=0.05 * i)
            seen |= _compare(p, ta, k, inputs, f"{W}x{H} seeded {i}", constant_buffer=bool(i & 1))
        if W * H >= 64:
            assert np.any(seen & TR.VALID) and np.any(seen & TR.CLAMPED) and np.any(seen & TR.DILATED) and np.any((seen & TR.WEIGHTS) == TR.WEIGHTS)
        if W >= 8 and H >= 4:
            for name, (k, *inputs) in TR.constructed_cases(W, H).items():
                _compare(p, ta, k, inputs, f"{W}x{H} {name}")
    finally:
        p.release()


# ---- 2. frames through the driver ---------------------------------------------------------------------------------------------
class Cornell:
    """The lit Cornell fixture on the device and what the reference chain needs of it."""

    def __init__(self, dev, oracle):
        self.s, self.inst, _, self.mats, self.camera = lit_cornell(oracle)
        self.sc = dict(self.s.as_oracle()); self.sc["instances"] = self.inst
        self.geo_v = (self.s.vertices, self.s.meshletVertexIds, self.s.meshletTriangles)
        self.gs = gpu_scene(dev, self.s, self.inst, self.s.vertices, self.mats)

    def driver(self, dev, f=0, **kw):
        from toyrenderer_amd.frame import FrameDriver
        eye, _ = TS.camera_at(self.camera, f)
        return FrameDriver(dev, self.gs, TS.view_at(self.camera, f), record_capacity=4096, culling_flags=7, post=True, dir_light=TS.LIGHT, camera_origin=eye,
                           auto_exposure=(0.004, 12.0, 0.5), **kw)

    def frame(self, drv, f):
        """Record and run frame f of the camera path."""
        eye, _ = TS.camera_at(self.camera, f)
        drv.view, drv.camera_origin, drv.frame_counter = TS.view_at(self.camera, f), eye, f
        drv.record(); drv.run(); drv.results()

    def reference(self, oracle, vr, gr, lr, drv):
        """(depth, motion words, LightingOutput) of the frame the driver just recorded, from its own jittered view and constants."""
        return TS.frame_inputs(oracle, vr, gr, lr, self.sc, self.geo_v, drv.taa_view, drv.taa_prev_world_to_clip, self.mats, drv.lighting_consts)


def _post_reference(pr, drv, lighting_output, colour, luminance):
    """The chain behind the resolve: histogram and exposure from LightingOutput, the post pass on `colour`."""
    hk, ak, pk = drv.post_consts
    luminance, _ = PR.adapt_exposure(pr, ak, PR.histogram(pr, lighting_output, hk), luminance)
    return PR.post(pr, pk, colour, bloom=None, luminance_in=luminance), luminance


def test_frames_match_the_reference_chain(dev, oracle, vr, gr, lr, pr, ta):
    """Six frames, jitter on, a camera that translates and turns between records: LightingOutput, depth, motion, the history, the
    anti-aliased output and the back buffer of every frame equal the existing frame reference fed drv.taa_view, then taa_ref on
    the carried history, then the post reference on the anti-aliased output.  The chain's path bytes meet taa_scenes.check_condition."""
    c = Cornell(dev, oracle)
    drv = c.driver(dev, taa=dict(TS.SETTINGS))
    W, H = TS.RENDER
    history, luminance, paths = np.zeros((H, W, 4), np.uint16), F(1.0), []
    try:
        for f in range(TS.FRAMES):
            c.frame(drv, f)
            what = f"frame {f}"
            current, previous = drv.taa_jitter
            assert tuple(map(float, current)) == tuple(map(float, TR.jitter_sequence(f + 1)[f])) and (f == 0 or tuple(map(float, previous)) == tuple(map(float, TR.jitter_sequence(f)[f - 1])))
            assert int(drv.taa_consts["m_bResetHistory"][0]) == int(f == 0)
            depth, motion, lit = c.reference(oracle, vr, gr, lr, drv)
            same(drv.depth.download_mip(0).view(np.uint32), depth.view(np.uint32), what + ": depth")
            same(drv.motion.download_mip(0).view(np.uint32).reshape(H, W), motion, what + ": motion")
            same(drv.lighting_output.download_mip(0), lit, what + ": LightingOutput")
            history, aa, path = TR.resolve(ta, drv.taa_consts, lit, depth, motion, history)
            paths.append(path)
            same(drv.download_taa_history().view(np.uint16), history, what + ": history")
            same(drv.download_anti_aliased_output(), aa, what + ": AntiAliasedLightingOutput")
            back, luminance = _post_reference(pr, drv, lit, aa, luminance)
            same(drv.back_buffer.download_mip(0), back, what + ": back buffer")
            if f:
                assert np.count_nonzero(aa != lit) > 50, "the resolve changes the image"
        TS.check_condition(paths)
    finally:
        drv.release(); c.gs.release()


def test_taa_off_changes_nothing_and_on_adds_one_dispatch(dev, oracle, vr, gr, lr, pr):
    """taa=None: the launches and commands of a post=True driver (which tests/test_gpu_postprocess.py pins) and the back buffer of
    the reference chain without a resolve.  taa=...: one dispatch more, in front of the post pass and behind the exposure passes."""
    c = Cornell(dev, oracle)
    off, on = c.driver(dev), c.driver(dev, taa=dict(TS.SETTINGS))
    try:
        assert off.taa is None and off.taa_history is None and off.anti_aliased_output is None
        ops_off, ops_on = op_counts(dev, off), op_counts(dev, on)
        assert NAME + "#main" not in ops_off and ops_on == {**ops_off, NAME + "#main": 1}
        kinds_off, kinds_on = recorded_kinds(off), recorded_kinds(on)
        assert kinds_on == {**kinds_off, "dispatch": kinds_off["dispatch"] + 1}
        order = [n for _, n in recorded(on) if n]
        assert order[-3:] == ["adaptluminance_CS_AdaptExposure", NAME, "postprocess_PS_PostProcess"] and NAME not in [n for _, n in recorded(off)]
        off.reset_exposure()
        off.record(); off.run(); off.results()
        view = off.view
        _, _, lit = TS.frame_inputs(oracle, vr, gr, lr, c.sc, c.geo_v, view, I.world_to_clip(view.prevWorldToView, view.viewToClip), c.mats, off.lighting_consts)
        same(off.lighting_output.download_mip(0), lit, "taa=None: LightingOutput")
        back, _ = _post_reference(pr, off, lit, lit, F(1.0))
        same(off.back_buffer.download_mip(0), back, "taa=None: back buffer")
        for call in (off.reset_taa, off.download_anti_aliased_output, off.download_taa_history):
            with pytest.raises(ValueError, match="taa=None"):
                call()
    finally:
        off.release(); on.release(); c.gs.release()


def test_without_jitter_a_static_camera_keeps_todays_motion(dev, oracle):
    """jitter=False and a camera that does not move: the projection is the view's own, so depth, motion and LightingOutput equal a
    taa=None driver's on every frame, and from the second frame on every texel has valid history at its own position."""
    c = Cornell(dev, oracle)
    off, on = c.driver(dev), c.driver(dev, taa=dict(TS.SETTINGS, jitter=False))
    try:
        for f in range(3):
            for d in (off, on):
                d.frame_counter = f
                d.record(); d.run(); d.results()
            assert np.array_equal(on.taa_view.viewToClip, off.view.viewToClip) and tuple(map(float, on.taa_jitter[0])) == (0.0, 0.0)
            assert on.taa_consts.tobytes() == TR.consts(*TS.RENDER, reset=f == 0, max_sample_count=TS.SETTINGS["max_sample_count"]).tobytes()
            for name in ("depth", "motion", "lighting_output"):
                same(getattr(on, name).download_mip(0).view(np.uint32), getattr(off, name).download_mip(0).view(np.uint32), f"frame {f}: {name}")
            count = on.download_taa_history()[..., 3].astype(F)
            assert np.all(count == f + 1), f
    finally:
        off.release(); on.release(); c.gs.release()


def test_reset_mid_run(dev, oracle):
    """reset_taa(): the next frame's output is LightingOutput's words and every count is 1 again."""
    c = Cornell(dev, oracle)
    drv = c.driver(dev, taa=dict(TS.SETTINGS))
    try:
        for f in range(4):
            if f == 2:
                drv.reset_taa()
            c.frame(drv, f)
            lit, aa = drv.lighting_output.download_mip(0), drv.download_anti_aliased_output()
            reset = f in (0, 2)
            assert int(drv.taa_consts["m_bResetHistory"][0]) == int(reset)
            assert np.array_equal(aa, lit) == reset, f
            assert np.all(drv.download_taa_history()[..., 3].astype(F) == 1.0) == reset, f
    finally:
        drv.release(); c.gs.release()


# ---- 3. misuse ------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused(dev, oracle):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import PUSH
    W, H = 24, 16
    p = Pass(dev, W, H)
    mk = lambda w, h, fmt, name: dev.create_texture(w, h, 1, fmt, name)                                # noqa: E731
    wrong = {"t0": (mk(W, H, rhi.FORMAT_R32_FLOAT, "R32"), "t0"), "t1": (mk(W, H, rhi.FORMAT_R16_FLOAT, "R16"), "t1"), "t2": (mk(W, H, rhi.FORMAT_RG32_UINT, "RG32"), "t2"),
             "t3": (mk(W, H, rhi.FORMAT_RGBA32_UINT, "RGBA32"), "t3"), "u0": (mk(W, H, rhi.FORMAT_RG16_FLOAT, "RG16"), "u0"), "u1": (mk(W, H, rhi.FORMAT_RGBA8_UNORM, "RGBA8"), "u1")}
    small = {"t0": mk(W // 2, H, rhi.FORMAT_R11G11B10_FLOAT, "small colour"), "t1": mk(W, H // 2, rhi.FORMAT_R32_FLOAT, "small depth"),
             "t2": mk(W // 2, H, rhi.FORMAT_RG16_FLOAT, "small motion"), "t3": mk(W, H + 1, rhi.FORMAT_RGBA16_FLOAT, "tall history"),
             "u0": mk(W + 1, H, rhi.FORMAT_RGBA16_FLOAT, "wide history"), "u1": mk(W // 2, H // 2, rhi.FORMAT_R11G11B10_FLOAT, "small output")}
    args = dev.create_buffer(12, "args", stride=12, indirect=True)
    args.upload(np.array([3, 2, 1], np.uint32))
    k, g = TR.consts(W, H), p.groups()
    cl = p.cl
    try:
        cl.open()
        cases = [("constants missing", p.bindings(), g, None, "TAAConsts"), ("constants too short", p.bindings() + [PUSH(0)], g, k.view(np.uint32)[:7], "TAAConsts"),
                 ("empty", p.bindings() + [PUSH(0)], g, TR.consts(0, H), "empty"), ("dims differ", p.bindings() + [PUSH(0)], g, TR.consts(W, H - 1), "m_OutputDims"),
                 ("t3 is u0", p.bindings(u0=p.history) + [PUSH(0)], g, k, "same texture"), ("t0 is u1", p.bindings(u1=p.colour) + [PUSH(0)], g, k, "same texture"),
                 ("grid too small", p.bindings() + [PUSH(0)], (g[0] - 1, g[1], 1), k, "covering"), ("grid too small in y", p.bindings() + [PUSH(0)], (g[0], g[1] - 1, 1), k, "covering")]
        for slot, (tex, text) in wrong.items():
            cases.append((slot + " wrong format", p.bindings(**{slot: tex}) + [PUSH(0)], g, k, text))
        for slot, tex in small.items():
            cases.append((slot + " wrong size", p.bindings(**{slot: tex}) + [PUSH(0)], g, k, "m_OutputDims"))
        for slot in ("t0", "t1", "t2", "t3", "u0", "u1"):
            b = [x for x, s in zip(p.bindings(), ("t0", "t1", "t2", "t3", "u0", "u1")) if s != slot]
            cases.append((slot + " missing", b + [PUSH(0)], g, k, slot))
        for what, b, grp, push, text in cases:
            with pytest.raises(rhi.TrhipError, match=text) as e:
                cl.dispatch(NAME, b, grp, push=push)
            assert NAME in str(e.value), (what, str(e.value))
        with pytest.raises(rhi.TrhipError, match="direct dispatch") as e:
            cl.dispatch_indirect(NAME, p.bindings() + [PUSH(0)], args, push=k)
        assert NAME in str(e.value)
        cl.dispatch(NAME, p.bindings() + [PUSH(0)], g, push=k)
        cl.close()
    finally:
        p.release(); args.release()
        for t in [t for t, _ in wrong.values()] + list(small.values()):
            t.release()
    c = Cornell(dev, oracle)
    try:
        from toyrenderer_amd.frame import FrameDriver
        kw = dict(record_capacity=64, dir_light=TS.LIGHT)
        with pytest.raises(ValueError, match="taa=... needs post=True"):
            FrameDriver(dev, c.gs, TS.view_at(c.camera, 0), lighting=True, taa={}, **kw)
        with pytest.raises(ValueError, match="unknown settings"):
            FrameDriver(dev, c.gs, TS.view_at(c.camera, 0), post=True, taa=dict(sharpening=0.5), **kw)
        with pytest.raises(ValueError, match="min_blend"):
            FrameDriver(dev, c.gs, TS.view_at(c.camera, 0), post=True, taa=dict(min_blend=2.0), **kw)
    finally:
        c.gs.release()


# ---- 4. the host mirror ---------------------------------------------------------------------------------------------------------
def test_host_path_over_six_frames(oracle, vr, gr, lr, pr, ta):
    """The C++ host mirror (trhost_set_taa) over the same six frames: View::Update's jitter, jittered projection and kept
    m_PrevWorldToClip are taa.begin_frame's (the sequence FrameDriver runs), trhost_get_taa_consts gives taa.consts of them, and
    LightingOutput, the history, the anti-aliased output and the back buffer equal the reference chain; a reset mid-run; with TAA
    switched off again the post pass reads LightingOutput; misuse at the facade."""
    from toyrenderer_amd import host
    from toyrenderer_amd import taa as T
    s, inst, _, mats, camera = lit_cornell(oracle)
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    settings = T.check_settings(TS.SETTINGS)
    W, H = TS.RENDER
    with host_renderer(s, inst, geo_v, mats, render=TS.RENDER, max_groups=4096) as r:
        with pytest.raises(host.HostError, match="post-processing is off"):
            r.set_taa(True)
        r.set_post_process(True)
        for call in (r.download_anti_aliased_output, r.download_taa_history, r.taa_consts, r.reset_taa_history):
            with pytest.raises(host.HostError, match="anti-aliasing"):
                call()
        for bad, text in (((1.5, 64.0), "min_blend"), ((0.1, 0.0), "max_sample_count")):
            with pytest.raises(host.HostError, match=text):
                r.set_taa(True, *bad)
        r.set_taa(True, settings["min_blend"], settings["max_sample_count"])
        r.set_auto_exposure(0.004, 12.0, 0.0025)
        r.set_frame_time_ms(16.0)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        r.set_directional_light(*TS.LIGHT)
        last, luminance, history, reset_at = None, F(1.0), np.zeros((H, W, 4), np.uint16), 3
        for f in range(TS.FRAMES):
            base = TS.view_at(camera, f)
            r.set_camera(base)
            if f == reset_at:
                r.reset_taa_history()
            r.frame()
            r.results()
            what = f"frame {f}"
            view, (current, previous), prev_world_to_clip, last = T.begin_frame(base, f + 1, settings, last)     # the host's frame counter is 1 in its first frame
            k, got_current, got_previous = r.taa_consts()
            assert k.tobytes() == T.consts(W, H, settings, current, previous, f in (0, reset_at)).tobytes(), what
            assert bits(got_current).tolist() == bits(current).tolist() and bits(got_previous).tolist() == bits(previous).tolist(), what
            sc = dict(s.as_oracle()); sc["instances"] = r.instances(len(s.instances))
            depth, motion, lit = TS.frame_inputs(oracle, vr, gr, lr, sc, geo_v, view, prev_world_to_clip, mats, r.deferred_lighting_consts())
            same(r.download_motion().view(np.uint32).reshape(H, W), motion, what + ": motion")
            same(r.download_lighting_output(), lit, what + ": LightingOutput")
            history, aa, _ = TR.resolve(ta, k, lit, depth, motion, history)
            same(r.download_taa_history().view(np.uint16), history, what + ": history")
            same(r.download_anti_aliased_output(), aa, what + ": AntiAliasedLightingOutput")
            hk, ak, pk = r.post_process_consts()
            luminance, _ = PR.adapt_exposure(pr, ak, PR.histogram(pr, lit, hk), luminance)
            same(r.download_back_buffer(), PR.post(pr, pk, aa, bloom=None, luminance_in=luminance), what + ": back buffer")
            if f in (0, reset_at):
                same(aa, lit, what + ": a reset gives LightingOutput")
        r.set_taa(False)
        r.set_camera(TS.view_at(camera, TS.FRAMES - 1))
        r.frame(); r.results()
        hk, ak, pk = r.post_process_consts()
        lit = r.download_lighting_output()
        luminance, _ = PR.adapt_exposure(pr, ak, PR.histogram(pr, lit, hk), luminance)
        same(r.download_back_buffer(), PR.post(pr, pk, lit, bloom=None, luminance_in=luminance), "TAA off again: the post pass reads LightingOutput")
        with pytest.raises(host.HostError, match="anti-aliasing"):
            r.download_anti_aliased_output()
