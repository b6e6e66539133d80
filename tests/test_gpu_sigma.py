"""The sun shadow denoiser on the GPU, every word of every output against tests/sigma_ref.c: the penumbra trace of
"shadowmask_CS_ShadowMask" with m_bDoDenoising = 1 and "shadowmask_CS_PackNormalAndRoughness" (csrc/k_shadowmask.hip), and
"SIGMA_Shadow_ClassifyTiles.cs", "SIGMA_Shadow_Blur.cs", "SIGMA_Shadow_PostBlur.cs" and "SIGMA_Shadow_TemporalStabilization.cs"
(csrc/k_sigma.hip) as direct dispatches on the inputs of tests/sigma_scenes.py (tests/test_sigma_ref.py asserts on the CPU that
those reach every path), whole frames through FrameDriver(shadow_denoise=...), the recorded command list and misuse.  Every target
is pre-filled with a sentinel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import alpha_test_scenes as A  # noqa: E402
import lighting_ref as LR  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
import sigma_passes as P  # noqa: E402
import sigma_ref as SG  # noqa: E402
import sigma_scenes as S  # noqa: E402
import taa_scenes as TS  # noqa: E402
from shadow_passes import REFIT, TRACE  # noqa: E402
from suite_support import bare_gpu_scene, dev, gpu_scene, lr, op_counts, recorded, recorded_kinds, ref_library, same, shadow_case_reference  # noqa: E402, F401
from toyrenderer_amd import accel, gltf_lite  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
sg = ref_library(SG)
OUTPUTS = ("normal_roughness", "tiles", "data0", "data1", "data2", "history", "mask")


INPUTS = S.inputs()
CONSTRUCTED = {"dilation": S.dilation, "depth step": S.depth_step, "sky band": S.sky_band, "hard 33x18": lambda: S.seeded(33, 18, 3, hard=True),
               "all lit": lambda: S.flat(33, 18), "constant": lambda: dict(S.flat(17, 17), penumbra=np.full((17, 17), 0x3800, np.uint16), history=np.full((17, 17), 0, np.uint16))}


def _compare(dev, sg, name, s):
    W, H = (int(x) for x in s["k"]["m_OutputDims"][0])
    want = S.run(sg, s)
    c = P.Chain(dev, W, H)
    try:
        got = c.run(s)
    finally:
        c.release()
    for key in OUTPUTS:
        same(got[key], want[key], f"{name}: {key}")
    return want


# ---- 1. the entries ------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_registered(dev):
    from toyrenderer_amd import rhi
    for name in P.ENTRIES:
        assert rhi.load().trhip_shader_exists(name.encode()) == 1, name


# ---- 2. the chain on seeded and constructed inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", INPUTS, ids=lambda c: c[0])
def test_the_chain_equals_the_definition(dev, sg, case):
    """Pack, classify, blur, post-blur and stabilisation, each fed what the one before left: every word of the normal roughness
    texture, the tiles, the shadow data after each of the three passes that write it, the new history and the mask."""
    _compare(dev, sg, *case)


@pytest.mark.parametrize("name", list(CONSTRUCTED))
def test_the_constructed_cases_equal_the_definition(dev, sg, name):
    want = _compare(dev, sg, name, CONSTRUCTED[name]())
    if name == "dilation":
        assert want["mask"][16, 16] < 255 and want["tiles"][0, 0] == 3 and want["tiles"][1, 1] == 1
    if name == "all lit":
        assert np.all(want["mask"] == 255) and not want["path"].any()


def test_a_second_frame_reads_the_first_frame_s_history(dev, sg):
    """The stabilisation once more on what a first frame left on the GPU, reading the history that frame wrote (ping-pong: it reads
    history 1 and writes history 0), against the reference fed the reference's history; then with a reset, which reads none of it."""
    s = S.seeded(47, 49, 31)
    first = S.run(sg, s)
    want = {}
    for reset in (False, True):
        k = S.consts(47, 49, frame=4, reset=reset)
        want[reset] = (k, *SG.stabilize(sg, k, first["data2"], s["lvd"], s["motion"], first["history"], first["tiles"]))
    assert want[False][3] > 1000 and want[True][3] == 0 and np.count_nonzero(want[False][2] != want[True][2]) > 100
    c = P.Chain(dev, 47, 49)
    try:
        got = c.run(s)
        same(got["history"], first["history"], "frame 0: history")
        for reset in (False, True):
            k, history, mask, _ = want[reset]
            c.history[0].upload_mip(0, np.full((49, 47), SG.SENTINEL16, np.uint16))
            c.mask.upload_mip(0, np.full((49, 47), SG.SENTINEL8, np.uint8))
            c.dispatch(P.STABILIZE, c.stabilize_bindings(src=1, dst=0), c.groups(), consts=k)
            same(c.history[0].download_mip(0), history, f"frame 1, reset {reset}: history")
            same(c.mask.download_mip(0), mask, f"frame 1, reset {reset}: mask")
    finally:
        c.release()


def test_push_constants_serve_as_b0(dev, sg):
    """SigmaConsts as push constants: the same words as through the constant buffer."""
    from toyrenderer_amd.rhi import PUSH
    s = S.seeded(33, 18, 40)
    want = S.run(sg, s)
    c = P.Chain(dev, 33, 18)
    try:
        c.penumbra.upload_mip(0, s["penumbra"]); c.lvd.upload_mip(0, s["lvd"])
        c.dispatch(P.CLASSIFY, [PUSH(0)] + c.classify_bindings(), c.groups(16), push=s["k"])
        same(c.tiles.download_mip(0), want["tiles"], "tiles")
        same(P.rg16_words(c.data[0].download_mip(0)), want["data0"], "shadow data")
    finally:
        c.release()


# ---- 3. the penumbra trace --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SS.CASES, ids=lambda c: c[0])
def test_the_penumbra_trace_equals_brute_force(dev, sg, case):
    """m_bDoDenoising = 1 on the mask tests' cases: u0 equals brute force's closest committing t, packed; u1 is what the m_bDoDenoising = 0
    trace writes; far texels keep u0's sentinel; a texel is occluded exactly where the mask is 0."""
    sc, acc, k, depth, g, noise, mask, lvd = shadow_case_reference(sg, case)
    W, H = case[2]
    want, want_lvd, _ = SG.trace_penumbra(sg, k, acc, depth, g, noise, SG.BRUTE)
    assert np.array_equal(want_lvd, lvd) and np.array_equal((want < SG.NO_OCCLUDER)[depth != 0], (mask == 0)[depth != 0])
    gs = bare_gpu_scene(dev, sc)
    p = P.PenumbraPass(dev, gs, W, H, noise)
    try:
        got, got_lvd = p.run(k, depth, g)
        same(got, want, f"{case[0]}: penumbra")
        same(got_lvd, lvd, f"{case[0]}: linear view depth")
        assert np.all(got[depth == 0] == SG.SENTINEL16)
    finally:
        p.release(); gs.release()


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_the_textured_penumbra_trace_equals_brute_force(dev, sg, soft):
    """The checker cut-out above a floor with the texture table at t19: the textured_penumbra instantiation equals brute force with the
    textured alpha test, and differs from the trace without the table (the solid card)."""
    from toyrenderer_amd.frame import GpuScene
    sc = A.shadow_scene()
    acc = SR.Accel(sc)
    W, H = 67, 35
    depth, g = SS.images(W, H, 50)
    g[..., 1] = S.oct_word(np.broadcast_to(np.array([0.0, 1.0, 0.0]), (H, W, 3)))
    k = SS.consts(W, H, SS.unit((0.15, 0.9, -0.25)), soft, 5, diameter=3.0, eye=(0.0, 0.6, 1.0))
    noise = SS.noise_image(3)
    gs = GpuScene(dev, sc["instances"], sc["meshData"], sc["meshlets"], sc["opaqueIds"], sc["alphaMaskIds"])
    gs.set_geometry(sc["vertices"], sc["vertexIds"], sc["triangles"])
    gs.set_textures(sc["textures"])
    gs.set_materials(sc["materials"])
    gs.set_raytracing(sc["indices"], sc["index_counts"])
    dev.profile_reset(); dev.profile_enable(True)
    p = P.PenumbraPass(dev, gs, W, H, noise, table=gs.texture_table)
    try:
        got, got_lvd = p.run(k, depth, g)
        names = set(dev.profile())
        assert "shadowmask_CS_ShadowMask#textured_penumbra" in names, names
        want, want_lvd, _ = SG.trace_penumbra(sg, k, acc, depth, g, noise, SG.BRUTE, textures=sc["textures"])
        same(got, want, "textured penumbra")
        same(got_lvd, want_lvd, "linear view depth")
        p.table = None
        dev.profile_reset()
        plain, _ = p.run(k, depth, g)
        assert "shadowmask_CS_ShadowMask#penumbra" in set(dev.profile())
        solid, _, _ = SG.trace_penumbra(sg, k, acc, depth, g, noise, SG.BRUTE)
        same(plain, solid, "penumbra without the table")
        assert 30 < (want < SG.NO_OCCLUDER).sum() < (solid < SG.NO_OCCLUDER).sum() - 30, ((want < SG.NO_OCCLUDER).sum(), (solid < SG.NO_OCCLUDER).sum())
    finally:
        dev.profile_enable(False)
        p.release(); gs.release()


def test_the_pack_pass_on_arbitrary_words(dev, sg):
    """Every texel is written, whatever GBufferA holds: arbitrary words at a size that is no multiple of any tile."""
    W, H = 67, 35
    g = np.random.default_rng(12).integers(0, 1 << 32, (H, W, 4), dtype=np.uint64).astype(np.uint32)
    c = P.Chain(dev, W, H)
    try:
        same(c.pack(g), SG.pack_normal_roughness(sg, g), "normal roughness")
    finally:
        c.release()


# ---- 4. misuse at the back end ------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused(dev, sg):
    """Each refusal happens while the command is recorded, so nothing is launched; a good chain directly behind is correct."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, TEX_SRV, TEX_UAV
    W, H = 33, 18
    s = S.seeded(W, H, 60)
    c = P.Chain(dev, W, H)
    mk = lambda w, h, fmt, name, mips=1: dev.create_texture(w, h, mips, fmt, name)                   # noqa: E731
    other = dict(r16=mk(W, H, rhi.FORMAT_R16_FLOAT, "R16"), r16_small=mk(W - 1, H, rhi.FORMAT_R16_FLOAT, "small R16"), rg16_small=mk(W, H - 1, rhi.FORMAT_RG16_FLOAT, "small RG16"),
                 r8=mk(W, H, rhi.FORMAT_R8_UNORM, "R8"), r8_small=mk(W - 1, H, rhi.FORMAT_R8_UNORM, "small R8"), r32=mk(W, H, rhi.FORMAT_R32_FLOAT, "R32"),
                 tiles_big=mk(4, 2, rhi.FORMAT_R8_UINT, "4x2 tiles"), tiles_unorm=mk(3, 2, rhi.FORMAT_R8_UNORM, "UNORM tiles"), nr_small=mk(W, H + 1, rhi.FORMAT_R10G10B10A2_UNORM, "small NR"),
                 r16_mips=mk(W, H, rhi.FORMAT_R16_FLOAT, "two mips", 2))
    args = dev.create_buffer(12, "args", stride=12, indirect=True)
    cl = dev.create_command_list()
    try:
        dev.profile_reset(); dev.profile_enable(True)
        cl.open()
        cb = cl.constant_buffer(s["k"], "SigmaConsts")
        short = cl.constant_buffer(s["k"].view(np.uint32).reshape(-1)[:27].copy(), "short")
        pass1 = cl.constant_buffer(SG.with_pass(s["k"], 1), "pass 1")
        empty = s["k"].copy(); empty["m_OutputDims"] = (0, H)
        cbe = cl.constant_buffer(empty, "empty")
        pk = np.zeros(1, I.PackNormalAndRoughnessConsts); pk["m_OutputResolution"] = (W, H)

        def swap(b, kind, slot, new):
            return [x for x in b if not (x.type == kind and x.slot == slot)] + ([new] if new is not None else [])
        S_, U_ = rhi.BIND_TEXTURE_SRV, rhi.BIND_TEXTURE_UAV
        cls, blr, stb = [CB(0, cb)] + c.classify_bindings(), [CB(0, cb)] + c.blur_bindings(0, 1), [CB(0, cb)] + c.stabilize_bindings()
        g8, g16 = c.groups(8), c.groups(16)
        bad = [(P.CLASSIFY, "112 bytes", cls[1:], g16), (P.CLASSIFY, "112 bytes", [CB(0, short)] + cls[1:], g16), (P.CLASSIFY, "is empty", [CB(0, cbe)] + cls[1:], g16),
               (P.CLASSIFY, "covering 33x18", cls, (2, 2, 1)), (P.CLASSIFY, "covering 33x18", cls, (3, 1, 1)),
               (P.CLASSIFY, "penumbra", swap(cls, S_, 0, None), g16), (P.CLASSIFY, "penumbra", swap(cls, S_, 0, TEX_SRV(0, other["r8"])), g16),
               (P.CLASSIFY, "is 32x18", swap(cls, S_, 0, TEX_SRV(0, other["r16_small"])), g16), (P.CLASSIFY, "linear view depth", swap(cls, S_, 1, TEX_SRV(1, other["r32"])), g16),
               (P.CLASSIFY, "tile texture", swap(cls, U_, 0, None), g16), (P.CLASSIFY, "tile texture", swap(cls, U_, 0, TEX_UAV(0, other["tiles_unorm"], 0)), g16),
               (P.CLASSIFY, "is 4x2", swap(cls, U_, 0, TEX_UAV(0, other["tiles_big"], 0)), g16), (P.CLASSIFY, "shadow data", swap(cls, U_, 1, TEX_UAV(1, other["r16"], 0)), g16),
               (P.CLASSIFY, "is 33x17", swap(cls, U_, 1, TEX_UAV(1, other["rg16_small"], 0)), g16),
               (P.BLUR, "m_Pass is 1", [CB(0, pass1)] + blr[1:], g8), (P.POST_BLUR, "m_Pass is 0", blr, g8), (P.BLUR, "covering 33x18", blr, (4, 3, 1)),
               (P.BLUR, "shadow data to read", swap(blr, S_, 0, TEX_SRV(0, other["r16"])), g8), (P.BLUR, "same texture", swap(blr, S_, 0, TEX_SRV(0, c.data[1])), g8),
               (P.BLUR, "R32_FLOAT depth", swap(blr, S_, 2, TEX_SRV(2, c.lvd)), g8), (P.BLUR, "normal roughness", swap(blr, S_, 3, TEX_SRV(3, other["r32"])), g8),
               (P.BLUR, "is 33x19", swap(blr, S_, 3, TEX_SRV(3, other["nr_small"])), g8), (P.BLUR, "is 4x2", swap(blr, S_, 4, TEX_SRV(4, other["tiles_big"])), g8),
               (P.BLUR, "tile texture", swap(blr, S_, 4, None), g8), (P.BLUR, "shadow data to write", swap(blr, U_, 0, None), g8),
               (P.STABILIZE, "same texture", swap(stb, S_, 3, TEX_SRV(3, c.history[1])), g8), (P.STABILIZE, "previous shadow history", swap(stb, S_, 3, TEX_SRV(3, other["r8"])), g8),
               (P.STABILIZE, "previous shadow history", swap(stb, S_, 3, TEX_SRV(3, other["r16_mips"])), g8), (P.STABILIZE, "as a history too", swap(stb, S_, 3, TEX_SRV(3, c.lvd)), g8),
               (P.STABILIZE, "motion target", swap(stb, S_, 2, TEX_SRV(2, other["r16"])), g8), (P.STABILIZE, "new shadow history", swap(stb, U_, 0, TEX_UAV(0, other["r8"], 0)), g8),
               (P.STABILIZE, "shadow mask", swap(stb, U_, 1, TEX_UAV(1, other["r16"], 0)), g8), (P.STABILIZE, "is 32x18", swap(stb, U_, 1, TEX_UAV(1, other["r8_small"], 0)), g8),
               (P.STABILIZE, "is 4x2", swap(stb, S_, 4, TEX_SRV(4, other["tiles_big"])), g8), (P.STABILIZE, "covering 33x18", stb, (5, 2, 1))]
        for name, match, bindings, groups in bad:
            with pytest.raises(rhi.TrhipError, match=match):
                cl.dispatch(name, bindings, groups)
        for name, bindings in ((P.CLASSIFY, cls), (P.BLUR, blr), (P.POST_BLUR, [CB(0, pass1)] + blr[1:]), (P.STABILIZE, stb)):
            with pytest.raises(rhi.TrhipError, match="direct dispatch"):
                cl.dispatch_indirect(name, bindings, args)
        pack = c.pack_bindings()
        for match, bindings, groups, push in (("8 bytes", pack, g8, None), ("8 bytes", pack, g8, np.zeros(1, np.uint32)), ("covering 33x18", pack, (4, 3, 1), pk),
                                              ("GBufferA", swap(pack, S_, 2, TEX_SRV(2, other["r32"])), g8, pk), ("normal roughness", swap(pack, U_, 0, TEX_UAV(0, other["r32"], 0)), g8, pk),
                                              ("is 33x19", swap(pack, U_, 0, TEX_UAV(0, other["nr_small"], 0)), g8, pk)):
            with pytest.raises(rhi.TrhipError, match=match):
                cl.dispatch(P.PACK, bindings, groups, push=push)
        with pytest.raises(rhi.TrhipError, match="direct dispatch"):
            cl.dispatch_indirect(P.PACK, pack, args, push=pk)
        cl.close()
        dev.execute(cl); dev.wait_idle()
        assert not any(n.startswith(("SIGMA_", "shadowmask_")) for n in dev.profile()), dev.profile()       # nothing was launched
        dev.profile_enable(False)
        want, got = S.run(sg, s), c.run(s)
        for key in OUTPUTS:
            same(got[key], want[key], f"a good chain after the refusals: {key}")
    finally:
        dev.profile_enable(False)
        cl.release(); args.release(); c.release()
        for t in other.values():
            t.release()


def test_the_penumbra_trace_refuses_the_mask_at_u0_and_one_texture_twice(dev):
    """m_bDoDenoising = 1 with the R8_UNORM mask at u0 is refused in words that name the flag; m_bDoDenoising = 0 with an R16_FLOAT
    texture there asks for the mask; the linear view depth at both u0 and u1 is refused."""
    from shadow_passes import TRACE
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import TEX_UAV
    W, H = 32, 16
    sc = SS.scattered(8)
    gs = bare_gpu_scene(dev, sc)
    p = P.PenumbraPass(dev, gs, W, H, SS.noise_image())
    r8 = dev.create_texture(W, H, 1, rhi.FORMAT_R8_UNORM, "Shadow Mask Texture")
    cl = dev.create_command_list()
    k = SS.consts(W, H, SS.LIGHTS["generic"], True, 0)
    on = k.copy(); on["m_bDoDenoising"] = 1
    try:
        cl.open()
        cb0, cb1 = cl.constant_buffer(k, "off"), cl.constant_buffer(on, "on")
        good = p.p.trace_bindings(cb1)
        u0 = lambda b, t: [x for x in b if not (x.type == rhi.BIND_TEXTURE_UAV and x.slot == 0)] + [TEX_UAV(0, t, 0)]      # noqa: E731
        with pytest.raises(rhi.TrhipError, match="m_bDoDenoising"):
            cl.dispatch(TRACE, u0(good, r8), p.p.groups())
        with pytest.raises(rhi.TrhipError, match="R8_UNORM shadow mask"):
            cl.dispatch(TRACE, p.p.trace_bindings(cb0), p.p.groups())
        with pytest.raises(rhi.TrhipError, match="same texture"):
            cl.dispatch(TRACE, u0(good, p.p.lvd), p.p.groups())
        cl.close()
    finally:
        cl.release(); r8.release(); p.release(); gs.release()


# ---- 5. frames through FrameDriver ----------------------------------------------------------------------------------------------------------------
LIGHT = SS.unit((0.25, 0.45, 0.9))                  # through the Cornell box's open side
SHADOWS = dict(ray_start_offset=0.01, soft=True, sun_angular_diameter=6.0)


class Cornell:
    """The lit Cornell fixture with its acceleration structure on the device (tests/test_gpu_shadowmask.py's), under the camera path
    of the temporal anti-aliasing tests (tests/taa_scenes.py)."""

    def __init__(self, dev, oracle):
        self.sc = sc = SS.cornell()
        s = sc["loaded"]
        inst = sc["instances"].copy()
        oracle.update_instance_consts(s.nodes, s.primToNode, inst)
        inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
        sc["instances"] = inst
        s.meshData = sc["meshData"]
        self.gs = gpu_scene(dev, s, inst, s.vertices, sc["materials"])
        self.gs.set_raytracing(sc["indices"], sc["cached"].meshSpecific)
        self.acc = SR.Accel(sc)
        self.camera = sc["camera"]
        self.noise = SS.noise_image(4)

    def driver(self, dev, taa=False, **kw):
        from toyrenderer_amd.frame import FrameDriver
        eye, _ = TS.camera_at(self.camera, 0)
        if "shadows" not in kw:
            kw["shadows"] = dict(SHADOWS, noise=self.noise)
        more = dict(post=True, taa=dict(TS.SETTINGS)) if taa else dict(lighting=True)
        return FrameDriver(dev, self.gs, TS.view_at(self.camera, 0), record_capacity=4096, culling_flags=7, dir_light=(LIGHT, 3.0), camera_origin=eye, **more, **kw)

    def frame(self, drv, f):
        """Record and run frame f of the camera path, the frame's targets pre-filled."""
        eye, _ = TS.camera_at(self.camera, f)
        drv.view, drv.camera_origin, drv.frame_counter = TS.view_at(self.camera, f), eye, f
        H, W = drv.view.renderH, drv.view.renderW
        drv.shadow_mask_texture.upload_mip(0, np.full((H, W), SG.SENTINEL8, np.uint8))
        drv.linear_view_depth.upload_mip(0, np.full((H, W), SG.SENTINEL16, np.uint16))
        if drv.shadow_denoise is not None:
            drv.shadow_penumbra.upload_mip(0, np.full((H, W), SG.SENTINEL16, np.uint16))
            drv.shadow_history[1 - drv.shadow_history_written].upload_mip(0, np.full((H, W), SG.SENTINEL16, np.uint16))
            drv.shadow_tiles.upload_mip(0, np.full(accel.sigma_tiles(W, H)[::-1], SG.SENTINEL8, np.uint8))
        drv.record(); drv.run(); drv.results()
        return eye

    def reference(self, sg, drv, eye, f, history, reset):
        """The reference chain of the frame the driver just ran, from the depth, GBufferA and motion it left: (penumbra, linear view
        depth, sigma_ref.denoise's dict)."""
        view = drv.taa_view if drv.taa is not None else drv.view
        W, H = view.renderW, view.renderH
        depth, g, motion = drv.depth.download_mip(0), drv.gbufferA.download_mip(0), P.rg16_words(drv.motion.download_mip(0))
        c2w = I.clip_to_world(view.worldToView, view.viewToClip)
        k = accel.shadow_consts(c2w, LIGHT, eye, W, H, drv.shadows, f, denoise=True)
        assert drv.shadow_consts.tobytes() == k.tobytes()
        pen, lvd, _ = SG.trace_penumbra(sg, k, self.acc, depth, g, self.noise, SG.BRUTE, instances=self.sc["instances"])
        delta = tuple(drv.taa_consts["m_JitterDelta"][0]) if drv.taa is not None else (0.0, 0.0)
        sk = accel.sigma_consts(c2w, view.viewToClip, W, H, drv.shadow_denoise, f, 0, reset, delta)
        assert drv.sigma_consts.tobytes() == sk.tobytes()
        return pen, lvd, SG.denoise(sg, sk, pen, lvd, depth, g, motion, history), depth, g


@pytest.mark.parametrize("taa", [False, True], ids=["no taa", "taa"])
def test_five_frames_equal_the_reference_chain(dev, oracle, sg, lr, taa):
    """FrameDriver(shadows=..., shadow_denoise={}) on the lit Cornell box under the moving camera of the TAA tests: penumbra, linear
    view depth, tiles, history, mask and LightingOutput of every frame equal the reference chain with the history carried; the
    history is valid from the second frame on, and the mask differs from the raw one."""
    c = Cornell(dev, oracle)
    drv = c.driver(dev, taa, shadow_denoise={})
    W, H = TS.RENDER
    history = np.zeros((H, W), np.uint16)
    try:
        for f in range(5):
            eye = c.frame(drv, f)
            what = f"frame {f}"
            pen, lvd, r, depth, g = c.reference(sg, drv, eye, f, history, f == 0)
            same(drv.download_shadow_penumbra(), pen, what + ": penumbra")
            same(drv.linear_view_depth.download_mip(0), lvd, what + ": linear view depth")
            same(drv.download_shadow_tiles(), r["tiles"], what + ": tiles")
            same(drv.download_shadow_history(), r["history"], what + ": history")
            same(drv.download_shadow_mask(), r["mask"], what + ": mask")
            same(drv.lighting_output.download_mip(0), LR.lighting(lr, drv.lighting_consts, g, depth, shadow=r["mask"], motion=drv.motion.download_mip(0)), what + ": LightingOutput")
            assert int(drv.sigma_consts["m_bResetHistory"][0]) == int(f == 0) and int(drv.sigma_consts["m_FrameIndex"][0]) == f
            assert ((r["path"] & SG.PATH_HISTORY) != 0).sum() > (200 if f else -1) and (f > 0 or r["reads"] == 0), what
            raw = np.where(pen < SG.NO_OCCLUDER, 0, 255)
            assert np.count_nonzero((r["mask"] != raw) & (depth != 0)) > 100 and np.any(pen < SG.NO_OCCLUDER) and np.any(pen == SG.NO_OCCLUDER), what
            history = r["history"]
    finally:
        drv.release(); c.gs.release()


def test_a_reset_mid_run(dev, oracle, sg):
    """reset_shadow_history() before frame 2: that frame runs with m_bResetHistory = 1 and equals the chain that reads no history."""
    c = Cornell(dev, oracle)
    drv = c.driver(dev, shadow_denoise=dict(sigma_scale=1.5, stabilization_strength=0.75))
    history = np.zeros(TS.RENDER[::-1], np.uint16)
    try:
        for f in range(4):
            if f == 2:
                drv.reset_shadow_history()
            eye = c.frame(drv, f)
            reset = f in (0, 2)
            assert int(drv.sigma_consts["m_bResetHistory"][0]) == int(reset) and drv.sigma_consts["m_SigmaScale"][0] == 1.5
            _, _, r, _, _ = c.reference(sg, drv, eye, f, history, reset)
            assert (r["reads"] == 0) == reset
            same(drv.download_shadow_history(), r["history"], f"frame {f}: history")
            same(drv.download_shadow_mask(), r["mask"], f"frame {f}: mask")
            history = r["history"]
    finally:
        drv.release(); c.gs.release()


def test_denoising_adds_five_dispatches_behind_the_trace(dev, oracle):
    """shadow_denoise=None records what a shadows=... driver records today, command for command and launch for launch;
    shadow_denoise=... adds exactly five dispatches between the trace and the lighting dispatch and turns the trace into its
    penumbra instantiation."""
    c = Cornell(dev, oracle)
    seen, counts, kinds = {}, {}, {}
    try:
        for name, extra in (("today", {}), ("none", dict(shadow_denoise=None)), ("on", dict(shadow_denoise={}))):
            drv = c.driver(dev, **extra)
            try:
                counts[name], seen[name], kinds[name] = op_counts(dev, drv), recorded(drv), recorded_kinds(drv)
                if name != "on":
                    assert drv.shadow_denoise is None and drv.shadow_penumbra is None and drv.shadow_history is None and drv.sigma_consts is None
                    for call in (drv.reset_shadow_history, drv.download_shadow_penumbra, drv.download_shadow_tiles, drv.download_shadow_history):
                        with pytest.raises(ValueError, match="shadow_denoise=None"):
                            call()
            finally:
                drv.release()
    finally:
        c.gs.release()
    assert seen["none"] == seen["today"] and counts["none"] == counts["today"] and kinds["none"] == kinds["today"]
    at = seen["today"].index(("dispatch", TRACE))
    assert seen["today"][at - 1] == ("dispatch", REFIT) and seen["today"][at + 1] == ("dispatch", "deferredlighting_PS_Main")
    assert seen["on"] == seen["today"][:at + 1] + [("dispatch", n) for n in P.ENTRIES] + seen["today"][at + 1:]
    assert kinds["on"] == {**kinds["today"], "dispatch": kinds["today"]["dispatch"] + 5, "constant_buffer": kinds["today"]["constant_buffer"] + 2}
    want = {k: v for k, v in counts["today"].items() if k != TRACE + "#main"}
    assert counts["on"] == {**want, TRACE + "#penumbra": 1, **{n + "#main": 1 for n in P.ENTRIES}}


def test_misuse_at_the_driver(dev, oracle):
    from toyrenderer_amd.frame import FrameDriver
    c = Cornell(dev, oracle)
    view = TS.view_at(c.camera, 0)
    try:
        with pytest.raises(ValueError, match="needs shadows="):
            FrameDriver(dev, c.gs, view, record_capacity=4096, lighting=True, shadow_denoise={})
        for bad, match in ((dict(strength=1.0), "unknown setting"), (dict(sigma_scale=-1.0), "sigma_scale"), (dict(stabilization_strength=2.0), "stabilization_strength"),
                           (dict(plane_distance_sensitivity=0.0), "plane_distance_sensitivity"), (True, "dict")):
            with pytest.raises(ValueError, match=match):
                c.driver(dev, shadow_denoise=bad)
    finally:
        c.gs.release()


# ---- 6. the host mirror ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taa", [False, True], ids=["no taa", "taa"])
def test_host_path_over_five_frames(oracle, sg, tmp_path, taa):
    """The C++ host mirror on the generated city with a moving camera, five frames, a reset before the fourth: trhost_get_sigma_consts
    equals the Python block byte for byte, and the penumbra, the tiles, the history and the mask equal the reference chain fed the
    frame's own depth, GBufferA and motion with the history carried.  Then the facade's refusals."""
    from gbuffer_scenes import with_normals_and_materials
    from toyrenderer_amd import cached_scene, host, synth
    from visibility_scenes import city
    s, sc0 = city(tmp_path, oracle, lods=False)
    v, sc0, mats = with_normals_and_materials(s, sc0)
    c = cached_scene.from_scene(s)
    cam = s.cameras[0]
    W, H = render = (48, 27)
    Pm = synth.perspective_rh_reverse_z_infinite(cam.yfov, W / H, cam.znear)
    inst_in = s.instances.copy()
    inst_in["m_MaterialDataIdx"] = sc0["instances"]["m_MaterialDataIdx"]
    sc = dict(vertices=v, indices=c.indices, meshData=c.meshData, index_counts=c.meshSpecific["m_NumIndices"], instances=sc0["instances"], opaqueIds=s.opaqueIds,
              alphaMaskIds=s.alphaMaskIds, materials=mats)
    acc = SR.Accel(sc)
    noise = SS.noise_image(2)
    light = SS.unit((0.2, 0.35, -0.9))
    setting = dict(soft=True, sun_angular_diameter=8.0, ray_start_offset=0.1)
    denoise = dict(plane_distance_sensitivity=0.03, stabilization_strength=0.75, sigma_scale=1.5)
    r = host.Renderer(render=render, max_groups=4096)
    try:
        r.load_scene(inst_in, c.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
        r.load_nodes(s.nodes, s.primToNode)
        r.load_geometry(v, s.meshletVertexIds, s.meshletTriangles)
        r.load_materials(mats)
        r.set_deferred_lighting(True)
        r.load_raytracing(c.indices, c.meshSpecific)
        r.upload_blue_noise(noise)
        with pytest.raises(host.HostError, match="shadow mask is off"):
            r.set_shadow_denoising(True)
        with pytest.raises(host.HostError, match="denoising is off"):
            r.reset_shadow_history()
        r.set_shadow_mask(True, **setting)
        with pytest.raises(host.HostError, match="denoising is off"):
            r.reset_shadow_history()
        for bad, match in ((dict(plane_distance_sensitivity=0.0), "sensitivity"), (dict(plane_distance_sensitivity=float("nan")), "sensitivity"),
                           (dict(stabilization_strength=1.5), "strength"), (dict(stabilization_strength=float("nan")), "strength"), (dict(sigma_scale=-1.0), "sigma scale"),
                           (dict(sigma_scale=float("inf")), "sigma scale")):
            with pytest.raises(host.HostError, match=match):
                r.set_shadow_denoising(True, **bad)
        for call in (r.sigma_consts, r.download_shadow_penumbra, r.download_shadow_tiles, r.download_shadow_history):
            with pytest.raises(host.HostError, match="did not run"):
                call()
        r.set_shadow_denoising(True, **denoise)
        if taa:
            r.set_post_process(True)
            r.set_taa(True)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        prevV = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
        history = np.zeros((H, W), np.uint16)
        settings = accel.check_denoise_settings(denoise)
        for f in range(5):
            V = synth.world_to_view((0.1 * f, 0.02 * f, -0.15 * f), cam.orientation)
            r.set_camera(synth.View(V, prevV, Pm, float(np.float32(cam.znear)), *render))
            prevV = V
            r.set_directional_light(light, 2.0)
            if f == 3:
                r.reset_shadow_history()
            r.frame()
            r.results()
            reset = f in (0, 3)
            k = r.shadow_mask_consts()
            assert k["m_bDoDenoising"][0] == 1
            delta = tuple(r.taa_consts()[0]["m_JitterDelta"][0]) if taa else (0.0, 0.0)
            got_k = r.sigma_consts()
            want_k = accel.sigma_consts(k["m_ClipToWorld"][0], Pm, W, H, settings, f + 1, 0, reset, delta)     # the frame is counted before it is recorded
            assert got_k.tobytes() == want_k.tobytes(), (f, got_k, want_k)
            if not taa:
                assert np.array_equal(k["m_ClipToWorld"][0], I.clip_to_world(V, Pm))
            depth, g, motion = r.download_depth(), r.download_gbuffer_a(), P.rg16_words(r.download_motion())
            pen, lvd, _ = SG.trace_penumbra(sg, k, acc, depth, g, noise, SG.BRUTE, penumbra=r.download_shadow_penumbra())     # far texels keep what the texture held
            same(r.download_shadow_penumbra(), pen, f"frame {f}: penumbra")
            want = SG.denoise(sg, want_k, pen, lvd, depth, g, motion, history)
            same(r.download_shadow_tiles(), want["tiles"], f"frame {f}: tiles")
            same(r.download_shadow_history(), want["history"], f"frame {f}: history")
            same(r.download_shadow_mask(), want["mask"], f"frame {f}: mask")
            assert (want["reads"] == 0) == reset, f
            assert (want["path"] & SG.PATH_FILTERED).any() and np.any(pen < SG.NO_OCCLUDER) and np.any(pen == SG.NO_OCCLUDER), f
            history = want["history"]
        r.set_shadow_denoising(False)
        r.frame(); r.results()
        assert r.shadow_mask_consts()["m_bDoDenoising"][0] == 0 and set(np.unique(r.download_shadow_mask()[r.download_depth() != 0]).tolist()) <= {0, 255}
        for call in (r.sigma_consts, r.download_shadow_penumbra, r.download_shadow_history):
            with pytest.raises(host.HostError, match="did not run"):
                call()
        r.set_shadow_denoising(True)
        r.set_shadow_mask(False)                                                  # switches the denoiser off with it
        with pytest.raises(host.HostError, match="shadow mask is off"):
            r.set_shadow_denoising(True)
    finally:
        r.shutdown()
