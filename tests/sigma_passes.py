"""What the shadow denoiser's GPU tests share (tests/test_gpu_sigma.py): the textures of one size and each pass of the chain as one
direct dispatch through rhi bindings, every target pre-filled with a sentinel.  Not a test module."""
import numpy as np

import sigma_ref as SG
from suite_support import halves_to_words
from toyrenderer_amd import accel
from toyrenderer_amd import interop as I

F = np.float32
PACK, CLASSIFY, BLUR, POST_BLUR, STABILIZE = ("shadowmask_CS_PackNormalAndRoughness", "SIGMA_Shadow_ClassifyTiles.cs", "SIGMA_Shadow_Blur.cs", "SIGMA_Shadow_PostBlur.cs",
                                              "SIGMA_Shadow_TemporalStabilization.cs")
ENTRIES = (PACK, CLASSIFY, BLUR, POST_BLUR, STABILIZE)


def rg16(words):
    """uint32 words (x in the low half) as the float16 [H, W, 2] an RG16_FLOAT texture uploads, bit for bit."""
    w = np.ascontiguousarray(words, np.uint32)
    return w.view(np.uint16).reshape(*w.shape, 2).view(np.float16)


def rg16_words(halves):
    return halves_to_words(np.ascontiguousarray(halves).view(np.uint16))


class Chain:
    """The denoiser's textures at W x H and its five entries, one dispatch each."""

    def __init__(self, dev, W, H):
        from toyrenderer_amd import rhi
        self.dev, self.W, self.H = dev, W, H
        tw, th = accel.sigma_tiles(W, H)
        mk = lambda w, h, fmt, name, **kw: dev.create_texture(w, h, 1, fmt, name, **kw)               # noqa: E731
        self.gbuffer = mk(W, H, rhi.FORMAT_RGBA32_UINT, "GBufferA")
        self.depth = mk(W, H, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
        self.penumbra = mk(W, H, rhi.FORMAT_R16_FLOAT, "Shadow Penumbra Texture")
        self.lvd = mk(W, H, rhi.FORMAT_R16_FLOAT, "Linear View Depth")
        self.normal_roughness = mk(W, H, rhi.FORMAT_R10G10B10A2_UNORM, "Normal Roughness Texture")
        self.tiles = mk(tw, th, rhi.FORMAT_R8_UINT, "Shadow Tiles")
        self.data = [mk(W, H, rhi.FORMAT_RG16_FLOAT, f"Shadow Data {i}") for i in range(2)]
        self.motion = mk(W, H, rhi.FORMAT_RG16_FLOAT, "GBufferMotion")
        self.history = [mk(W, H, rhi.FORMAT_R16_FLOAT, f"Shadow History {i}") for i in range(2)]
        self.mask = mk(W, H, rhi.FORMAT_R8_UNORM, "Shadow Mask Texture")
        self.cl = dev.create_command_list()

    def textures(self):
        return [self.gbuffer, self.depth, self.penumbra, self.lvd, self.normal_roughness, self.tiles, *self.data, self.motion, *self.history, self.mask]

    def groups(self, side=8):
        return ((self.W + side - 1) // side, (self.H + side - 1) // side, 1)

    def dispatch(self, name, bindings, groups, consts=None, push=None):
        """One dispatch in a command list of its own; consts: bound as the constant buffer b0."""
        from toyrenderer_amd.rhi import CB
        self.cl.open()
        if consts is not None:
            bindings = [CB(0, self.cl.constant_buffer(consts, "consts"))] + bindings
        self.cl.dispatch(name, bindings, groups, push=push)
        self.cl.close()
        self.dev.execute(self.cl); self.dev.wait_idle()

    # ---- the bindings of each entry --------------------------------------------------------------------------------------------------
    def pack_bindings(self):
        from toyrenderer_amd.rhi import PUSH, TEX_SRV, TEX_UAV
        return [PUSH(0), TEX_SRV(2, self.gbuffer), TEX_UAV(0, self.normal_roughness, 0)]

    def classify_bindings(self):
        from toyrenderer_amd.rhi import TEX_SRV, TEX_UAV
        return [TEX_SRV(0, self.penumbra), TEX_SRV(1, self.lvd), TEX_UAV(0, self.tiles, 0), TEX_UAV(1, self.data[0], 0)]

    def blur_bindings(self, src, dst):
        from toyrenderer_amd.rhi import TEX_SRV, TEX_UAV
        return [TEX_SRV(0, self.data[src]), TEX_SRV(1, self.lvd), TEX_SRV(2, self.depth), TEX_SRV(3, self.normal_roughness), TEX_SRV(4, self.tiles), TEX_UAV(0, self.data[dst], 0)]

    def stabilize_bindings(self, src=0, dst=1):
        from toyrenderer_amd.rhi import TEX_SRV, TEX_UAV
        return [TEX_SRV(0, self.data[0]), TEX_SRV(1, self.lvd), TEX_SRV(2, self.motion), TEX_SRV(3, self.history[src]), TEX_SRV(4, self.tiles),
                TEX_UAV(0, self.history[dst], 0), TEX_UAV(1, self.mask, 0)]

    # ---- the passes, each on uploaded inputs -----------------------------------------------------------------------------------------
    def pack(self, g):
        self.gbuffer.upload_mip(0, np.ascontiguousarray(g, np.uint32))
        self.normal_roughness.upload_mip(0, np.full((self.H, self.W), SG.SENTINEL32, np.uint32))
        k = np.zeros(1, I.PackNormalAndRoughnessConsts)
        k["m_OutputResolution"] = (self.W, self.H)
        self.dispatch(PACK, self.pack_bindings(), self.groups(), push=k)
        return self.normal_roughness.download_mip(0)

    def classify(self, k, penumbra, lvd):
        tw, th = accel.sigma_tiles(self.W, self.H)
        self.penumbra.upload_mip(0, penumbra); self.lvd.upload_mip(0, lvd)
        self.tiles.upload_mip(0, np.full((th, tw), SG.SENTINEL8, np.uint8))
        self.data[0].upload_mip(0, rg16(np.full((self.H, self.W), SG.SENTINEL32, np.uint32)))
        self.dispatch(CLASSIFY, self.classify_bindings(), self.groups(16), consts=k)
        return self.tiles.download_mip(0), rg16_words(self.data[0].download_mip(0))

    def blur(self, k, pass_index, data, lvd, depth, normal_roughness, tiles):
        src, dst = pass_index, 1 - pass_index
        self.data[src].upload_mip(0, rg16(data)); self.lvd.upload_mip(0, lvd); self.depth.upload_mip(0, np.ascontiguousarray(depth, F))
        self.normal_roughness.upload_mip(0, normal_roughness); self.tiles.upload_mip(0, tiles)
        self.data[dst].upload_mip(0, rg16(np.full((self.H, self.W), SG.SENTINEL32, np.uint32)))
        self.dispatch(POST_BLUR if pass_index else BLUR, self.blur_bindings(src, dst), self.groups(), consts=SG.with_pass(k, pass_index))
        return rg16_words(self.data[dst].download_mip(0))

    def stabilize(self, k, data, lvd, motion, history, tiles):
        self.data[0].upload_mip(0, rg16(data)); self.lvd.upload_mip(0, lvd); self.motion.upload_mip(0, rg16(motion)); self.history[0].upload_mip(0, history)
        self.tiles.upload_mip(0, tiles)
        self.history[1].upload_mip(0, np.full((self.H, self.W), SG.SENTINEL16, np.uint16))
        self.mask.upload_mip(0, np.full((self.H, self.W), SG.SENTINEL8, np.uint8))
        self.dispatch(STABILIZE, self.stabilize_bindings(), self.groups(), consts=k)
        return self.history[1].download_mip(0), self.mask.download_mip(0)

    def run(self, s):
        """The chain on one input of tests/sigma_scenes.py, each pass fed what the pass before it left on the GPU: the dict of
        sigma_ref.denoise (without path and reads)."""
        nr = self.pack(s["g"])
        tiles, data0 = self.classify(s["k"], s["penumbra"], s["lvd"])
        data1 = self.blur(s["k"], 0, data0, s["lvd"], s["depth"], nr, tiles)
        data2 = self.blur(s["k"], 1, data1, s["lvd"], s["depth"], nr, tiles)
        history, mask = self.stabilize(s["k"], data2, s["lvd"], s["motion"], s["history"], tiles)
        return dict(normal_roughness=nr, tiles=tiles, data0=data0, data1=data1, data2=data2, history=history, mask=mask)

    def release(self):
        self.cl.release()
        for t in self.textures():
            t.release()


class PenumbraPass:
    """tests/shadow_passes.py's Pass with the R16_FLOAT penumbra texture at u0: the trace with m_bDoDenoising = 1.  table: a
    rhi.TextureTable bound at t19 (the textured instantiation)."""

    def __init__(self, dev, gs, W, H, noise, table=None):
        from shadow_passes import Pass
        from toyrenderer_amd import rhi
        self.p = Pass(dev, gs, W, H, noise)
        self.p.mask.release()
        self.p.mask = dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, "Shadow Penumbra Texture")
        self.table = table

    def run(self, k, depth, g):
        """(penumbra words, linear view depth words); k: ShadowMaskConsts, its m_bDoDenoising set here."""
        from shadow_passes import REFIT, TRACE
        from toyrenderer_amd.rhi import TEX_TABLE
        p = self.p
        k = np.ascontiguousarray(k, I.ShadowMaskConsts).copy()
        k["m_bDoDenoising"] = 1
        p.depth.upload_mip(0, np.ascontiguousarray(depth, F))
        p.gbuffer.upload_mip(0, np.ascontiguousarray(g, np.uint32))
        p.mask.upload_mip(0, np.full((p.H, p.W), SG.SENTINEL16, np.uint16))
        p.lvd.upload_mip(0, np.full((p.H, p.W), SG.SENTINEL16, np.uint16))
        p.cl.open()
        p.cl.dispatch(REFIT, p.refit_bindings(), ((p.gs.numInstances + 63) // 64, 1, 1), push=p.refit_push())
        cb = p.cl.constant_buffer(k, "ShadowMaskConsts")
        p.cl.dispatch(TRACE, p.trace_bindings(cb) + ([TEX_TABLE(self.table)] if self.table is not None else []), p.groups())
        p.cl.close()
        p.dev.execute(p.cl); p.dev.wait_idle()
        return p.mask.download_mip(0), p.lvd.download_mip(0)

    def release(self):
        self.p.release()
