"""The frame's tail as FrameDriver records it: BloomRenderer's mip chain, AdaptLuminanceRenderer's exposure and PostProcessRenderer's
tone map into the back buffer (csrc/k_bloom.hip, csrc/k_adaptluminance.hip, csrc/k_postprocess.hip)."""
import numpy as np

from . import interop as I
from . import rhi
from .rhi import PUSH, SAMPLER, SRV, TEX_SRV, TEX_UAV, UAV


class BloomPass:
    """bloom_mips: 0 (the default) changes nothing.  >= 2 (needs post=True, and no external bloom texture): BloomRenderer
    (BloomRenderer.cpp; the reference's defaults are 6 mips, radius 0.005, strength 0.1).  The driver owns self.bloom_texture,
    an R11G11B10_FLOAT render target with that many mips; after the lighting dispatch and before the histogram clear it
    records bloom_mips - 1 "bloom_PS_Downsample" dispatches (pass i reads mip i, LightingOutput for i = 0, and writes mip
    i + 1) and bloom_mips - 1 "bloom_PS_Upsample" dispatches (each overwrites the next finer mip) and binds the texture,
    read at mip 0, as the post pass's t2 with bloom_strength.  bloom_filter_radius: m_FilterRadius, in UV.  The count may
    not exceed floor(log2(min(W, H))) + 1: every mip has at least one texel in both axes (the reference's slider allows
    W >> k = 0; this project does not).  self.bloom_consts holds the BloomConsts of the last record(), downsamples first;
    download_bloom(mip) reads a mip back."""
    bloom_mips, bloom_texture, bloom_consts = 0, None, None

    def _check_bloom(self, bloom_mips, bloom_filter_radius, bloom_strength, bloom, post):
        self.bloom_mips = int(bloom_mips)
        if self.bloom_mips != 0:
            W, H = self.view.renderW, self.view.renderH
            most = int(min(W, H)).bit_length()                                           # floor(log2(min(W, H))) + 1
            if self.bloom_mips < 2:
                raise ValueError(f"bloom_mips = {self.bloom_mips}: the chain needs at least 2 mips (0 turns bloom generation off)")
            if self.bloom_mips > most:
                raise ValueError(f"bloom_mips = {self.bloom_mips}: a {W}x{H} image has at most {most} mips with a texel in both axes")
            if not post:
                raise ValueError("bloom_mips > 0 needs post=True: the post pass is what reads the bloom texture")
            if bloom[0] is not None:
                raise ValueError("bloom_mips > 0 together with an external bloom=(texture, strength): the driver generates the texture itself")
            if not (np.isfinite(bloom_filter_radius) and bloom_filter_radius >= 0.0):
                raise ValueError(f"bloom_filter_radius = {bloom_filter_radius}: needs a finite radius >= 0")
            self.bloom_strength = np.float32(bloom_strength)
        self.bloom_filter_radius = np.float32(bloom_filter_radius)

    def _create_bloom(self):                         # BloomRenderer::Setup (BloomRenderer.cpp:41-50)
        if self.bloom_mips:
            self.bloom_texture = self._own(self.dev.create_texture(self.view.renderW, self.view.renderH, self.bloom_mips, rhi.FORMAT_R11G11B10_FLOAT, "Bloom Texture",
                                                                   render_target=True))

    # ---- BloomRenderer::Render (BloomRenderer.cpp:57-141) ---------------------------------------------------------------
    def _bloom(self, cl):
        v, tex, n = self.view, self.bloom_texture, self.bloom_mips - 1
        self.bloom_consts = np.zeros(2 * n, I.BloomConsts)

        def groups(mip):
            return I.groups8(v.renderW >> mip, v.renderH >> mip)
        for i in range(n):                                                               # downsample: mip i -> mip i + 1
            k = self.bloom_consts[i:i + 1]
            k["m_bIsFirstDownsample"] = int(i == 0)
            k["m_InvSourceResolution"] = (np.float32(1.0) / np.float32(v.renderW >> i), np.float32(1.0) / np.float32(v.renderH >> i))
            src = TEX_SRV(0, self.lighting_output) if i == 0 else TEX_SRV(0, tex, i)
            cl.dispatch("bloom_PS_Downsample", [PUSH(0), src, TEX_UAV(0, tex, i + 1), SAMPLER(0)], groups(i + 1), push=k)
        for i in range(n):                                                               # upsample: mip n - i -> mip n - i - 1, overwritten
            k = self.bloom_consts[n + i:n + i + 1]
            k["m_FilterRadius"] = self.bloom_filter_radius
            cl.dispatch("bloom_PS_Upsample", [PUSH(0), TEX_SRV(0, tex, n - i), TEX_UAV(0, tex, n - i - 1), SAMPLER(0)], groups(n - i - 1), push=k)

    def download_bloom(self, mip: int = 0) -> np.ndarray:
        """The words of one mip of the generated bloom texture, (H >> mip, W >> mip) uint32."""
        return self._download("download_bloom", self.bloom_texture, "bloom generation is off (bloom_mips = 0)", lambda: self.bloom_texture.download_mip(mip))


class PostPass:
    """post: implies lighting (and carries its refusals); after the lighting dispatch the frame runs AdaptLuminanceRenderer and
    PostProcessRenderer: with a manual exposure of 0, a clear of the 256-word histogram, "adaptluminance_CS_GenerateLuminanceHistogram"
    and "adaptluminance_CS_AdaptExposure"; with a manual exposure > 0, one write of it into self.luminance instead
    (AdaptLuminanceRenderer.cpp:149-153); then always "postprocess_PS_PostProcess" into self.back_buffer (RGBA8_UNORM).
    exposure = (manual, middle_gray): m_ManualExposureOverride and m_MiddleGray; auto_exposure = (min_luminance, max_luminance,
    adaptation_speed): the speed is the already clamped m_AdaptationSpeed of one frame (the reference's 0.0025 per ms times the
    frame time; the driver has no clock); bloom = (rhi.Texture or None, strength): an R11G11B10_FLOAT texture at render
    resolution, None = unbound = black.  self.luminance (one float, 1.0 at construction and after reset_exposure()) and
    self.exposure_texture (1 x 1 R32_FLOAT) survive across record() and frames.  self.post_consts holds the three parameter
    structs of the last record() (histogram, adapt, post; the first two None with a manual exposure)."""
    back_buffer = exposure_texture = luminance = histogram = post_consts = None

    def _check_post(self, post, exposure, auto_exposure, bloom):
        self.post_on = bool(post)
        self.manual_exposure, self.middle_gray = np.float32(exposure[0]), np.float32(exposure[1])
        self.min_luminance, self.max_luminance, self.adaptation_speed = (np.float32(x) for x in auto_exposure)
        self.bloom, self.bloom_strength = bloom[0], np.float32(bloom[1])

    def _create_post(self):                          # AdaptLuminanceRenderer::Initialize (AdaptLuminanceRenderer.cpp:54-76) + the swap chain's format
        dev = self.dev
        if self.post_on:
            self.back_buffer = self._own(dev.create_texture(self.view.renderW, self.view.renderH, 1, rhi.FORMAT_RGBA8_UNORM, "Back Buffer"))
            self.exposure_texture = self._own(dev.create_texture(1, 1, 1, rhi.FORMAT_R32_FLOAT, "Exposure Texture"))
            self.luminance = self._own(dev.create_buffer(4, "Exposure Buffer"))
            self.histogram = self._own(dev.create_buffer(4 * 256, "Luminance Histogram"))
            self.reset_exposure()

    # ---- AdaptLuminanceRenderer::Render (AdaptLuminanceRenderer.cpp:119-215) + PostProcessRenderer::Render (:37-74) -----
    def reset_exposure(self):
        """The adapted luminance and the exposure texel back to kInitialExposure = 1.0."""
        self.dev.wait_idle()
        self.luminance.upload(np.array([1.0], np.float32))
        self.exposure_texture.upload_mip(0, np.array([[1.0]], np.float32))

    def _adapt_luminance(self, cl):
        v = self.view
        hk = ak = None
        if self.manual_exposure > 0.0:                                                   # :149-153
            cl.write_buffer(self.luminance, np.array([self.manual_exposure], np.float32))
        else:
            lo, hi = I.log_luminance_range(self.min_luminance, self.max_luminance)      # :155-156
            cl.clear_buffer_u32(self.histogram, 0)
            hk = np.zeros(1, I.GenerateLuminanceHistogramParameters)
            hk["m_SrcColorDims"] = (v.renderW, v.renderH)
            hk["m_MinLogLuminance"] = lo
            hk["m_InverseLogLuminanceRange"] = np.float32(1.0) / np.float32(hi - lo)
            cl.dispatch("adaptluminance_CS_GenerateLuminanceHistogram", [PUSH(0), TEX_SRV(0, self.lighting_output), UAV(0, self.histogram)],
                        ((v.renderW + 15) // 16, (v.renderH + 15) // 16, 1), push=hk)
            ak = np.zeros(1, I.AdaptExposureParameters)
            ak["m_AdaptationSpeed"] = self.adaptation_speed
            ak["m_MinLogLuminance"] = lo
            ak["m_LogLuminanceRange"] = np.float32(hi - lo)
            ak["m_NbPixels"] = v.renderW * v.renderH
            ak["m_MiddleGray"] = self.middle_gray
            cl.dispatch("adaptluminance_CS_AdaptExposure", [PUSH(0), SRV(0, self.histogram), UAV(0, self.luminance), TEX_UAV(1, self.exposure_texture, 0)],
                        (1, 1, 1), push=ak)
        self.post_consts = (hk, ak, None)

    def _post_process(self, cl, colour):
        """colour: what the pass tone-maps, LightingOutput or the anti-aliased output (PostProcessRenderer.cpp:25-27, :52)."""
        v = self.view
        pk = np.zeros(1, I.PostProcessParameters)
        pk["m_OutputDims"] = (v.renderW, v.renderH)
        pk["m_ManualExposure"] = self.manual_exposure
        pk["m_MiddleGray"] = self.middle_gray
        bloom = self.bloom_texture if self.bloom_texture is not None else self.bloom     # generated, or the caller's
        pk["m_BloomStrength"] = self.bloom_strength if bloom is not None else 0.0       # m_bEnableBloom ? m_BloomStrength : 0
        b = [PUSH(0), TEX_SRV(0, colour), SRV(1, self.luminance), TEX_UAV(0, self.back_buffer, 0), SAMPLER(0)]
        if bloom is not None:
            b.append(TEX_SRV(2, bloom))
        cl.dispatch("postprocess_PS_PostProcess", b, I.groups8(v.renderW, v.renderH), push=pk)
        self.post_consts = (*self.post_consts[:2], pk)
