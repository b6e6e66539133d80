// k_gbuffer.hip -- "basepass_PS_Main_GBuffer": both render targets of the reference's base-pass pixel shader
// (source/shaders/basepass.hlsl:231-253 PS_Main_GBuffer: SV_Target0 = GBufferA, RGBA32_UINT, PackGBuffer of
// lightingcommon.hlsli:28-34; SV_Target1 = GBufferMotion).  Without a texture table: materials WITHOUT textures (GetCommonGBufferParams,
// lightingcommon.hlsli:435-493, is then closed arithmetic on MaterialData's constants); with one at t19: the TEXTURED
// instantiation, which samples the four material textures in software (material_textures.hip.h).  Resolved from the visibility
// buffer in one direct dispatch after the base pass's last raster.  One per-pixel gather serves both targets; the motion
// words are those of "basepass_PS_Main_motion" (k_motion.hip).  There is no GBufferA-only variant: nothing would call it.
//
// The kernel is the GBUFFER = true instantiation of the resolve in visibility_resolve.hip.h; the convention is stated
// there, restated in tests/gbuffer_ref.c, tests/material_textures_ref.c and in DESIGN.md 3.  With a min-mip or feedback map in the table
// the STREAMED instantiation runs (#streamed; material_textures.hip.h, tests/texture_streaming_ref.c, DESIGN.md 12, twentieth amendment):
// 128 VGPRs, 64 bytes of scratch per lane, 4 waves per SIMD; the four samples are taken by one rolled loop so that the sampler with
// its marks exists once in the code object.  #main and #textured are instruction for instruction what they were before it.
// ALPHA_MASK_MODE's discard is not this kernel's: it changes depth, so it runs in the rasters (k_raster.hip, the ALPHA_MASK_MODE=1
// shader names); the resolve shades whatever texels they left.
//
// Cost: on top of the motion resolve the addition has to move 16 B per pixel stored (133 MB at 3840x2160), 24 B of
// material per covered pixel (lines shared by a wave's pixels) and three 4-byte normals from vertex records that are
// already fetched, plus three normalisations (3 sqrt, 9 divisions) and 6 more divisions per pixel.  MEASURED
// (tools/gbuffer_cost.py, generated city of 2251 instances at 3840x2160, 8.29 M covered pixels, modes alternated three times on
// one MI355X; profiles/gbuffer/): the motion resolve alone 103.8 us, this kernel 155.1 us, so GBufferA costs 51 us where its
// 133 MB alone would stream in 21 us at the box's 6.3 TB/s.  The rest is arithmetic: a build that only stores takes 109.5 us,
// one without the vertex normals 121.8 us, one with approximate division and square root 131.4 us -- the correctly rounded
// operations, which the bit-exact bar needs, are the cost; the gather and the store are not.  A first version that divided by
// 1023 nine times per pixel took 184.6 us.  Code object: 59 VGPRs (capped for 8 waves per SIMD), no scratch, no LDS
// (-Rpass-analysis=kernel-resource-usage).
//
// The TEXTURED instantiation (resolveKernel<true, true>) is a divergent gather: up to 16 taps x 2 levels x 4 texels per texture and
// pixel, each texel one 4-byte load whose address depends on the pixel's uv, followed by three LDS table reads.  What hides that
// latency is independent loads in flight, not arithmetic: the eight texels of a tap are issued together, and the bound is
// amdgpu_waves_per_eu(4, 4) -- the 8 waves of the texture-free kernel would need its state (three interpolation points, four
// table entries, the sampler's loop) in 64 VGPRs and spill.  Code object: 116 VGPRs, 32 SGPRs, no scratch, 2048 B of LDS (the sRGB
// and UNORM decode tables), 4 waves per SIMD (-Rpass-analysis=kernel-resource-usage).  The texture-free instantiation is unchanged
// by it: 59 VGPRs, no LDS, 8 waves, the same 1037 instructions as before.  MEASURED (tools/material_texture_cost.py, the city above,
// three modes alternated three times in one session; profiles/gbuffer/material_textures.txt): texture-free on the build before
// textures 157.5 / 157.8 / 158.0 us, texture-free here 157.3 / 158.2 / 157.0 us (inside that spread), all four textures out of 16
// random 256 x 256 textures on every covered pixel 902.2 / 900.7 / 901.3 us: 186 us per texture.  Not attributed yet; part of it is
// the convention's N = ceil(Pmax / Pmin) >= 2 for every footprint that is not exactly isotropic.
#include "visibility_resolve.hip.h"

namespace
{

trhip::ShaderRegistrar r0("basepass_PS_Main_GBuffer", vres::recordResolve<true>, 0);

} // namespace
