// k_gbuffer.hip -- "basepass_PS_Main_GBuffer": both render targets of the reference's base-pass pixel shader
// (source/shaders/basepass.hlsl:231-253 PS_Main_GBuffer: SV_Target0 = GBufferA, RGBA32_UINT, PackGBuffer of
// lightingcommon.hlsli:28-34; SV_Target1 = GBufferMotion), for materials WITHOUT textures (GetCommonGBufferParams,
// lightingcommon.hlsli:435-493, is then closed arithmetic on MaterialData's constants), resolved from the visibility
// buffer in one direct dispatch after the base pass's last raster.  One per-pixel gather serves both targets; the motion
// words are those of "basepass_PS_Main_motion" (k_motion.hip).  There is no GBufferA-only variant: nothing would call it.
//
// The kernel is the GBUFFER = true instantiation of the resolve in visibility_resolve.hip.h; the convention is stated
// there, restated in tests/gbuffer_ref.c and in DESIGN.md 3.  Texture sampling, sampler feedback, normal maps and the
// alpha-mask discard are out of scope.
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
#include "visibility_resolve.hip.h"

namespace
{

trhip::ShaderRegistrar r0("basepass_PS_Main_GBuffer", vres::recordResolve<true>, 0);

} // namespace
