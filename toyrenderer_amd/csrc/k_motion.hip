// k_motion.hip -- "basepass_PS_Main_motion": the motion target (GBufferMotion, RG16_FLOAT) of the reference's base pass
// (source/shaders/basepass.hlsl:226-237 GetGBufferParams: prevClip = mul(float4(prevWorldPos, 1), m_PrevWorldToClip),
// motion = ClipXYToUV(prevClip.xy / prevClip.w) * m_OutputResolution - svPosition.xy, 0 when prevClip.w <= 0), resolved
// from the visibility buffer that "basepass_MS_Main_visibility" (k_raster.hip) wrote, in one direct dispatch after the
// base pass's last raster.
//
// CONVENTION (parity unpinned; restated in tests/visibility_ref.c): per pixel with a nonzero texel, decode slot, list
// position and triangle; recompute the three vertices' screen positions and clip w and the edge functions at the pixel
// centre with the functions the raster calls (mesh_stage.hip.h); interpolate prevWorld = mulPoint(position,
// m_PrevWorldMatrix) with perspective weights q_i = e_i / w_i, s = (q0 + q1) + q2, per component
// fma(q2, P2, fma(q1, P1, q0 * P0)) / s; prevClip = the
// 4-column chain of orc_raster_depth's mul_point4; ClipXYToUV = xy * (0.5, -0.5) + 0.5 as a multiply then an add.  Both
// components are stored as fp16, round to nearest even (a NaN as 0x7E00).  Pixels without a texel keep their value.
//
// Cost: meant to be bound by the 8-byte texel read plus a gather (list entry, record, instance, meshlet, triangle, three
// vertices) per covered pixel.  About 8.3 M pixels at 3840x2160 make roughly 100 MB, so a few tens of us were expected;
// tools/visibility_cost.py measured 134 us on a 2251-instance city at 3840x2160 with a 1-D grid-stride mapping: the
// per-pixel gather and the recomputation (~10 divisions) dominate, not the texel stream.  Now one workgroup per 16x16
// pixels (no 64-bit divide; a wave's 16x4 pixels mostly share a triangle, so its gathers hit the same lines): 104 us.  A per-wave
// triangle cache could go further; not done.
//
// The kernel itself is the GBUFFER = false instantiation of the resolve in visibility_resolve.hip.h, which
// "basepass_PS_Main_GBuffer" (k_gbuffer.hip) shares: the same operations, so the same words.
#include "visibility_resolve.hip.h"

namespace
{

trhip::ShaderRegistrar r0("basepass_PS_Main_motion", vres::recordResolve<false>, 0);

} // namespace
