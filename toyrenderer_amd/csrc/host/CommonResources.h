// CommonResources.h -- the samplers, dummy resources and the unit sphere the path binds
// (source/CommonResources.cpp:40-102,157,270,276-287,298).  Samplers carry their description only: the
// back end samples the HZB in software with exactly the LinearClampMinReduction semantics.
#pragma once

#include "nvrhi_lite.h"
#include "../ShaderInterop.h"

#include <vector>

class CommonResources
{
public:
    void Initialize();

    nvrhi::SamplerHandle PointClampSampler;
    nvrhi::SamplerHandle LinearClampSampler;               // min/mag/mip linear, clamp: the bloom passes' sampler (BloomRenderer.cpp)
    nvrhi::SamplerHandle LinearClampMinReductionSampler;   // min/mag/mip linear, clamp, SamplerReductionType::Minimum
    nvrhi::BufferHandle DummyUIntStructuredBuffer;         // bound when occlusion culling is off (BasePassRenderers.cpp:318-320)
    nvrhi::TextureHandle BlackTexture;                     // bound as HZB when occlusion culling is off (:357)

    // CreateUnitSphereMesh (:40-102): tessellation 6, 91 vertices, 468 indices, winding reversed; what GIDebugRenderer draws a probe as.
    // The table is exact (BuildUnitSphere): byte for byte ddgi.unit_sphere()'s and tests/ddgi_probe_draw_ref.c's.
    struct Mesh
    {
        nvrhi::BufferHandle m_VertexBuffer, m_IndexBuffer;
        uint32_t m_NumIndices = 0;
    } UnitSphere;
    static void BuildUnitSphere(std::vector<interop::UncompressedRawVertexFormat>& vertices, std::vector<uint32_t>& indices);
};
#define g_CommonResources (*Graphic::GetInstance().m_CommonResources)
