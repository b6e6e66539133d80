#include "CommonResources.h"

#include "Graphic.h"

// Every angle of the tessellation-6 sphere is a multiple of pi / 6, so its sines are exactly 0, 1/2, RN(sqrt(3) / 2) and 1 with the
// quadrant's sign: the table is defined from them and from binary32 products, through no libm (the reference's ScalarSinCos is
// DirectXMath's polynomial, which is not in the tree).  The poles and the seam column are then exactly degenerate: 120 of the 156
// triangles have area.  ReverseWinding (:25-38) is applied: (a, b, c) is stored as (c, b, a) and u as 1 - u.
void CommonResources::BuildUnitSphere(std::vector<interop::UncompressedRawVertexFormat>& vertices, std::vector<uint32_t>& indices)
{
    const float R = 0x1.bb67aep-1f;                                           // RN(sqrt(3) / 2)
    const float S[12] = { 0.0f, 0.5f, R, 1.0f, R, 0.5f, 0.0f, -0.5f, -R, -1.0f, -R, -0.5f };     // sin(k pi / 6)
    const uint32_t kVerticalSegments = 6, kHorizontalSegments = 12, stride = kHorizontalSegments + 1;
    vertices.clear(); indices.clear();
    for (uint32_t i = 0; i <= kVerticalSegments; i++) {
        const float dy = S[(i + 9) % 12], dxz = S[i];                         // sin and cos of the latitude i pi / 6 - pi / 2
        for (uint32_t j = 0; j <= kHorizontalSegments; j++) {
            const float normal[3] = { S[j % 12] * dxz, dy, S[(j + 3) % 12] * dxz };
            interop::UncompressedRawVertexFormat v;
            for (int a = 0; a < 3; ++a) { v.m_Position[a] = normal[a] * 0.5f; v.m_Normal[a] = normal[a]; }
            v.m_TexCoord[0] = 1.0f - float(j) / float(kHorizontalSegments);
            v.m_TexCoord[1] = 1.0f - float(i) / float(kVerticalSegments);
            vertices.push_back(v);
        }
    }
    for (uint32_t i = 0; i < kVerticalSegments; i++)
        for (uint32_t j = 0; j <= kHorizontalSegments; j++) {
            const uint32_t nextI = i + 1, nextJ = (j + 1) % stride;
            const uint32_t quad[6] = { i * stride + nextJ, nextI * stride + j, i * stride + j, nextI * stride + nextJ, nextI * stride + j, i * stride + nextJ };
            indices.insert(indices.end(), quad, quad + 6);
        }
}

void CommonResources::Initialize()
{
    nvrhi::DeviceHandle device = g_Graphic.m_NVRHIDevice;
    nvrhi::SamplerDesc point;
    point.minFilter = point.magFilter = point.mipFilter = false;
    PointClampSampler = device->createSampler(point);
    LinearClampSampler = device->createSampler(nvrhi::SamplerDesc{});
    nvrhi::SamplerDesc minReduction;                                          // CommonResources.cpp:276-287,298
    minReduction.reductionType = nvrhi::SamplerReductionType::Minimum;
    LinearClampMinReductionSampler = device->createSampler(minReduction);

    nvrhi::BufferDesc dummy;                                                  // CommonResources.cpp:270
    dummy.byteSize = 16;
    dummy.structStride = sizeof(uint32_t);
    dummy.canHaveUAVs = true;
    dummy.debugName = "DummyUIntStructuredBuffer";
    DummyUIntStructuredBuffer = device->createBuffer(dummy);

    nvrhi::TextureDesc black;                                                 // CommonResources.cpp:157
    black.width = black.height = 1;
    black.format = nvrhi::Format::R16_FLOAT;
    black.debugName = "BlackTexture";
    BlackTexture = device->createTexture(black);
    std::vector<interop::UncompressedRawVertexFormat> sphereVertices;         // CommonResources.cpp:104-120
    std::vector<uint32_t> sphereIndices;
    BuildUnitSphere(sphereVertices, sphereIndices);
    nvrhi::BufferDesc vb;
    vb.byteSize = sphereVertices.size() * sizeof(interop::UncompressedRawVertexFormat);
    vb.structStride = sizeof(interop::UncompressedRawVertexFormat);
    vb.debugName = "Unit Sphere Vertex Buffer";
    UnitSphere.m_VertexBuffer = device->createBuffer(vb);
    nvrhi::throwIfFailed(trhip_buffer_upload(UnitSphere.m_VertexBuffer->native(), 0, sphereVertices.data(), vb.byteSize), "CommonResources::Initialize");
    nvrhi::BufferDesc ib;
    ib.byteSize = sphereIndices.size() * sizeof(uint32_t);
    ib.structStride = sizeof(uint32_t);
    ib.debugName = "Unit Sphere Index Buffer";
    UnitSphere.m_IndexBuffer = device->createBuffer(ib);
    nvrhi::throwIfFailed(trhip_buffer_upload(UnitSphere.m_IndexBuffer->native(), 0, sphereIndices.data(), ib.byteSize), "CommonResources::Initialize");
    UnitSphere.m_NumIndices = (uint32_t)sphereIndices.size();

    nvrhi::CommandListHandle cl = g_Graphic.AllocateCommandList();
    {
        SCOPED_COMMAND_LIST_AUTO_QUEUE(cl, "CommonResources::Initialize");
        cl->clearBufferUInt(DummyUIntStructuredBuffer, 0);
        cl->clearTextureFloat(BlackTexture, nvrhi::AllSubresources, nvrhi::Color{ 0.0f });
    }
}
