// TextureFeedbackManager.h -- the host loop of texture streaming, with the frame shape of the reference's TextureFeedbackManager
// (source/TextureFeedbackManager.{h,cpp}): PrepareTexturesToProcessThisFrame, BeginFrame, EndFrame.  The residency decisions are
// TextureResidency.h's (the reference's come from rtxts, which is not in its tree); the Python driver's loop is
// toyrenderer_amd/streaming.py, and both give the same maps for the same frames (tests/test_gpu_texture_streaming_loop.py).
//
// A material texture created while streaming is on (trhost_set_texture_streaming before trhost_create_material_texture) and whose
// size is a multiple of the region (trhost_set_texture_streaming_region; default D3D's 64 KB tile shape of its format; a size that is
// no multiple of a GIVEN region is refused, of the default one it stays fully resident) is STREAMED: its mips stay on the host, only its
// packed tail is uploaded, the rest of its storage is filled with kPoisonWord when poison is on, and a min-mip map and a feedback map
// of it take the descriptor indices kMaxMaterialTextures - 1 - 2 j and - 2 - 2 j, which Scene::LoadMaterials fills into the
// materials' slots.  The G-buffer resolve brackets its dispatch with BeginFrame and EndFrame:
//   BeginFrame : for every earlier frame whose read-back slot has arrived (trhip_readback_poll: NEVER waiting for the device; a slot
//                that has not arrived is looked at again next frame), one round of the rule per texture it decoded, tile writes
//                (trhip_cmd_write_texture_region), poison over unmapped tiles, min-mip rewrites; then the round-robin choice of this
//                frame's textures, m_TexturesPerFrame at a time, and the clear of their feedback;
//   EndFrame   : decode of this frame's textures' feedback and the copy into this frame's slot (skipped when every slot is still
//                in flight).
// Textures keep their full device allocation: this saves upload traffic, not memory (twentieth amendment).
#pragma once

#include <deque>
#include <vector>

#include "TextureResidency.h"
#include "nvrhi_lite.h"

class TextureFeedbackManager
{
public:
    static constexpr uint32_t kPoisonWord = 0xFF00FFFFu;
    static constexpr uint32_t kSlots = 3;                  // read-back slots: frames whose feedback may be in flight

    struct Streamed
    {
        uint32_t m_Index = 0, m_MinMipIndex = 0, m_FeedbackIndex = 0;      // descriptor indices of the texture and of its maps
        uint32_t m_BlockBytes = 0;
        nvrhi::TextureHandle m_Texture, m_MinMip, m_Feedback;
        residency::Tiled m_Tiled;
        residency::State m_State;
        std::vector<uint8_t> m_MinMipBytes;
        std::vector<std::vector<uint8_t>> m_Mips;          // the host copy, level by level
        uint32_t m_Offset = 0;                             // first byte of its regions in the decoded buffer
    };

    struct Stats { uint32_t tilesTotal = 0, tilesResident = 0, tilesUploaded = 0, texturesProcessed = 0; uint64_t bytesUploaded = 0; };

    bool m_bEnabled = false, m_bPoison = false;
    uint32_t m_TexturesPerFrame = 1, m_EvictAfter = 4, m_RegionW = 0, m_RegionH = 0;
    std::vector<Streamed> m_Textures;
    Stats m_Stats;

    // Graphic::CreateMaterialTexture's streamed path: true when the texture was taken (`texture` is created, partly uploaded, and
    // its maps are in `table`); false for a texture that is not tiled.
    bool AddTexture(nvrhi::IDevice* device, nvrhi::IDescriptorTable* table, uint32_t capacity, uint32_t index, uint32_t width, uint32_t height, uint32_t mips,
                    nvrhi::Format format, uint32_t blockBytes, const uint8_t* data, nvrhi::TextureHandle& texture);
    const Streamed* Find(uint32_t descriptorIndex) const;
    void BeginFrame(nvrhi::ICommandList* commandList);
    void EndFrame(nvrhi::ICommandList* commandList);
    void Shutdown();

private:
    struct Pending { uint32_t slot; std::vector<uint32_t> textures; };
    void PrepareTexturesToProcessThisFrame();
    void WriteTile(nvrhi::ICommandList* commandList, Streamed& t, uint32_t tile, bool poison);
    std::deque<Pending> m_Pending;
    std::vector<uint32_t> m_ThisFrame;
    uint32_t m_Next = 0, m_Frame = 0;
    nvrhi::BufferHandle m_Decoded;
    nvrhi::StagingBufferHandle m_Readback;
    uint32_t m_DecodedBytes = 0;
};

extern TextureFeedbackManager g_TextureFeedbackManager;
