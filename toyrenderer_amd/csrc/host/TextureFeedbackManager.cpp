// TextureFeedbackManager.cpp -- the host loop of texture streaming (TextureFeedbackManager.h states it).
#include "TextureFeedbackManager.h"
#include "Graphic.h"

#include <algorithm>
#include <cstring>
#include <string>

TextureFeedbackManager g_TextureFeedbackManager;

namespace
{
uint32_t MipDim(uint32_t d, uint32_t k) { return std::max(d >> k, 1u); }

uint64_t LevelBytes(uint32_t w, uint32_t h, uint32_t k, uint32_t blockBytes)
{
    const uint64_t mw = MipDim(w, k), mh = MipDim(h, k);
    return blockBytes ? ((mw + 3) / 4) * ((mh + 3) / 4) * blockBytes : mw * mh * 4u;
}
} // namespace

bool TextureFeedbackManager::AddTexture(nvrhi::IDevice* device, nvrhi::IDescriptorTable* table, uint32_t capacity, uint32_t index, uint32_t width, uint32_t height,
                                        uint32_t mips, nvrhi::Format format, uint32_t blockBytes, const uint8_t* data, nvrhi::TextureHandle& texture)
{
    const bool given = m_RegionW != 0 || m_RegionH != 0;
    uint32_t rw = m_RegionW, rh = m_RegionH;
    if (!given) {                                                             // D3D's 64 KB tile shapes
        if (!blockBytes) rw = rh = 128;
        else if (blockBytes == 8) { rw = 512; rh = 256; }
        else rw = rh = 256;
    }
    if (width % rw || height % rh) {
        if (given)
            throw nvrhi::Error("material texture: " + std::to_string(width) + " x " + std::to_string(height) + " texels are no multiple of the streaming region " +
                               std::to_string(rw) + " x " + std::to_string(rh));
        return false;                                                         // not tiled: fully resident, no maps
    }
    if (index + 2u * ((uint32_t)m_Textures.size() + 1u) >= capacity) throw nvrhi::Error("material texture: the descriptor table has no room left for the streaming maps");
    Streamed s;
    s.m_Index = index;
    s.m_BlockBytes = blockBytes;
    s.m_MinMipIndex = capacity - 1u - 2u * (uint32_t)m_Textures.size();
    s.m_FeedbackIndex = s.m_MinMipIndex - 1u;
    s.m_Tiled.width = width; s.m_Tiled.height = height; s.m_Tiled.mips = mips; s.m_Tiled.regionW = rw; s.m_Tiled.regionH = rh;
    s.m_Tiled.tileBytes = blockBytes ? rw * rh / 16u * blockBytes : rw * rh * 4u;
    s.m_State.reset(s.m_Tiled);
    const uint32_t S = s.m_Tiled.standardLevels();
    nvrhi::TextureDesc d;
    d.width = width; d.height = height; d.mipLevels = mips; d.format = format;
    d.debugName = "Material Texture " + std::to_string(index);
    d.initialState = nvrhi::ResourceStates::ShaderResource;
    s.m_Texture = device->createTexture(d);
    nvrhi::throwIfFailed(trhip_texture_set_streaming_region(s.m_Texture->native(), rw, rh), "material texture: streaming region");
    const uint8_t* p = data;
    for (uint32_t k = 0; k < mips; ++k) {                                     // the packed tail is resident; the rest is poison or as allocated
        const uint64_t n = LevelBytes(width, height, k, blockBytes);
        s.m_Mips.emplace_back(p, p + n);
        if (k >= S) nvrhi::throwIfFailed(trhip_texture_upload(s.m_Texture->native(), k, p, n), "material texture upload");
        else if (m_bPoison) {
            std::vector<uint32_t> poison((size_t)(n / 4), kPoisonWord);
            nvrhi::throwIfFailed(trhip_texture_upload(s.m_Texture->native(), k, poison.data(), n), "material texture poison");
        }
        p += n;
    }
    nvrhi::TextureDesc m;
    m.width = s.m_Tiled.regionsX(); m.height = s.m_Tiled.regionsY(); m.format = nvrhi::Format::R8_UINT;
    m.debugName = d.debugName + " min-mip";
    m.initialState = nvrhi::ResourceStates::ShaderResource;
    s.m_MinMip = device->createTexture(m);
    s.m_MinMipBytes.assign((size_t)m.width * m.height, (uint8_t)S);
    nvrhi::throwIfFailed(trhip_texture_upload(s.m_MinMip->native(), 0, s.m_MinMipBytes.data(), s.m_MinMipBytes.size()), "min-mip upload");
    trhip_texture fb = nullptr;
    nvrhi::throwIfFailed(trhip_sampler_feedback_create(device->native(), s.m_Texture->native(), (d.debugName + " feedback").c_str(), &fb), "sampler feedback");
    nvrhi::TextureDesc f;
    f.width = m.width; f.height = m.height; f.debugName = d.debugName + " feedback";
    s.m_Feedback = nvrhi::TextureHandle(new nvrhi::ITexture(fb, f));
    device->writeDescriptorTable(table, s.m_MinMipIndex, s.m_MinMip);
    device->writeDescriptorTable(table, s.m_FeedbackIndex, s.m_Feedback);
    texture = s.m_Texture;
    m_Textures.push_back(std::move(s));
    return true;
}

const TextureFeedbackManager::Streamed* TextureFeedbackManager::Find(uint32_t descriptorIndex) const
{
    for (const Streamed& s : m_Textures)
        if (s.m_Index == descriptorIndex) return &s;
    return nullptr;
}

void TextureFeedbackManager::PrepareTexturesToProcessThisFrame()
{
    const uint32_t T = (uint32_t)m_Textures.size(), n = std::min(std::max(m_TexturesPerFrame, 1u), T);
    m_ThisFrame.clear();
    for (uint32_t i = 0; i < n; ++i) m_ThisFrame.push_back((m_Next + i) % T);
    m_Next = (m_Next + n) % T;
}

void TextureFeedbackManager::WriteTile(nvrhi::ICommandList* commandList, Streamed& t, uint32_t tile, bool poison)
{
    const residency::Tiled& d = t.m_Tiled;
    uint32_t k = 0;
    while (tile >= d.tilesX(k) * d.tilesY(k)) { tile -= d.tilesX(k) * d.tilesY(k); ++k; }
    const uint32_t x = (tile % d.tilesX(k)) * d.regionW, y = (tile / d.tilesX(k)) * d.regionH;
    const uint32_t unit = t.m_BlockBytes ? 4u : 1u, bytes = t.m_BlockBytes ? t.m_BlockBytes : 4u;   // rows and columns of blocks, or of texels
    const uint32_t levelCols = (MipDim(d.width, k) + unit - 1u) / unit, cols = d.regionW / unit, rows = d.regionH / unit;
    std::vector<uint8_t> rect((size_t)cols * rows * bytes);
    for (uint32_t r = 0; r < rows; ++r) {
        uint8_t* dst = rect.data() + (size_t)r * cols * bytes;
        if (poison) for (uint32_t i = 0; i < cols * bytes / 4u; ++i) std::memcpy(dst + 4u * i, &kPoisonWord, 4);
        else std::memcpy(dst, t.m_Mips[k].data() + ((size_t)(y / unit + r) * levelCols + x / unit) * bytes, (size_t)cols * bytes);
    }
    nvrhi::throwIfFailed(trhip_cmd_write_texture_region(commandList->native(), t.m_Texture->native(), k, x, y, d.regionW, d.regionH, rect.data(), rect.size()),
                         "TextureFeedbackManager: tile write");
}

void TextureFeedbackManager::BeginFrame(nvrhi::ICommandList* commandList)
{
    if (!m_bEnabled || m_Textures.empty()) return;
    uint32_t total = 0;
    for (Streamed& t : m_Textures) { t.m_Offset = total; total += t.m_Tiled.regionsX() * t.m_Tiled.regionsY(); }
    total = (total + 3u) & ~3u;
    m_Stats = Stats();
    // what earlier frames decoded and has arrived, oldest first; never waiting for the device
    while (!m_Pending.empty() && m_Readback) {
        int ready = 0;
        nvrhi::throwIfFailed(trhip_readback_poll(m_Readback->native(), m_Pending.front().slot, &ready), "TextureFeedbackManager: poll");
        if (!ready) break;
        std::vector<uint8_t> decoded(m_DecodedBytes);
        uint64_t written = 0;
        nvrhi::throwIfFailed(trhip_readback_read(m_Readback->native(), m_Pending.front().slot, decoded.data(), decoded.size(), &written), "TextureFeedbackManager: read");
        if (written == decoded.size())
            for (uint32_t j : m_Pending.front().textures) {
                Streamed& t = m_Textures[j];
                std::vector<uint32_t> mapped, unmapped;
                const residency::Stats s = residency::round(t.m_Tiled, decoded.data() + t.m_Offset, m_EvictAfter, t.m_State, mapped, unmapped);
                for (uint32_t tile : mapped) WriteTile(commandList, t, tile, false);
                if (m_bPoison) for (uint32_t tile : unmapped) WriteTile(commandList, t, tile, true);
                std::vector<uint8_t> minMip(t.m_MinMipBytes.size());
                residency::minMip(t.m_Tiled, t.m_State, minMip.data());
                if (minMip != t.m_MinMipBytes) {
                    t.m_MinMipBytes = minMip;
                    nvrhi::throwIfFailed(trhip_cmd_write_texture_region(commandList->native(), t.m_MinMip->native(), 0, 0, 0, t.m_Tiled.regionsX(), t.m_Tiled.regionsY(),
                                                                        minMip.data(), minMip.size()), "TextureFeedbackManager: min-mip rewrite");
                }
                m_Stats.tilesUploaded += s.tilesMapped;
                m_Stats.bytesUploaded += s.bytesUploaded;
                ++m_Stats.texturesProcessed;
            }
        m_Pending.pop_front();
    }
    for (const Streamed& t : m_Textures) {
        m_Stats.tilesTotal += (uint32_t)t.m_State.resident.size();
        for (uint8_t r : t.m_State.resident) m_Stats.tilesResident += r;
    }
    m_DecodedBytes = total;
    PrepareTexturesToProcessThisFrame();
    for (uint32_t j : m_ThisFrame)
        nvrhi::throwIfFailed(trhip_cmd_clear_sampler_feedback(commandList->native(), m_Textures[j].m_Feedback->native()), "TextureFeedbackManager: clear");
}

void TextureFeedbackManager::EndFrame(nvrhi::ICommandList* commandList)
{
    if (!m_bEnabled || m_Textures.empty() || m_ThisFrame.empty()) return;
    if (m_Pending.size() >= kSlots) { m_ThisFrame.clear(); return; }          // every slot is in flight: this frame's feedback is dropped
    if (!m_Decoded || m_Decoded->getDesc().byteSize != m_DecodedBytes) {      // created once the textures are known; a later texture starts over
        nvrhi::IDevice* device = g_Graphic.m_NVRHIDevice;
        nvrhi::BufferDesc d;
        d.byteSize = m_DecodedBytes; d.structStride = 4; d.canHaveUAVs = true; d.debugName = "Decoded Sampler Feedback";
        d.initialState = nvrhi::ResourceStates::UnorderedAccess;
        m_Decoded = device->createBuffer(d);
        m_Readback = device->createStagingBuffer(m_DecodedBytes, kSlots);
        m_Pending.clear();
    }
    for (uint32_t j : m_ThisFrame)
        nvrhi::throwIfFailed(trhip_cmd_decode_sampler_feedback(commandList->native(), m_Decoded->native(), m_Textures[j].m_Offset, m_Textures[j].m_Feedback->native()),
                             "TextureFeedbackManager: decode");
    const uint32_t slot = m_Frame % kSlots;
    nvrhi::throwIfFailed(trhip_cmd_copy_to_readback(commandList->native(), m_Readback->native(), slot, m_Decoded->native(), 0, m_DecodedBytes), "TextureFeedbackManager: copy");
    m_Pending.push_back({ slot, m_ThisFrame });
    m_ThisFrame.clear();
    ++m_Frame;
}

void TextureFeedbackManager::Shutdown()
{
    m_Textures.clear();
    m_Pending.clear();
    m_ThisFrame.clear();
    m_Decoded = nullptr;
    m_Readback = nullptr;
    m_Next = m_Frame = m_DecodedBytes = 0;
    m_Stats = Stats();
    m_bEnabled = m_bPoison = false;
    m_TexturesPerFrame = 1; m_EvictAfter = 4; m_RegionW = m_RegionH = 0;
}
