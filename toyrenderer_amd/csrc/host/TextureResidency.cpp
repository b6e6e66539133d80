// TextureResidency.cpp -- the residency rule of texture streaming (TextureResidency.h states it).
#include "TextureResidency.h"

namespace residency
{

uint32_t Tiled::standardLevels() const
{
    uint32_t s = 0;
    while (s + 1u < mips && (width >> s) >= regionW && (height >> s) >= regionH && (width >> s) % regionW == 0u && (height >> s) % regionH == 0u) ++s;
    return s;
}

uint32_t Tiled::tileOffset(uint32_t k) const
{
    uint32_t off = 0;
    for (uint32_t j = 0; j < k; ++j) off += tilesX(j) * tilesY(j);
    return off;
}

Stats round(const Tiled& t, const uint8_t* feedback, uint32_t evictAfter, State& state, std::vector<uint32_t>& mapped, std::vector<uint32_t>& unmapped)
{
    const uint32_t S = t.standardLevels(), total = t.tileOffset(S), rx = t.regionsX(), ry = t.regionsY();
    if (state.resident.size() != total) state.reset(t);
    std::vector<uint8_t> required(total, 0);
    for (uint32_t y = 0; y < ry; ++y)
        for (uint32_t x = 0; x < rx; ++x) {
            const uint32_t q = feedback[y * rx + x];
            if (q == 0xFFu) continue;
            for (uint32_t k = q; k < S; ++k) required[t.tileOffset(k) + (y >> k) * t.tilesX(k) + (x >> k)] = 1;
        }
    Stats stats;
    stats.tilesTotal = total;
    mapped.clear();
    unmapped.clear();
    for (uint32_t i = 0; i < total; ++i) {
        if (required[i]) {
            state.idle[i] = 0;
            if (!state.resident[i]) { state.resident[i] = 1; mapped.push_back(i); }
        } else if (state.resident[i] && ++state.idle[i] >= evictAfter) {
            state.resident[i] = 0;
            unmapped.push_back(i);
        }
        stats.tilesResident += state.resident[i];
    }
    stats.tilesMapped = (uint32_t)mapped.size();
    stats.tilesUnmapped = (uint32_t)unmapped.size();
    stats.bytesUploaded = (uint64_t)mapped.size() * t.tileBytes;
    return stats;
}

void minMip(const Tiled& t, const State& state, uint8_t* out)
{
    const uint32_t S = t.standardLevels(), rx = t.regionsX(), ry = t.regionsY();
    for (uint32_t y = 0; y < ry; ++y)
        for (uint32_t x = 0; x < rx; ++x) {
            uint32_t m = S;
            while (m > 0 && state.resident[t.tileOffset(m - 1u) + (y >> (m - 1u)) * t.tilesX(m - 1u) + (x >> (m - 1u))]) --m;
            out[y * rx + x] = (uint8_t)m;
        }
}

} // namespace residency
