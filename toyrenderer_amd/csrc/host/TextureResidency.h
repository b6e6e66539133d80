// TextureResidency.h -- THE RESIDENCY RULE of texture streaming, stated once in host code with no GPU in it.  Its callers are
// trhost_residency_round (include/trhost.h) and, through it, Python (host.residency_round: FrameDriver(streaming=...));
// tests/texture_streaming_ref.c restates it.  The reference links a tiled-texture library that is not in its tree; like RTXGI
// and NRD before, the rule is this project's own statement.
//
// A streamable texture of W x H texels and `mips` levels has a region of RW x RH texels of mip 0.  Level k is STANDARD when every
// level j <= k has (W >> j) and (H >> j) a multiple >= 1 of RW and RH, so that it is whole tiles and the tile (rx >> k, ry >> k) exists
// for every region (a size that is no power of two stops early: 24 x 24 with 8 x 8 has one standard level, 48 x 32 two), and
// k < mips - 1 (the last level always belongs to the PACKED TAIL, which is resident); S = the number of standard levels.
// Level k has (W >> k) / RW x (H >> k) / RH TILES; the tile of level k that covers region (rx, ry) is (rx >> k, ry >> k).  Tiles are numbered level by level, row-major.  One ROUND = one processed (decoded) feedback of the texture:
//   required : a region with byte q != 0xFF requires its covering tile at every standard level k >= q;
//   map      : a required tile that is not resident is mapped -- there is no budget (the reference runs with zero standby tiles); its
//              idle count becomes 0;
//   evict    : a resident tile that is not required adds one to its idle count and is unmapped when the count reaches evictAfter:
//              it was not required by any of the last evictAfter rounds;
//   min-mip  : per region, the finest level m such that its covering tiles are resident at every standard level >= m; S if none.
// A frame in which the texture's feedback is not processed changes nothing.
#pragma once

#include <cstdint>
#include <vector>

namespace residency
{

struct Tiled
{
    uint32_t width = 0, height = 0, mips = 0, regionW = 0, regionH = 0;
    uint32_t tileBytes = 0;                                    // bytes uploaded per mapped tile

    uint32_t standardLevels() const;
    uint32_t tilesX(uint32_t k) const { return (width >> k) / regionW; }
    uint32_t tilesY(uint32_t k) const { return (height >> k) / regionH; }
    uint32_t tileOffset(uint32_t k) const;                     // first tile of level k; level S: the total
    uint32_t regionsX() const { return width / regionW; }
    uint32_t regionsY() const { return height / regionH; }
};

// tiles total, tiles resident, tiles and bytes uploaded this round: the numbers of the reference's ImGui panel
struct Stats { uint32_t tilesTotal = 0, tilesResident = 0, tilesMapped = 0, tilesUnmapped = 0; uint64_t bytesUploaded = 0; };

// The residency of one texture: one entry per tile.  Starts with the packed tail alone.
struct State
{
    std::vector<uint8_t> resident;
    std::vector<uint32_t> idle;
    void reset(const Tiled& t) { resident.assign(t.tileOffset(t.standardLevels()), 0); idle.assign(resident.size(), 0); }
};

// One round.  feedback: regionsX x regionsY decoded bytes.  mapped / unmapped: the tiles this round maps / unmaps (tile numbers, in order).
Stats round(const Tiled& t, const uint8_t* feedback, uint32_t evictAfter, State& state, std::vector<uint32_t>& mapped, std::vector<uint32_t>& unmapped);

// regionsX x regionsY bytes from the residency
void minMip(const Tiled& t, const State& state, uint8_t* out);

} // namespace residency
