/* bc_ref.c -- the decode of the block-compressed material textures (BC1, BC2, BC3, BC4, BC5; csrc/material_textures.hip.h,
 * DESIGN.md 3), in C: the definition the GPU sampler, interop.bc_decode and Pillow's DDS decoder are compared against.
 *
 * A BC texture samples exactly as its decoded twin would: an RGBA8_UNORM (or SRGBA8_UNORM, for the _SRGB variants) texture whose
 * level-k texels are the words this file gives for the level-k blocks.  Everything else of the sampler is
 * tests/material_textures_ref.c, evaluated on the twin.
 *
 * The decode is integer and byte-exact.  Texel (x, y) of a level is texel i = 4 * (y & 3) + (x & 3) of block (x >> 2, y >> 2);
 * a level of w x h texels has ceil(w / 4) x ceil(h / 4) blocks, row-major.  All fields are little-endian, every division truncates.
 *   colour block (8 bytes): c0 (RGB565) at bytes 0-1, c1 at bytes 2-3, 2-bit indices at bytes 4-7, texel i at bits 2i.
 *       Endpoints to 8 bits by bit replication: r = r5 << 3 | r5 >> 2, g = g6 << 2 | g6 >> 4, b like r.
 *       Four-colour mode: p2 = (2 p0 + p1) / 3, p3 = (p0 + 2 p1) / 3 per channel, alpha 255.
 *       Three-colour mode: p2 = (p0 + p1) / 2, p3 = (0, 0, 0) with alpha 0.
 *       BC1: four-colour mode iff c0 > c1 (unsigned 16-bit words).  BC2, BC3: always four-colour mode.
 *   alpha block (8 bytes: BC3's alpha, BC4, each half of BC5): a0, a1, then 48 bits of 3-bit indices, texel i at bits 3i.
 *       a0 > a1: p[k] = ((8 - k) a0 + (k - 1) a1) / 7, k = 2..7; else p[k] = ((6 - k) a0 + (k - 1) a1) / 5, k = 2..5, p6 = 0, p7 = 255.
 *   BC2 (16 bytes): bytes 0-7 sixteen 4-bit alphas, texel i at bits 4i, alpha = a4 * 17; bytes 8-15 the colour block.
 *   BC3 (16 bytes): alpha block, colour block.  BC4 (8 bytes): (R, 0, 0, 255).  BC5 (16 bytes): R block, G block: (R, G, 0, 255).
 * The format numbers are include/trhip.h's TRHIP_FORMAT_BC*; a _SRGB variant decodes to the same bytes as its UNORM twin. */
#include <stdint.h>

enum { BC1 = 14, BC1_SRGB = 15, BC2 = 16, BC2_SRGB = 17, BC3 = 18, BC3_SRGB = 19, BC4 = 20, BC5 = 21 };

uint32_t bc_block_bytes(uint32_t format)
{
    if (format == BC1 || format == BC1_SRGB || format == BC4) return 8;
    if (format == BC2 || format == BC2_SRGB || format == BC3 || format == BC3_SRGB || format == BC5) return 16;
    return 0;
}

static uint32_t u16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

static void colour_texel(const uint8_t* blk, uint32_t i, int bc1, uint8_t out[4])
{
    const uint32_t c0 = u16(blk), c1 = u16(blk + 2);
    const uint32_t indices = (uint32_t)blk[4] | (uint32_t)blk[5] << 8 | (uint32_t)blk[6] << 16 | (uint32_t)blk[7] << 24;
    const uint32_t k = (indices >> (2 * i)) & 3;
    const int four = !bc1 || c0 > c1;
    uint32_t p0[3], p1[3];
    const uint32_t r0 = c0 >> 11, g0 = (c0 >> 5) & 63, b0 = c0 & 31, r1 = c1 >> 11, g1 = (c1 >> 5) & 63, b1 = c1 & 31;
    p0[0] = r0 << 3 | r0 >> 2; p0[1] = g0 << 2 | g0 >> 4; p0[2] = b0 << 3 | b0 >> 2;
    p1[0] = r1 << 3 | r1 >> 2; p1[1] = g1 << 2 | g1 >> 4; p1[2] = b1 << 3 | b1 >> 2;
    for (int c = 0; c < 3; ++c) {
        uint32_t v;
        if (k == 0) v = p0[c];
        else if (k == 1) v = p1[c];
        else if (four) v = k == 2 ? (2 * p0[c] + p1[c]) / 3 : (p0[c] + 2 * p1[c]) / 3;
        else v = k == 2 ? (p0[c] + p1[c]) / 2 : 0;
        out[c] = (uint8_t)v;
    }
    out[3] = (!four && k == 3) ? 0 : 255;
}

static uint8_t alpha_texel(const uint8_t* blk, uint32_t i)
{
    const uint32_t a0 = blk[0], a1 = blk[1];
    uint64_t bits = 0;
    for (int j = 0; j < 6; ++j) bits |= (uint64_t)blk[2 + j] << (8 * j);
    const uint32_t k = (uint32_t)(bits >> (3 * i)) & 7;
    if (k == 0) return (uint8_t)a0;
    if (k == 1) return (uint8_t)a1;
    if (a0 > a1) return (uint8_t)(((8 - k) * a0 + (k - 1) * a1) / 7);
    if (k == 6) return 0;
    if (k == 7) return 255;
    return (uint8_t)(((6 - k) * a0 + (k - 1) * a1) / 5);
}

/* R, G, B, A of texel i (0..15) of one block */
void bc_texel(uint32_t format, const uint8_t* blk, uint32_t i, uint8_t out[4])
{
    out[0] = out[1] = out[2] = 0; out[3] = 255;
    switch (format) {
    case BC1: case BC1_SRGB: colour_texel(blk, i, 1, out); break;
    case BC2: case BC2_SRGB:
        colour_texel(blk + 8, i, 0, out);
        out[3] = (uint8_t)(((blk[i >> 1] >> (4 * (i & 1))) & 15) * 17);
        break;
    case BC3: case BC3_SRGB:
        colour_texel(blk + 8, i, 0, out);
        out[3] = alpha_texel(blk, i);
        break;
    case BC4: out[0] = alpha_texel(blk, i); break;
    case BC5: out[0] = alpha_texel(blk, i); out[1] = alpha_texel(blk + 8, i); break;
    default: break;
    }
}

/* One level of w x h texels from its ceil(w / 4) x ceil(h / 4) blocks: out is h x w x 4 bytes.  Texels of an edge block beyond
 * the level are not written anywhere.  Returns 0, or -1 for a format that is not block-compressed. */
int bc_decode_level(uint32_t format, const uint8_t* blocks, uint32_t w, uint32_t h, uint8_t* out)
{
    const uint32_t nb = bc_block_bytes(format), bw = (w + 3) / 4;
    if (!nb) return -1;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            bc_texel(format, blocks + (uint64_t)((y >> 2) * bw + (x >> 2)) * nb, 4 * (y & 3) + (x & 3), out + ((uint64_t)y * w + x) * 4);
    return 0;
}
