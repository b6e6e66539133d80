// dds_parse.cpp -- trhip_dds_parse (include/trhip.h): the header of a .dds file, from the public description of the container
// (the "DDS" programming guide: DDS_HEADER, DDS_PIXELFORMAT, DDS_HEADER_DXT10).  Plain C++, no device, like trhip_blas_build.
//
// The file: the magic "DDS " (4 bytes), DDS_HEADER (124 bytes), DDS_HEADER_DXT10 (20 bytes) iff the pixel format's fourCC is "DX10",
// then the levels of the one surface back to back, largest first, without padding.  All fields are little-endian uint32.
//   offset   4 dwSize (124)      8 dwFlags     12 dwHeight    16 dwWidth    24 dwDepth    28 dwMipMapCount
//           76 ddspf.dwSize (32)  80 ddspf.dwFlags (DDPF_FOURCC = 4)        84 ddspf.dwFourCC             112 dwCaps2
//          128 dxgiFormat        132 resourceDimension (TEXTURE2D = 3)     136 miscFlag (TEXTURECUBE = 4)  140 arraySize
// The parser answers what the file says; which of a UNORM / _SRGB pair a material slot wants is the loaders' choice.
#include <cstring>

#include "trhip_internal.h"

namespace
{

using trhip::fail;

constexpr uint32_t kMagic = 0x20534444u;                          // "DDS "
constexpr uint32_t kHeaderBytes = 124, kPixelFormatBytes = 32, kDx10Bytes = 20;
constexpr uint32_t DDSD_DEPTH = 0x800000u, DDPF_FOURCC = 0x4u, DDSCAPS2_CUBEMAP = 0x200u, DDSCAPS2_VOLUME = 0x200000u;
constexpr uint32_t kDimensionTexture2D = 3, kMiscTextureCube = 0x4u;

constexpr uint32_t fourCC(char a, char b, char c, char d) { return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24; }

uint32_t word(const uint8_t* p, uint64_t off)
{
    return (uint32_t)p[off] | (uint32_t)p[off + 1] << 8 | (uint32_t)p[off + 2] << 16 | (uint32_t)p[off + 3] << 24;
}

// TRHIP_FORMAT_* of a legacy fourCC, 0 for one that is not accepted
uint32_t legacyFormat(uint32_t cc)
{
    if (cc == fourCC('D', 'X', 'T', '1')) return TRHIP_FORMAT_BC1_UNORM;
    if (cc == fourCC('D', 'X', 'T', '2') || cc == fourCC('D', 'X', 'T', '3')) return TRHIP_FORMAT_BC2_UNORM;
    if (cc == fourCC('D', 'X', 'T', '4') || cc == fourCC('D', 'X', 'T', '5')) return TRHIP_FORMAT_BC3_UNORM;
    if (cc == fourCC('A', 'T', 'I', '1') || cc == fourCC('B', 'C', '4', 'U')) return TRHIP_FORMAT_BC4_UNORM;
    if (cc == fourCC('A', 'T', 'I', '2') || cc == fourCC('B', 'C', '5', 'U')) return TRHIP_FORMAT_BC5_UNORM;
    return 0;
}

// TRHIP_FORMAT_* of a DXGI_FORMAT, 0 for one that is not accepted
uint32_t dxgiFormat(uint32_t f)
{
    switch (f) {
    case 28: return TRHIP_FORMAT_RGBA8_UNORM;
    case 29: return TRHIP_FORMAT_SRGBA8_UNORM;
    case 71: return TRHIP_FORMAT_BC1_UNORM;
    case 72: return TRHIP_FORMAT_BC1_UNORM_SRGB;
    case 74: return TRHIP_FORMAT_BC2_UNORM;
    case 75: return TRHIP_FORMAT_BC2_UNORM_SRGB;
    case 77: return TRHIP_FORMAT_BC3_UNORM;
    case 78: return TRHIP_FORMAT_BC3_UNORM_SRGB;
    case 80: return TRHIP_FORMAT_BC4_UNORM;
    case 83: return TRHIP_FORMAT_BC5_UNORM;
    default: return 0;
    }
}

} // namespace

int trhip_dds_parse(const void* file, uint64_t bytes, trhip_dds_info* out)
{
    if (!file || !out) return fail(TRHIP_ERR_INVALID, "dds_parse: null argument");
    const uint8_t* p = (const uint8_t*)file;
    if (bytes < 4 + (uint64_t)kHeaderBytes) return fail(TRHIP_ERR_INVALID, "dds_parse: %llu bytes are shorter than the magic and the 124-byte header", (unsigned long long)bytes);
    if (word(p, 0) != kMagic) return fail(TRHIP_ERR_INVALID, "dds_parse: bad magic 0x%08x, a DDS file begins with 'DDS '", word(p, 0));
    if (word(p, 4) != kHeaderBytes || word(p, 76) != kPixelFormatBytes)
        return fail(TRHIP_ERR_INVALID, "dds_parse: bad header sizes %u and %u, the header is 124 bytes and its pixel format 32", word(p, 4), word(p, 76));
    const uint32_t flags = word(p, 8), height = word(p, 12), width = word(p, 16), depth = word(p, 24), mips = word(p, 28);
    const uint32_t pfFlags = word(p, 80), cc = word(p, 84), caps2 = word(p, 112);
    if (width == 0 || height == 0 || width > 65536u || height > 65536u) return fail(TRHIP_ERR_INVALID, "dds_parse: bad dimensions %u x %u", width, height);
    if (mips == 0) return fail(TRHIP_ERR_INVALID, "dds_parse: mipMapCount is 0; a file states at least one level");
    if (mips > 16) return fail(TRHIP_ERR_INVALID, "dds_parse: %u levels, at most 16", mips);
    if (caps2 & DDSCAPS2_CUBEMAP) return fail(TRHIP_ERR_INVALID, "dds_parse: a cube texture is not supported");
    if ((caps2 & DDSCAPS2_VOLUME) || ((flags & DDSD_DEPTH) && depth > 1)) return fail(TRHIP_ERR_INVALID, "dds_parse: a volume texture is not supported");
    if (!(pfFlags & DDPF_FOURCC))
        return fail(TRHIP_ERR_INVALID, "dds_parse: the pixel format has no fourCC (flags 0x%x): uncompressed legacy layouts are not supported, RGBA8 comes with a DX10 header", pfFlags);
    uint64_t data = 4 + (uint64_t)kHeaderBytes;
    uint32_t format = 0;
    if (cc == fourCC('D', 'X', '1', '0')) {
        if (bytes < data + kDx10Bytes) return fail(TRHIP_ERR_INVALID, "dds_parse: %llu bytes are shorter than the DX10 header", (unsigned long long)bytes);
        const uint32_t dxgi = word(p, 128), dimension = word(p, 132), misc = word(p, 136), arraySize = word(p, 140);
        data += kDx10Bytes;
        if (misc & kMiscTextureCube) return fail(TRHIP_ERR_INVALID, "dds_parse: a cube texture is not supported");
        if (dimension != kDimensionTexture2D) return fail(TRHIP_ERR_INVALID, "dds_parse: resource dimension %u: a 1D or volume texture is not supported, a 2D texture is 3", dimension);
        if (arraySize != 1) return fail(TRHIP_ERR_INVALID, "dds_parse: array size %u, only 1 is supported", arraySize);
        if (dxgi == 81 || dxgi == 84) return fail(TRHIP_ERR_INVALID, "dds_parse: DXGI format %u is an SNORM variant (BC%u_SNORM), not supported", dxgi, dxgi == 81 ? 4u : 5u);
        if (dxgi >= 94 && dxgi <= 99) return fail(TRHIP_ERR_INVALID, "dds_parse: DXGI format %u is %s, not supported", dxgi, dxgi <= 96 ? "BC6H" : "BC7");
        format = dxgiFormat(dxgi);
        if (!format) return fail(TRHIP_ERR_INVALID, "dds_parse: unsupported pixel format: DXGI format %u", dxgi);
    } else {
        if (cc == fourCC('B', 'C', '4', 'S') || cc == fourCC('B', 'C', '5', 'S'))
            return fail(TRHIP_ERR_INVALID, "dds_parse: fourCC '%c%c%c%c' is an SNORM variant, not supported", (char)p[84], (char)p[85], (char)p[86], (char)p[87]);
        format = legacyFormat(cc);
        if (!format) return fail(TRHIP_ERR_INVALID, "dds_parse: unsupported pixel format: fourCC 0x%08x", cc);
    }
    const uint32_t blockBytes = trhip_format_block_bytes(format);
    memset(out, 0, sizeof *out);
    out->width = width; out->height = height; out->mipLevels = mips; out->format = format;
    for (uint32_t k = 0; k < mips; ++k) {
        const uint64_t w = (width >> k) ? (width >> k) : 1u, h = (height >> k) ? (height >> k) : 1u;
        out->levelOffset[k] = data;
        out->levelBytes[k] = blockBytes ? ((w + 3) / 4) * ((h + 3) / 4) * blockBytes : w * h * 4;
        data += out->levelBytes[k];
    }
    if (data > bytes)
        return fail(TRHIP_ERR_INVALID, "dds_parse: the file is %llu bytes, shorter than its %u levels, which end at byte %llu", (unsigned long long)bytes, mips, (unsigned long long)data);
    return TRHIP_OK;
}
