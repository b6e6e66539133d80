// hzb_table_probe.hip -- test-only source of toyrenderer_amd/lib/libtrhip_probe.so (never linked into libtrhip.so).
//
// Reads back the footprint-min table of an HZB (trhip_texture_t::quad, hzb_quad.hip.h): private derived data that no ABI call
// exposes.  A `trhip_texture` handle IS a trhip_texture_t*, so the probe includes the back end's internal header, looks into
// the struct and copies quad.ptr[0 .. quadTotal), quadOffset[] and the version stamps to the host.  No kernel, no write to
// device memory.  Used by tests/test_gpu_hzb.py.
//
// The two libraries are compiled separately: before it trusts any other field, the probe compares width, height, mips and every
// mip offset it reads through the struct with what the product's own trhip_texture_mip_info reports (the caller passes the
// function, the probe does not link the product), and format and total size with what the caller got from the ABI.
//
// The caller synchronises first (trhip_device_join_side_stream + trhip_device_wait_idle): the copy is a plain blocking hipMemcpy.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../toyrenderer_amd/csrc/trhip_internal.h"

extern "C" {

struct HzbTableInfo
{
    uint32_t width, height, mips, format;
    uint32_t quadTotal;               // entries (2 bytes each)
    uint32_t hasTable;                // quad.ptr != nullptr
    uint32_t quadOffset[16];
    uint64_t tableBytes;              // quad.bytes
    uint64_t builtVersion;            // quad.built.version: the texture version the table was last built from (0: never)
    uint64_t version;                 // the texture's current version
};

typedef int (*HzbTableMipInfoFn)(void* texture, uint32_t mip, uint32_t* w, uint32_t* h, uint64_t* offset);

enum { HZB_TABLE_OK = 0, HZB_TABLE_BAD_ARGUMENT = 1, HZB_TABLE_LAYOUT_MISMATCH = 2, HZB_TABLE_NONE = 3, HZB_TABLE_TOO_SMALL = 4, HZB_TABLE_HIP_ERROR = 5 };

unsigned int hzb_table_info_size(void) { return (unsigned int)sizeof(HzbTableInfo); }

// out == nullptr: only *info is filled (HZB_TABLE_OK also without a table: hasTable = 0).  Otherwise copies the quadTotal
// entries into out[0 .. outEntries); HZB_TABLE_NONE if no table has been allocated.
int hzb_table_probe(void* texture, HzbTableMipInfoFn mipInfo, uint32_t expectFormat, uint64_t expectBytes, HzbTableInfo* info,
                    uint16_t* out, uint64_t outEntries)
{
    if (!texture || !mipInfo || !info) return HZB_TABLE_BAD_ARGUMENT;
    const trhip_texture_t* t = (const trhip_texture_t*)texture;
    memset(info, 0, sizeof *info);
    // the struct as this library sees it against the product's own view of it
    if (t->mips == 0 || t->mips > 16 || t->format != expectFormat || t->totalBytes != expectBytes) return HZB_TABLE_LAYOUT_MISMATCH;
    for (uint32_t k = 0; k < t->mips; ++k) {
        uint32_t w = 0, h = 0;
        uint64_t off = 0;
        if (mipInfo(texture, k, &w, &h, &off) != 0) return HZB_TABLE_LAYOUT_MISMATCH;
        const uint32_t ew = (t->width >> k) ? (t->width >> k) : 1u, eh = (t->height >> k) ? (t->height >> k) : 1u;
        if (w != ew || h != eh || off != t->mipOffset[k]) return HZB_TABLE_LAYOUT_MISMATCH;
    }
    {
        uint32_t w, h;
        uint64_t off;
        if (mipInfo(texture, t->mips, &w, &h, &off) == 0) return HZB_TABLE_LAYOUT_MISMATCH;      // the product sees more mips than the struct says
    }
    info->width = t->width; info->height = t->height; info->mips = t->mips; info->format = t->format;
    info->quadTotal = t->quadTotal;
    info->hasTable = t->quad.ptr != nullptr;
    memcpy(info->quadOffset, t->quadOffset, sizeof info->quadOffset);
    info->tableBytes = t->quad.bytes;
    info->builtVersion = t->quad.built.version;
    info->version = t->version.load();
    if (!out) return HZB_TABLE_OK;
    if (!t->quad.ptr) return HZB_TABLE_NONE;
    if (t->quad.bytes < (uint64_t)t->quadTotal * 2 || !t->dev) return HZB_TABLE_LAYOUT_MISMATCH;
    if (outEntries < t->quadTotal) return HZB_TABLE_TOO_SMALL;
    if (hipSetDevice(t->dev->index) != hipSuccess) return HZB_TABLE_HIP_ERROR;
    if (hipMemcpy(out, t->quad.ptr, (size_t)t->quadTotal * 2, hipMemcpyDeviceToHost) != hipSuccess) return HZB_TABLE_HIP_ERROR;
    return HZB_TABLE_OK;
}

} // extern "C"
