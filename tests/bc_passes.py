"""What the GPU tests of the block-compressed textures share (tests/test_gpu_bc_textures.py): tables of BC textures with their
decoded twins, and one visibility dispatch followed by one textured G-buffer resolve through raw dispatches.

Not a test module: every assert here says what it compared."""
import numpy as np

import bc_blocks as B
import bc_ref
import material_textures_ref as MT
import visibility_ref as VR
from toyrenderer_amd import interop as I

FILL = 0xABCD1234
SRGB_FORMATS = (B.BC1_SRGB, B.BC2_SRGB, B.BC3_SRGB)


def twin_of(lib, entry):
    """(mips, format) of the decoded twin of a table entry: a BC entry's levels decoded by tests/bc_ref.c, as SRGBA8_UNORM for the
    _SRGB variants and RGBA8_UNORM for the others; any other entry as it is."""
    if entry is None or not isinstance(entry[0], I.BlockMips):
        return entry
    mips, fmt = entry
    return bc_ref.twin(lib, mips, fmt), (MT.FORMAT_SRGBA8 if fmt in SRGB_FORMATS else MT.FORMAT_RGBA8)


def twins(lib, textures):
    return [twin_of(lib, t) for t in textures]


def upload(dev, textures):
    """(table, [textures]) of a list of (mips, format)."""
    table = dev.create_texture_table(max(len(textures), 1))
    made = []
    for i, t in enumerate(textures):
        made.append(dev.create_sampled_texture(t[0], t[1], f"material texture {i}"))
        table.set(i, made[-1])
    return table, made


def resolve(dev, k, scene, render, materials, table):
    """One visibility dispatch and one G-buffer resolve with `table` at t19: (vis, GBufferA, motion halves, the profile's
    basepass_PS names)."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, PUSH, SRV, TEX_SRV, TEX_TABLE, TEX_UAV
    sc, v, vid, tri, rec, lst = scene
    W, H = render
    k = np.ascontiguousarray(k).copy()
    bufs = [dev.buffer_from(sc["instances"], "inst", uav=False), dev.buffer_from(v, "v", uav=False, min_bytes=20),
            dev.buffer_from(sc["meshData"], "md", uav=False), dev.buffer_from(sc["meshlets"], "ml", uav=False, min_bytes=32),
            dev.buffer_from(vid, "vid", uav=False), dev.buffer_from(tri, "tri", uav=False), dev.buffer_from(rec, "rec", min_bytes=12),
            dev.buffer_from(lst, "lst"), dev.buffer_from(np.ascontiguousarray(materials, I.MaterialData), "materials", uav=False, min_bytes=124)]
    empty = dev.create_buffer(16, "empty")
    args = dev.create_buffer(12, "drawArgs", stride=12, indirect=True)
    args.upload(np.array([len(lst), 1, 1], np.uint32))
    depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
    vis = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "VisibilityBuffer")
    mot = dev.create_texture(W, H, 1, rhi.FORMAT_RG16_FLOAT, "GBufferMotion")
    gba = dev.create_texture(W, H, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA")
    cl = dev.create_command_list()
    try:
        cl.open()
        cl.clear_texture_f32(depth, 0.0); cl.clear_texture_u32(vis, 0); cl.clear_texture_f32(mot, 0.0); cl.clear_texture_u32(gba, FILL)
        cb = cl.constant_buffer(k, "BasePassConstants")
        geo = [CB(0, cb), SRV(0, bufs[0]), SRV(1, bufs[1]), SRV(2, bufs[2]), SRV(4, bufs[3]), SRV(5, bufs[4]), SRV(6, bufs[5])]
        cl.dispatch_indirect("basepass_MS_Main_visibility", geo + [SRV(7, bufs[6]), SRV(9, bufs[7]), TEX_UAV(0, depth, 0), TEX_UAV(1, vis, 0), PUSH(1)],
                             args, push=np.array([0], np.uint32))
        slots = []
        for s in range(4):
            slots += [SRV(10 + s, bufs[6] if s == 0 else empty), SRV(14 + s, bufs[7] if s == 0 else empty)]
        bind = geo + slots + [SRV(3, bufs[8]), TEX_SRV(18, vis), TEX_UAV(0, gba, 0), TEX_UAV(1, mot, 0)]
        cl.dispatch("basepass_PS_Main_GBuffer", bind + [TEX_TABLE(table)], ((W + 7) // 8, (H + 7) // 8, 1))
        cl.close()
        dev.profile_reset(); dev.profile_enable(True)
        try:
            dev.execute(cl); dev.wait_idle()
            prof = dev.profile()
        finally:
            dev.profile_enable(False)
        return vis.download_mip(0), gba.download_mip(0), mot.download_mip(0).view(np.uint16), sorted(n for n in prof if n.startswith("basepass_PS"))
    finally:
        cl.release(); depth.release(); vis.release(); mot.release(); gba.release(); args.release(); empty.release()
        for b in bufs:
            b.release()


def reference(vr, mt, k, scene, render, materials, twin_textures):
    """(vis, GBufferA, motion halves, taps) of tests/material_textures_ref.c on the decoded twins."""
    sc, v, vid, tri, rec, lst = scene
    W, H = render
    geo = VR.Geometry(sc, v, vid, tri)
    depth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
    VR.raster(vr, k, geo, rec, lst, 0, depth, vis)
    table = [None if t is None else MT.Texture(*t) for t in twin_textures]
    g, m, taps = MT.gbuffer(mt, k, geo, [rec, None, None, None], [lst, None, None, None], vis, materials, table, 0,
                            gbuffer_init=np.full((H, W, 4), FILL, np.uint32))
    return vis, g, VR.to_half_bits(m), taps
