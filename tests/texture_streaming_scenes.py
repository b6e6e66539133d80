"""Scenes, tables and the two runners (GPU, reference) that the texture-streaming tests share (tests/test_texture_streaming_ref.py,
tests/test_gpu_texture_streaming.py, tests/test_gpu_texture_streaming_loop.py): the quads of tests/material_texture_scenes.py at
80 x 56 pixels over streamable textures of 32 x 32, 64 x 32 and 16 x 64 texels with regions of 8 x 8 (3, 3 and 2 standard levels).
The rule scenes (tests/texture_streaming_rule_scenes.py) bring the regions that are not 8 x 8 and not square, and the textures whose
sides are no powers of two.

A TABLE here is a list of entries in descriptor order: ("texture", mips, format, region or None), ("minmip", texture index, uint8
[ry, rx]) and ("feedback", texture index).  Not a test module: every assert says what it compared."""
import numpy as np

import bc_blocks as B
import bc_ref
import material_texture_scenes as S
import texture_streaming_ref as TS
import visibility_ref as VR
from toyrenderer_amd import interop as I

REGION = (8, 8)
SIZES = [(32, 32), (64, 32), (16, 64)]
FORMATS = [S.RGBA8, S.SRGBA8, B.BC1, B.BC3]
FILL = 0xABCD1234
SRGB_BC = (B.BC1_SRGB, B.BC2_SRGB, B.BC3_SRGB)
STREAMED, TEXTURED = ["basepass_PS_Main_GBuffer#streamed"], ["basepass_PS_Main_GBuffer#textured"]


def full_chain(w, h):
    return max(w, h).bit_length()


def texture(seed, w, h, fmt, region=REGION, normal=False):
    """("texture", mips, format, region) with a full mip chain of independent random levels."""
    levels = full_chain(w, h)
    if fmt in B.BLOCK_BYTES:
        return ("texture", B.block_mips(seed, w, h, levels, fmt), fmt, region)
    return ("texture", S.normal_mips(seed, w, h, levels) if normal else S.random_mips(seed, w, h, levels), fmt, region)


def size_of(mips):
    """(width, height) of mip 0 of a list of uint8 [h, w, 4] levels or of an interop.BlockMips."""
    return (mips.width, mips.height) if isinstance(mips, I.BlockMips) else (mips[0].shape[1], mips[0].shape[0])


def with_maps(textures, minmips=None, feedback=True, minmip=True):
    """The table of `textures` followed by a min-mip map and a feedback map of each streamable one, and {texture index: (min-mip
    index or NONE, feedback index or NONE)}.  minmips: {texture index: uint8 [ry, rx]} (default: all zero)."""
    table, where = list(textures), {}
    for i, t in enumerate(textures):
        if t is None or t[3] is None:
            continue
        w, h = size_of(t[1])
        rx, ry = w // t[3][0], h // t[3][1]
        mm = fb = S.NONE
        if minmip:
            mm = len(table)
            table.append(("minmip", i, np.zeros((ry, rx), np.uint8) if minmips is None or i not in minmips else np.asarray(minmips[i], np.uint8).reshape(ry, rx)))
        if feedback:
            fb = len(table)
            table.append(("feedback", i))
        where[i] = (mm, fb)
    return table, where


def material(where, flags, indices, streamed=None, **kw):
    """S.material with the map indices of `where` filled in for the slots whose texture has maps (streamed: the slots to fill, default all)."""
    m = S.material(flags=flags, indices=indices, **kw)
    for c, (slot, d) in enumerate(zip(S.SLOTS, indices)):
        if d in where and (streamed is None or c in streamed):
            m[slot]["m_MinMapTextureDescriptorIndex"], m[slot]["m_FeedbackTextureDescriptorIndex"] = where[d]
    return m


def random_minmip(seed, w, h, region=REGION, hi=6):
    return np.random.default_rng([seed, w, h]).integers(0, hi, (h // region[1], w // region[0]), dtype=np.uint16).astype(np.uint8)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def ref_table(bc, table):
    """The reference's entries of a table (BC textures as their decoded twins), in order; Feedback entries start as never sampled."""
    out = []
    for e in table:
        if e is None:
            out.append(None)
        elif e[0] == "texture":
            _, mips, fmt, region = e
            if isinstance(mips, I.BlockMips):
                mips, fmt = bc_ref.twin(bc, mips, fmt), (S.SRGBA8 if fmt in SRGB_BC else S.RGBA8)
            out.append(TS.Streamable(mips, fmt, region) if region else TS.MT.Texture(mips, fmt))
        elif e[0] == "minmip":
            out.append(TS.MinMip(e[2]))
        else:
            out.append(TS.Feedback(out[e[1]]))
    return out


def reference(vr, ts, bc, k, scene, materials, table, feedback=True, visualize=False, render=S.RENDER):
    """(vis, GBufferA, motion halves, {feedback entry index: decoded bytes}) of tests/texture_streaming_ref.c."""
    sc, v, vid, tri, rec, lst = scene
    W, H = render
    geo = VR.Geometry(sc, v, vid, tri)
    depth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
    VR.raster(vr, k, geo, rec, lst, 0, depth, vis)
    entries = ref_table(bc, table)
    g, m, _ = TS.gbuffer(ts, k, geo, [rec, None, None, None], [lst, None, None, None], vis, materials, entries, gbuffer_init=np.full((H, W, 4), FILL, np.uint32),
                         feedback=feedback, visualize=visualize)
    return vis, g, VR.to_half_bits(m), {i: TS.decode(ts, e.words) for i, e in enumerate(entries) if isinstance(e, TS.Feedback)}


# ---- the GPU ---------------------------------------------------------------------------------------------------------------------
def upload(dev, table):
    """(rhi.TextureTable, [rhi.Texture in table order]) of a table."""
    from toyrenderer_amd import rhi
    tt = dev.create_texture_table(max(len(table), 1))
    made = []
    for i, e in enumerate(table):
        if e is None:
            made.append(None)
            continue
        if e[0] == "texture":
            t = dev.create_sampled_texture(e[1], e[2], f"material texture {i}")
            if e[3]:
                t.set_streaming_region(*e[3])
        elif e[0] == "minmip":
            t = dev.create_texture(e[2].shape[1], e[2].shape[0], 1, rhi.FORMAT_R8_UINT, f"min-mip of {e[1]}", uav=False)
            t.upload_mip(0, e[2])
        else:
            t = dev.create_sampler_feedback(made[e[1]], f"feedback of {e[1]}")
        made.append(t)
        tt.set(i, t)
    return tt, made


def release(tt, made):
    tt.release()
    for t in made:
        if t is not None:
            t.release()


def decoded_feedback(dev, table, made):
    """{feedback entry index: uint8 [ry, rx]} through decode_sampler_feedback, copy_to_readback and the read-back's read."""
    which = [i for i, e in enumerate(table) if e is not None and e[0] == "feedback"]
    if not which:
        return {}
    sizes = [made[i].w * made[i].hgt for i in which]
    buf = dev.create_buffer((sum(sizes) + 3) // 4 * 4, "decoded feedback")
    rb = dev.create_readback(buf.size, 1)
    cl = dev.create_command_list()
    try:
        cl.open()
        off = 0
        for i, n in zip(which, sizes):
            cl.decode_sampler_feedback(buf, made[i], off)
            off += n
        cl.copy_to_readback(rb, 0, buf, 0, buf.size)
        cl.close()
        dev.execute(cl)
        data, written = rb.read(0)
        assert written == buf.size, (written, buf.size)
        out, off = {}, 0
        for i, n in zip(which, sizes):
            out[i] = data[off:off + n].reshape(made[i].hgt, made[i].w).copy()
            off += n
        return out
    finally:
        cl.release(); rb.release(); buf.release()


def gpu(dev, k, scene, materials, table, feedback=True, visualize=False, render=S.RENDER):
    """(vis, GBufferA, motion halves, profile names, {feedback entry index: decoded bytes}) of one raster and one resolve."""
    import bc_passes as P
    k = np.ascontiguousarray(k).copy()
    k["m_bWriteSamplerFeedback"], k["m_bVisualizeMinMipTilesOnAlbedoOutput"] = int(bool(feedback)), int(bool(visualize))
    tt, made = upload(dev, table)
    try:
        vis, g, mot, names = P.resolve(dev, k, scene, render, materials, tt)
        return vis, g, mot, names, decoded_feedback(dev, table, made)
    finally:
        release(tt, made)


def both(dev, vr, ts, bc, scene, mats, table, what, feedback=True, visualize=False, names=STREAMED):
    """The scene on the GPU and in the reference: every word of the three outputs and every decoded feedback byte equal.  Returns
    (vis, GBufferA, {entry: feedback bytes})."""
    from suite_support import same
    from visibility_scenes import consts
    k = consts(S.view())
    vis, g, mot, got_names, fb = gpu(dev, k, scene, mats, table, feedback, visualize)
    rvis, rg, rmot, rfb = reference(vr, ts, bc, k, scene, mats, table, feedback, visualize)
    same(vis, rvis, what + ": visibility texels")
    same(g, rg, what + ": GBufferA")
    same(mot, rmot, what + ": motion")
    assert sorted(fb) == sorted(rfb), (sorted(fb), sorted(rfb))
    for i in fb:
        same(fb[i], rfb[i], what + f": decoded feedback of entry {i}")
    assert got_names == names, got_names
    assert np.all(g[vis == 0] == FILL), what + ": nothing drawn, nothing written"
    return vis, g, fb


# ---- the scenes of the loop tests (a static camera; the CPU test proves convergence on each before the GPU test relies on it) ---------
def turn(a=0.3):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, s, 0, 0], [-s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def loop_scene(name):
    """(quads, textures, materials builder taking `where`) of a loop scene: 'three' = three quads over three textures (magnified,
    wrapped and rotated, minified into the tail), all four slots of the first streamed; 'floor' = the grazing floor, anisotropic."""
    if name == "three":
        quads = [S.facing(z=-1.2, half=0.3, uv_lo=0.2, uv_hi=0.45, material=0, centre=(-0.45, 0.25)),
                 S.facing(z=-3.0, half=0.6, uv_lo=-1.5, uv_hi=2.5, material=1, centre=(0.55, -0.3), world=turn()),
                 S.facing(z=-30.0, half=5.0, uv_lo=0.0, uv_hi=64.0, material=2, centre=(-8.0, 5.0))]
        textures = [texture(21, 32, 32, S.SRGBA8), texture(22, 64, 32, S.RGBA8, normal=True), texture(23, 16, 64, S.RGBA8)]
        ALL = S.ALBEDO | S.NORMAL | S.MR | S.EMISSIVE

        def mats(where):
            return np.concatenate([material(where, ALL, (0, 1, 2, 0), emissive=(2.0, 0.5, 4.0)),
                                   material(where, S.ALBEDO | S.MR, (1, S.NONE, 0, S.NONE), wrap=(1, 1, 0, 1)),
                                   material(where, S.ALBEDO, (2, S.NONE, S.NONE, S.NONE))])
        return quads, textures, mats
    assert name == "floor", name
    textures = [texture(31, 64, 32, S.SRGBA8), texture(32, 32, 32, S.RGBA8)]
    return [S.floor(material=0)], textures, lambda where: material(where, S.ALBEDO | S.MR, (0, S.NONE, 1, S.NONE))


LOOP_SCENES = ("three", "floor")
