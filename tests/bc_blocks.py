"""The one generator of test blocks for the block-compressed formats (tests/test_bc_decode.py, tests/test_bc_formats.py,
tests/test_gpu_bc_textures.py): directed blocks that take every branch of the decode, then seeded random bytes.  Every 8- or
16-byte pattern is a valid block of these formats, so random bytes are legitimate inputs.

Directed blocks:
  colour  : c0 > c1, c0 == c1 and c0 < c1, each with indices that use index 3 (transparent black in BC1's three-colour mode, the
            fourth colour in BC2 and BC3, where four-colour mode holds whatever the order), and with every index value at texels 5
            and 10;
  alpha   : a0 > a1, a0 == a1 and a0 < a1, each with indices that use 6 and 7 (0 and 255 in the six-value mode) and with every
            index value at texels 5 and 10, whose 3-bit fields straddle the byte and word boundaries of the block;
  BC2     : explicit alphas 0..15 in order, all 0 and all 15.
BC2 and BC3 pair every alpha half with every colour half; BC5 pairs alpha blocks with themselves, shifted."""
import numpy as np

from toyrenderer_amd import interop as I

BC1, BC1_SRGB, BC2, BC2_SRGB, BC3, BC3_SRGB, BC4, BC5 = range(14, 22)
FORMATS = (BC1, BC2, BC3, BC4, BC5)                       # the five decodes; a _SRGB variant shares its twin's
BLOCK_BYTES = {BC1: 8, BC1_SRGB: 8, BC2: 16, BC2_SRGB: 16, BC3: 16, BC3_SRGB: 16, BC4: 8, BC5: 16}
COLOUR_ENDS = ((0xF81F, 0x07E0), (0x8410, 0x8410), (0x0821, 0xFFDF))          # c0 > c1, c0 == c1, c0 < c1
ALPHA_ENDS = ((200, 40), (77, 77), (30, 220))                                  # a0 > a1, a0 == a1, a0 < a1


def colour_block(c0, c1, indices):
    """8 bytes: the endpoints and sixteen 2-bit indices."""
    word = sum(int(k) << (2 * i) for i, k in enumerate(indices))
    return np.frombuffer(int(c0).to_bytes(2, "little") + int(c1).to_bytes(2, "little") + word.to_bytes(4, "little"), np.uint8)


def alpha_block(a0, a1, indices):
    """8 bytes: the endpoints and sixteen 3-bit indices."""
    word = sum(int(k) << (3 * i) for i, k in enumerate(indices))
    return np.frombuffer(bytes([a0, a1]) + word.to_bytes(6, "little"), np.uint8)


def explicit_alpha(nibbles):
    """8 bytes: BC2's sixteen 4-bit alphas."""
    return np.frombuffer(sum(int(a) << (4 * i) for i, a in enumerate(nibbles)).to_bytes(8, "little"), np.uint8)


def _index_patterns(values):
    """Every index in order, then each value at texel 5 with its complement at texel 10."""
    out = [[i % values for i in range(16)]]
    for v in range(values):
        p = [(i + v) % values for i in range(16)]
        p[5], p[10] = v, values - 1 - v
        out.append(p)
    return out


def directed_colour():
    return [colour_block(c0, c1, p) for c0, c1 in COLOUR_ENDS for p in _index_patterns(4)]


def directed_alpha():
    return [alpha_block(a0, a1, p) for a0, a1 in ALPHA_ENDS for p in _index_patterns(8)]


def directed_explicit():
    return [explicit_alpha(range(16)), explicit_alpha([0] * 16), explicit_alpha([15] * 16)]


def directed(fmt):
    """uint8 [n, block bytes]."""
    fmt = {BC1_SRGB: BC1, BC2_SRGB: BC2, BC3_SRGB: BC3}.get(fmt, fmt)
    col, alp = directed_colour(), directed_alpha()
    if fmt == BC1:
        blocks = col
    elif fmt == BC2:
        blocks = [np.concatenate([a, c]) for a in directed_explicit() for c in col]
    elif fmt == BC3:
        blocks = [np.concatenate([a, c]) for a in alp for c in col]
    elif fmt == BC4:
        blocks = alp
    else:
        blocks = [np.concatenate([a, alp[(i + 7) % len(alp)]]) for i, a in enumerate(alp)]
    return np.stack(blocks).astype(np.uint8)


def blocks(fmt, seed=0, random=4096):
    """The directed blocks of the format followed by `random` blocks of seeded random bytes: uint8 [n, block bytes]."""
    r = np.random.default_rng([seed, fmt, 0xBC])
    return np.concatenate([directed(fmt), r.integers(0, 256, (random, BLOCK_BYTES[fmt]), dtype=np.uint16).astype(np.uint8)])


def block_mips(seed, w, h, levels, fmt):
    """An interop.BlockMips of w x h texels: every level's blocks drawn independently from blocks(fmt) (a wrong level shows), the
    padding texels of edge blocks filled like the others (reading them would show)."""
    pool = blocks(fmt, seed, 256)
    r = np.random.default_rng([seed, w, h, fmt])
    out = []
    for k in range(levels):
        n = ((max(w >> k, 1) + 3) // 4) * ((max(h >> k, 1) + 3) // 4)
        out.append(np.ascontiguousarray(pool[r.integers(0, len(pool), n)]))
    return I.BlockMips(out, w, h)


def full_chain(w, h):
    return max(w, h).bit_length()


# ---- DDS files built from the public description of the container ---------------------------------------------------------------------
DDSD_CAPS, DDSD_HEIGHT, DDSD_WIDTH, DDSD_PIXELFORMAT, DDSD_MIPMAPCOUNT, DDSD_LINEARSIZE, DDSD_DEPTH = 0x1, 0x2, 0x4, 0x1000, 0x20000, 0x80000, 0x800000
DDPF_FOURCC, DDPF_RGB, DDPF_ALPHAPIXELS = 0x4, 0x40, 0x1
DDSCAPS_TEXTURE, DDSCAPS_MIPMAP, DDSCAPS_COMPLEX = 0x1000, 0x400000, 0x8
DDSCAPS2_CUBEMAP, DDSCAPS2_VOLUME = 0x200, 0x200000
LEGACY_FOURCC = {BC1: (b"DXT1",), BC2: (b"DXT2", b"DXT3"), BC3: (b"DXT4", b"DXT5"), BC4: (b"ATI1", b"BC4U"), BC5: (b"ATI2", b"BC5U")}
DXGI = {71: BC1, 72: BC1_SRGB, 74: BC2, 75: BC2_SRGB, 77: BC3, 78: BC3_SRGB, 80: BC4, 83: BC5, 28: 10, 29: 11}


def make_dds(w, h, levels, fourcc=None, dxgi=None, **fields):
    """The bytes of a .dds file of one 2D surface: `levels` are its levels' bytes, largest first; fourcc (4 bytes) for a legacy
    header or dxgi (a DXGI_FORMAT number) for a DX10 header.  fields overrides header words by name: magic, size, flags, height,
    width, depth, mips, pf_size, pf_flags, fourcc, caps2, dimension, misc, array_size."""
    assert (fourcc is None) != (dxgi is None)
    f = dict(magic=0x20534444, size=124, flags=DDSD_CAPS | DDSD_HEIGHT | DDSD_WIDTH | DDSD_PIXELFORMAT | DDSD_MIPMAPCOUNT | DDSD_LINEARSIZE, height=h, width=w,
             pitch=len(levels[0]) if levels else 0, depth=0, mips=len(levels), pf_size=32, pf_flags=DDPF_FOURCC,
             fourcc=int.from_bytes(fourcc if fourcc is not None else b"DX10", "little"), caps=DDSCAPS_TEXTURE | (DDSCAPS_MIPMAP | DDSCAPS_COMPLEX if len(levels) > 1 else 0),
             caps2=0, dxgi=dxgi or 0, dimension=3, misc=0, array_size=1)
    f.update(fields)
    words = [f["magic"], f["size"], f["flags"], f["height"], f["width"], f["pitch"], f["depth"], f["mips"]] + [0] * 11
    words += [f["pf_size"], f["pf_flags"], f["fourcc"], 0, 0, 0, 0, 0, f["caps"], f["caps2"], 0, 0, 0]
    assert len(words) == 32
    if f["fourcc"] == int.from_bytes(b"DX10", "little"):
        words += [f["dxgi"], f["dimension"], f["misc"], f["array_size"], 0]
    return b"".join(int(x).to_bytes(4, "little") for x in words) + b"".join(bytes(np.ascontiguousarray(m).reshape(-1).view(np.uint8)) if not isinstance(m, bytes) else m for m in levels)
