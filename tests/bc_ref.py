"""ctypes wrapper of tests/bc_ref.c, the definition of the block-compressed decode (BC1, BC2, BC3, BC4, BC5): one level's blocks to
its RGBA8 texels, and the decoded twin of a whole interop.BlockMips.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref


def _declare(lib):
    lib.bc_block_bytes.argtypes = [C.c_uint32]
    lib.bc_block_bytes.restype = C.c_uint32
    lib.bc_texel.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.bc_texel.restype = None
    lib.bc_decode_level.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.bc_decode_level.restype = C.c_int


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "bc_ref", _declare)


def _raw(blocks):
    return np.frombuffer(bytes(blocks), np.uint8) if isinstance(blocks, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blocks, np.uint8).reshape(-1)


def decode_level(lib, fmt, blocks, w, h) -> np.ndarray:
    """uint8 [h, w, 4] of one level's blocks (bytes or a uint8 array)."""
    raw = _raw(blocks)
    need = ((w + 3) // 4) * ((h + 3) // 4) * int(lib.bc_block_bytes(fmt))
    assert need and raw.size == need, (fmt, w, h, raw.size, need)
    out = np.full((h, w, 4), 0xEE, np.uint8)
    rc = lib.bc_decode_level(fmt, raw.ctypes.data, w, h, out.ctypes.data)
    assert rc == 0, rc
    return out


def decode_blocks(lib, fmt, blocks) -> np.ndarray:
    """uint8 [n, 4, 4, 4] (block, y, x, channel) of n separate blocks, uint8 [n, block bytes]: a level of 4 n x 4 texels."""
    n = len(blocks)
    img = decode_level(lib, fmt, blocks, 4 * n, 4)
    return np.ascontiguousarray(img.reshape(4, n, 4, 4).transpose(1, 0, 2, 3))


def twin(lib, mips, fmt):
    """The decoded twin of an interop.BlockMips: uint8 [h_k, w_k, 4] per level."""
    return [decode_level(lib, fmt, m, max(mips.width >> k, 1), max(mips.height >> k, 1)) for k, m in enumerate(mips)]
