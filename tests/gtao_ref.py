"""ctypes wrapper of tests/gtao_ref.c, the definition of the three "ambientocclusion_CS_XeGTAO_*" passes (csrc/k_ambientocclusion.hip) and of
the software sine and cosine, and the constant blocks, depth images and G-buffers the CPU and the GPU tests share.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import gtao, synth
from toyrenderer_amd import interop as I

F = np.float32
SENTINEL8 = 0xA7                                   # pre-fill of the byte targets
SENTINEL16 = 0xFE5A                                # pre-fill of the depth chain: a NaN word, which the prefilter never stores


def _declare(lib):
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    for n in ("gt_r16", "gt_sin", "gt_cos"):
        getattr(lib, n).argtypes = [f32]
        getattr(lib, n).restype = f32
    for n in ("gt_r16_n", "gt_half_bits_n", "gt_half_value_n", "gt_sin_n", "gt_cos_n"):
        getattr(lib, n).argtypes = [vp, u64, vp]
        getattr(lib, n).restype = None
    lib.gt_hilbert.argtypes = [u32, u32]
    lib.gt_hilbert.restype = u32
    lib.gt_chain_offset.argtypes = [u32, u32, u32]
    lib.gt_chain_offset.restype = u64
    lib.gt_prefilter.argtypes = [vp, u32, u32, vp, vp]
    lib.gt_main.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    lib.gt_denoise.argtypes = [vp, u32, u32, u32, vp, vp, vp]
    for n in ("gt_prefilter", "gt_main", "gt_denoise"):
        getattr(lib, n).restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "gtao_ref", _declare)


def sincos_bound(lib) -> float:
    return C.c_double.in_dll(lib, "GT_SINCOS_BOUND").value


def _map(lib, fn, x, out_dtype=F, in_dtype=F):
    x = np.ascontiguousarray(x, in_dtype)
    out = np.empty(x.shape, out_dtype)
    getattr(lib, fn)(x.ctypes.data, x.size, out.ctypes.data)
    return out


def r16(lib, x): return _map(lib, "gt_r16_n", x)
def half_bits(lib, x): return _map(lib, "gt_half_bits_n", x, np.uint16)
def half_value(lib, w): return _map(lib, "gt_half_value_n", w, F, np.uint16)
def sin(lib, x): return _map(lib, "gt_sin_n", x)
def cos(lib, x): return _map(lib, "gt_cos_n", x)


# ---- the depth chain's layout: five mips packed back to back, mip k = max(W >> k, 1) x max(H >> k, 1) ---------------------------
def mip_dims(W, H, k):
    return max(W >> k, 1), max(H >> k, 1)


def chain_offsets(W, H):
    offs, off = [], 0
    for k in range(gtao.DEPTH_MIP_LEVELS):
        offs.append(off)
        w, h = mip_dims(W, H, k)
        off += w * h
    return offs, off


def chain_mip(chain, W, H, k):
    offs, _ = chain_offsets(W, H)
    w, h = mip_dims(W, H, k)
    return chain[offs[k]:offs[k] + w * h].reshape(h, w)


# ---- the passes ------------------------------------------------------------------------------------------------------------------
def prefilter(lib, consts, depth) -> np.ndarray:
    """The packed chain (uint16 words) of a depth image (H, W); pre-filled with SENTINEL16."""
    d = np.ascontiguousarray(depth, F)
    H, W = d.shape
    k = np.ascontiguousarray(consts, I.GTAOConstants)
    chain = np.full(chain_offsets(W, H)[1], SENTINEL16, np.uint16)
    lib.gt_prefilter(k.ctypes.data, W, H, d.ctypes.data, chain.ctypes.data)
    return chain


def main_pass(lib, consts, push, W, H, chain, gbufferA):
    """(working AO bytes, edge bytes), each (H, W) uint8."""
    k = np.ascontiguousarray(consts, I.GTAOConstants)
    p = np.ascontiguousarray(push, I.XeGTAOMainPassConstantBuffer)
    c = np.ascontiguousarray(chain, np.uint16)
    g = np.ascontiguousarray(gbufferA, np.uint32)
    assert g.shape == (H, W, 4) and c.size == chain_offsets(W, H)[1]
    ao, edges = np.full((H, W), SENTINEL8, np.uint8), np.full((H, W), SENTINEL8, np.uint8)
    lib.gt_main(k.ctypes.data, p.ctypes.data, W, H, c.ctypes.data, g.ctypes.data, ao.ctypes.data, edges.ctypes.data)
    return ao, edges


def denoise(lib, consts, final_apply, ao, edges) -> np.ndarray:
    k = np.ascontiguousarray(consts, I.GTAOConstants)
    a, e = np.ascontiguousarray(ao, np.uint8), np.ascontiguousarray(edges, np.uint8)
    H, W = a.shape
    out = np.full((H, W), SENTINEL8, np.uint8)
    lib.gt_denoise(k.ctypes.data, int(bool(final_apply)), W, H, a.ctypes.data, e.ctypes.data, out.ctypes.data)
    return out


def denoise_chain(lib, consts, passes, working, edges, ssao=None):
    """AmbientOcclusionRenderer.cpp:211-247: max(1, passes) dispatches ping-ponging between the working texture and the SSAO
    texture, the last with m_FinalApply.  Returns (working, ssao) as they are left: with 2 passes the finally-applied image is in
    `working` and `ssao` holds the first pass's output."""
    pp = [np.array(working, np.uint8), np.full_like(working, SENTINEL8) if ssao is None else np.array(ssao, np.uint8)]
    which = [0, 1]
    n = max(1, passes)
    for i in range(n):
        pp[which[1]] = denoise(lib, consts, i == n - 1, pp[which[0]], edges)
        which.reverse()
    return pp[0], pp[1]


def frame(lib, consts, push, depth, gbufferA, passes):
    """All three passes: dict(chain, working_after_main, edges, working, ssao)."""
    H, W = np.asarray(depth).shape
    chain = prefilter(lib, consts, depth)
    ao, edges = main_pass(lib, consts, push, W, H, chain, gbufferA)
    working, ssao = denoise_chain(lib, consts, passes, ao, edges)
    return dict(chain=chain, working_after_main=ao, edges=edges, working=working, ssao=ssao)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def consts(W, H, settings=None, frame_counter=0, fov_deg=45.0, near=0.1):
    """GTAOConstants of a W x H view of the project's camera."""
    view = synth.make_view(render=(W, H), fov_deg=fov_deg, near=near)
    return gtao.update_constants(W, H, gtao.check_settings(settings or {}), view.viewToClip, frame_counter)


def push(quality, matrix=None):
    return gtao.main_pass_constants(np.eye(4, dtype=F) if matrix is None else matrix, quality)


def pack_normal(n) -> np.ndarray:
    """PackOctadehron + unorm16 of unit normals (..., 3): the word of GBufferA.y."""
    n = np.asarray(n, np.float64)
    n = n / np.sum(np.abs(n), axis=-1, keepdims=True)
    xy = n[..., :2].copy()
    neg = n[..., 2] < 0
    folded = (1.0 - np.abs(xy[..., ::-1])) * np.where(xy >= 0, 1.0, -1.0)
    xy = np.where(neg[..., None], folded, xy)
    q = np.clip(np.floor((xy * 0.5 + 0.5) * 65535.0 + 0.5), 0, 65535).astype(np.uint32)
    return q[..., 0] | q[..., 1] << 16


def gbuffer(normals) -> np.ndarray:
    """GBufferA words (H, W, 4) carrying world normals (H, W, 3); the other fields are zero (the pass reads .y only)."""
    n = np.asarray(normals)
    g = np.zeros(n.shape[:2] + (4,), np.uint32)
    g[..., 1] = pack_normal(n)
    return g


def random_gbuffer(W, H, seed):
    """Seeded unit normals in the hemisphere facing a camera that looks down -Z, every word of the texel filled."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(H, W, 3))
    n[..., 2] = np.abs(n[..., 2]) + 0.05
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    g = rng.integers(0, 2 ** 32, size=(H, W, 4), dtype=np.uint64).astype(np.uint32)
    g[..., 1] = pack_normal(n)
    return g


def depth_images(W, H, seed, near=0.1):
    """name -> (H, W) float32 depth words (reverse z: near / view depth, 0 = sky)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = {}
    out["plane"] = np.full((H, W), near / 4.0, F)
    out["tilted"] = (near / (3.0 + 0.02 * x + 0.011 * y)).astype(F)
    step = np.where(x < W / 2.0, 2.5, 6.0)
    out["step"] = (near / step).astype(F)
    out["noise"] = (near / rng.uniform(0.5, 40.0, size=(H, W))).astype(F)
    out["sky"] = np.zeros((H, W), F)
    checker = (near / (4.0 + 0.1 * rng.uniform(size=(H, W)))).astype(F)
    checker[((x.astype(int) // 3) + (y.astype(int) // 2)) % 2 == 0] = 0.0
    out["checker"] = checker
    bad = out["tilted"].copy()
    bad[H // 2, W // 2] = np.nan
    bad[H // 3, (2 * W) // 3] = -0.25
    out["nan_negative"] = bad
    return out


def view_rays(k, W, H):
    """(vx, vy) per pixel: view-space x / z and y / z of the pixel centre, from the block's own terms in float64."""
    k = np.asarray(k)[0]
    u = (np.arange(W) + 0.5) * float(k["ViewportPixelSize"][0])
    v = (np.arange(H) + 0.5) * float(k["ViewportPixelSize"][1])
    vx = float(k["NDCToViewMul"][0]) * u + float(k["NDCToViewAdd"][0])
    vy = float(k["NDCToViewMul"][1]) * v + float(k["NDCToViewAdd"][1])
    return np.meshgrid(vx, vy)


def crease_scene(k, W, H, near=0.1, depth_at_crease=4.0):
    """Two walls meeting in a concave right angle along the screen's vertical centre line, seen from inside: view depth
    z = depth_at_crease - |x|.  Returns (depth words, GBufferA) with the walls' normals."""
    vx, _ = view_rays(k, W, H)
    z = depth_at_crease / (1.0 + np.abs(vx))
    n = np.zeros((H, W, 3))
    n[..., 0] = np.where(vx > 0, -1.0, 1.0)         # world normal; the pass negates z: view normal (-+1, 0, -1) / sqrt 2
    n[..., 2] = 1.0
    return (near / z).astype(F), gbuffer(n / np.sqrt(2.0))


def wall_scene(W, H, near=0.1, depth=4.0):
    """A fronto-parallel wall at one view depth."""
    n = np.zeros((H, W, 3))
    n[..., 2] = 1.0
    return np.full((H, W), near / depth, F), gbuffer(n)
