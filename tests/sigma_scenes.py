"""Seeded and constructed inputs of the shadow denoiser's tests (tests/test_sigma_ref.py on the CPU, tests/test_gpu_sigma.py on the GPU):
the six images one frame of the chain reads (penumbra, linear view depth, depth, GBufferA, motion, history) with its SigmaConsts.

An input is a dict: k (SigmaConsts), penumbra / lvd / history (uint16 words [H, W]), depth (float32 [H, W]), g (GBufferA uint32
[H, W, 4]), motion (uint32 [H, W], x in the low half).  seeded(): a surface facing the camera with a depth step, blobs of shadow with
penumbrae from a fraction of a pixel to far beyond the cap, sky, and a share of arbitrary words in every image; whole_format(): every
image arbitrary words.  check_condition() says what the seeded set has to reach for the tests that run it to mean anything."""
import numpy as np

import shadow_scenes as SS
import sigma_ref as SG
from toyrenderer_amd import accel, synth
from toyrenderer_amd import interop as I

F = np.float32
SIZES = [(1, 1), (16, 16), (17, 17), (33, 18), (47, 49)]
LIT = SG.NO_OCCLUDER
ONE = 0x3C00                                        # binary16 1.0
JITTER = (0.25, -0.125)


def half_words(x) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def consts(W, H, frame=3, reset=False, jitter=JITTER, settings=None, eye=SS.EYE):
    v = synth.make_view(eye=eye, render=(W, H))
    s = accel.check_denoise_settings({} if settings is None else settings)
    return accel.sigma_consts(I.clip_to_world(v.worldToView, v.viewToClip), v.viewToClip, W, H, s, frame, 0, reset, jitter)


def world_positions(k, depth):
    """float64 [H, W, 3]: where the passes' worldPosition puts every texel, to rounding."""
    k = np.ascontiguousarray(k, I.SigmaConsts)
    W, H = (int(x) for x in k["m_OutputDims"][0])
    M = k["m_ClipToWorld"][0].astype(np.float64)
    x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2.0 - 1.0, (np.arange(H) + 0.5) / H * -2.0 + 1.0)
    clip = np.stack([x, y, np.asarray(depth, np.float64), np.ones((H, W))], -1)
    with np.errstate(all="ignore"):
        h = clip @ M
        return h[..., :3] / h[..., 3:4]


def oct_word(n) -> np.ndarray:
    """PackUnorm2x16(PackOctadehron(n)) of float64 normals [..., 3], to rounding: GBufferA's second word."""
    n = np.asarray(n, np.float64)
    p = n / np.abs(n).sum(-1, keepdims=True)
    fold = p[..., 2] < 0
    x = np.where(fold, (1 - np.abs(p[..., 1])) * np.where(p[..., 0] >= 0, 1, -1), p[..., 0])
    y = np.where(fold, (1 - np.abs(p[..., 0])) * np.where(p[..., 1] >= 0, 1, -1), p[..., 1])
    return (np.rint((x * 0.5 + 0.5) * 65535).astype(np.uint32) | np.rint((y * 0.5 + 0.5) * 65535).astype(np.uint32) << 16)


def flat(W, H, distance=5.0, step_from=None, step_distance=9.0, k=None, **kw):
    """Everything lit on a surface `distance` in front of the camera and facing it (from column step_from on: step_distance), no
    motion, a history of ones.  The view axis is -z and reverse-Z depth = near / distance along it."""
    k = consts(W, H, **kw) if k is None else k
    d = np.full((H, W), distance, np.float64)
    if step_from is not None:
        d[:, step_from:] = step_distance
    depth = (F(0.1) / d.astype(F)).astype(F)
    g = np.zeros((H, W, 4), np.uint32)
    g[..., 1] = oct_word(np.broadcast_to(np.array([0.0, 0.0, 1.0]), (H, W, 3)))
    g[..., 3] = 0x80
    lvd = half_words(np.linalg.norm(world_positions(k, depth) - np.array(SS.EYE), axis=-1))
    return dict(k=k, penumbra=np.full((H, W), LIT, np.uint16), lvd=lvd, depth=depth, g=g, motion=np.zeros((H, W), np.uint32),
                history=np.full((H, W), ONE, np.uint16))


def _arbitrary(rng, shape, share, base):
    """`base` with a share of its words replaced by arbitrary 16-bit words."""
    out = np.array(base, np.uint16)
    at = rng.random(shape) < share
    out[at] = rng.integers(0, 1 << 16, int(at.sum()), dtype=np.uint64).astype(np.uint16)
    return out


def seeded(W, H, seed, hard=False, arbitrary=0.03, **kw):
    """The image the module docstring describes.  hard: every occluded texel's penumbra is 0 (m_TanSunAngularRadius = 0) and no
    arbitrary words."""
    rng = np.random.default_rng([seed, W, H])
    if hard:
        arbitrary = 0.0
    s = flat(W, H, step_from=(2 * W) // 3 if W > 8 else None, **kw)
    # the surface: a little relief (plane weights between 0 and 1) and a tenth of the normals arbitrary
    d = (F(0.1) / s["depth"]).astype(np.float64) * (1.0 + rng.uniform(-4e-3, 4e-3, (H, W)))
    s["depth"] = (F(0.1) / d.astype(F)).astype(F)
    odd = rng.random((H, W)) < 0.1
    s["g"][..., 1][odd] = rng.integers(0, 1 << 32, int(odd.sum()), dtype=np.uint64).astype(np.uint32)
    s["g"][..., 3] = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    lvd = half_words(np.linalg.norm(world_positions(s["k"], s["depth"]) - np.array(SS.EYE), axis=-1))
    # shadow: blobs of a smooth random field; the penumbra grows from left to right, from a fraction of a pixel to far beyond the cap
    yy, xx = np.mgrid[0:H, 0:W]
    field = sum(np.cos(rng.uniform(0.15, 0.6) * xx + rng.uniform(0.15, 0.6) * yy + rng.uniform(0, 6.28)) for _ in range(4))
    occluded = field > 0.3
    width = 0.0 if hard else 0.02 * 400.0 ** (xx / max(W - 1, 1)) * rng.uniform(0.7, 1.3, (H, W))
    penumbra = np.where(occluded, half_words(np.broadcast_to(width, (H, W))), LIT).astype(np.uint16)
    sky = rng.random((H, W)) < (0.0 if hard else 0.06)
    lvd[sky] = LIT
    if not hard:
        beyond = rng.random((H, W)) < 0.02                                       # at and beyond m_DenoisingRange
        lvd[beyond] = half_words(rng.choice([100.0, 100.0625, 4000.0], int(beyond.sum())))
    s["penumbra"], s["lvd"] = _arbitrary(rng, (H, W), arbitrary, penumbra), _arbitrary(rng, (H, W), arbitrary, lvd)
    if arbitrary:
        at = rng.random((H, W)) < arbitrary
        s["depth"].view(np.uint32)[at] = rng.integers(0, 1 << 32, int(at.sum()), dtype=np.uint64).astype(np.uint32)
    # motion: within two pixels, a few far outside; history: a blurred-looking field in [0, 1]
    mv = rng.uniform(-2.0, 2.0, (H, W, 2))
    far = rng.random((H, W)) < 0.05
    mv[far] = rng.uniform(-80.0, 80.0, (int(far.sum()), 2))
    m = _arbitrary(rng, (H, W, 2), arbitrary, half_words(mv))
    s["motion"] = (m[..., 0].astype(np.uint32) | m[..., 1].astype(np.uint32) << 16)
    s["history"] = _arbitrary(rng, (H, W), arbitrary, half_words(np.clip(0.5 + 0.8 * np.cos(0.3 * xx) * np.sin(0.25 * yy) + rng.uniform(-0.2, 0.2, (H, W)), 0, 1)))
    return s


def whole_format(W, H, seed, **kw):
    """Every word of every image arbitrary: the binary16 NaN and infinity codes in penumbra, depth and history among them.  A third of
    the linear view depths are kept ordinary, or nearly every texel would be sky or its tile unfiltered."""
    rng = np.random.default_rng([seed, W, H, 9])
    s = seeded(W, H, seed, **kw)
    words = lambda shape: rng.integers(0, 1 << 16, shape, dtype=np.uint64).astype(np.uint16)       # noqa: E731
    s["penumbra"], s["history"] = words((H, W)), words((H, W))
    keep = rng.random((H, W)) < 0.34
    s["lvd"] = np.where(keep, s["lvd"], words((H, W))).astype(np.uint16)
    for key in ("penumbra", "lvd", "history"):                                   # the codes a uniform draw rarely holds: both infinities, quiet and signalling NaNs
        at = rng.choice(W * H, 6, replace=False)
        s[key].reshape(-1)[at] = [0x7C00, 0xFC00, 0x7E00, 0x7C01, 0xFFFF, 0x7BFF]
    s["depth"] = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32).view(F)
    s["motion"] = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    s["g"] = rng.integers(0, 1 << 32, (H, W, 4), dtype=np.uint64).astype(np.uint32)
    return s


def seeded_set():
    """[(name, input)] at SIZES: seeded images, images of arbitrary words, a reset and a frame without jitter; inputs() adds the sizes
    around the kernels' own tiles."""
    return [(f"seeded {W}x{H}", seeded(W, H, 7 + W)) for W, H in SIZES] + [(f"whole format {W}x{H}", whole_format(W, H, 11 + W)) for W, H in SIZES[2:]] + \
           [("reset 33x18", seeded(33, 18, 5, reset=True)), ("no jitter 47x49", seeded(47, 49, 6, jitter=(0.0, 0.0), frame=14))]


def tile_sizes():
    """The sizes around the tiles the kernels run in: one tile, one texel more in each direction, and a third classified tile in y."""
    from suite_support import kernel_constant
    tw, th, st = kernel_constant("screen_pass.hip.h", "kTileW"), kernel_constant("screen_pass.hip.h", "kTileH"), kernel_constant("k_sigma.hip", "kSigmaTile")
    assert st == accel.kSigmaTile
    return [(tw, th), (tw + 1, th + 1), (st - 1, 2 * st + 1)]


_INPUTS = []


def inputs():
    """seeded_set() and seeded images at tile_sizes(), made once: what both test files run."""
    if not _INPUTS:
        _INPUTS.extend(seeded_set() + [(f"seeded {W}x{H}", seeded(W, H, 21 + W)) for W, H in tile_sizes()])
    return _INPUTS


def run(lib, s):
    return SG.denoise(lib, s["k"], s["penumbra"], s["lvd"], s["depth"], s["g"], s["motion"], s["history"])


def check_condition(results):
    """results: [(name, input, SG.denoise's dict)] of seeded_set().  The set reaches every path bit, the two larger seeded sizes each
    reach all four alone, both tile bytes 1, 2 and 3 occur, and some mask byte is neither 0 nor 255."""
    union = 0
    tile_bytes = set()
    for name, s, r in results:
        bits = int(np.bitwise_or.reduce(r["path"].reshape(-1)))
        union |= bits
        tile_bytes |= set(int(t) for t in r["tiles"].reshape(-1))
        if name in ("seeded 33x18", "seeded 47x49", "no jitter 47x49"):
            assert bits == 15, f"{name}: path bits {bits:#x}, not every path is reached"
            assert np.any((r["mask"] != 0) & (r["mask"] != 255)), f"{name}: the mask is binary"
            capped = int(((r["path"] & SG.PATH_CAPPED) != 0).sum())
            assert 0 < capped < int(((r["path"] & SG.PATH_FILTERED) != 0).sum()), f"{name}: {capped} texels at the radius cap"
    assert union == 15, f"path bits {union:#x}"
    assert {1, 2, 3} <= tile_bytes, tile_bytes


# ---- the constructed cases ------------------------------------------------------------------------------------------------------------
def dilation(W=48, H=48):
    """Everything lit but one occluded texel at (15, 15), the last texel of tile (0, 0).  Its penumbra is 2.5 pixels wide where it
    is seen from, and frame 0 turns nothing at (16, 16) (rotation index 0 in pass 0), so that texel's first tap, 2.5 times
    (-0.47, -0.44), lands on (15, 15)."""
    s = flat(W, H, frame=0)
    zc = float(s["lvd"][16, 16].view(np.float16))
    s["penumbra"][15, 15] = half_words(2.5 * zc * float(s["k"]["m_PixelUnproject"][0]))
    return s


def depth_step(W=32, H=32, at=16):
    """Lit left of column `at`, occluded with a wide penumbra from it on, and the surface steps away there: no tap across the step has weight."""
    s = flat(W, H, step_from=at)
    s["penumbra"][:, at:] = half_words(8.0)                                       # some 34 pixels where it is seen from: the cap holds it at 16
    return s


def sky_band(W=32, H=32):
    """depth_step without the step, and rows 10 to 13 sky with arbitrary penumbra and shadow data."""
    s = flat(W, H)
    s["penumbra"][:, 16:] = half_words(2.0)
    s["lvd"][10:14] = LIT
    s["penumbra"][10:14] = 0x0000
    return s
