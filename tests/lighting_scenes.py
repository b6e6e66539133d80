"""Seeded inputs of the deferred lighting tests (tests/test_lighting_ref.py on the CPU, tests/test_gpu_lighting.py on the GPU):
GBufferA words, depth, motion, shadow and SSAO images, cameras and lights."""
import numpy as np

from toyrenderer_amd import interop as I
from toyrenderer_amd import synth

F = np.float32


def camera(render, eye=(0.3, 1.2, 2.0), yaw=0.35):
    """(m_ClipToWorld, eye) of a real camera: the float64 inverse of WorldToView * ViewToClip rounded once."""
    v = synth.make_view(eye=eye, yaw=yaw, render=render)
    return I.clip_to_world(v.worldToView, v.viewToClip), np.asarray(eye, F)


def degenerate_clip_to_world(render):
    """A camera's matrix with a zero last column: w = 0 for every pixel, so worldPosition divides by zero."""
    m, eye = camera(render)
    m = m.copy()
    m[:, 3] = 0
    return m, eye


def gbuffer_image(W, H, seed, roughness_metallic_ramp=False):
    """uint32 [H, W, 4]: random albedo / debug bytes; normal words random with 0 and 0xFFFFFFFF among them; emissive words
    random with exponent 31 among them (and word 0 for most texels, so that the light shows); w = roughness | metallic << 8,
    random bytes, or roughness = x and metallic = y with roughness_metallic_ramp."""
    rng = np.random.default_rng(seed)
    g = np.zeros((H, W, 4), np.uint32)
    g[..., 0] = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    g[..., 1] = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    e = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    g[..., 2] = np.where(rng.random((H, W)) < 0.5, 0, e)
    flat = g.reshape(-1, 4)
    n = len(flat)
    flat[0 % n, 1] = 0
    flat[1 % n, 1] = 0xFFFFFFFF
    flat[2 % n, 2] = 0xFFFFFFFF                      # exponent 31, every mantissa bit
    flat[3 % n, 2] = (31 << 27) | 1
    if roughness_metallic_ramp:
        g[..., 3] = np.arange(W, dtype=np.uint32)[None, :] & 0xFF | (np.arange(H, dtype=np.uint32)[:, None] & 0xFF) << 8
    else:
        g[..., 3] = rng.integers(0, 1 << 16, (H, W), dtype=np.uint64).astype(np.uint32)
    return g


def depth_image(W, H, seed):
    """float32 [H, W]: random in (0, 1], with 0, -0, NaN, +inf, -1, a subnormal and a negative NaN among the first texels
    (row-major, as far as the image has that many)."""
    rng = np.random.default_rng(seed + 1000)
    d = (F(1.0) - rng.random((H, W), dtype=F)).astype(F)
    special = np.array([0.0, -0.0, np.nan, np.inf, -1.0, 1e-40, -np.inf], F)
    flat = d.reshape(-1)
    if len(flat) > 4:
        k = min(len(special), len(flat) - 4)
        flat[4:4 + k] = special[:k]
    return d


def motion_image(W, H, seed):
    """float16 [H, W, 2] in pixels, with inf, NaN, -0 and a subnormal among them."""
    rng = np.random.default_rng(seed + 2000)
    m = rng.normal(0.0, 20.0, (H, W, 2)).astype(np.float16)
    flat = m.reshape(-1)
    special = np.array([np.inf, np.nan, -0.0, 6e-8, -np.inf, 65504.0], np.float16)
    if len(flat) > 12:
        flat[6:6 + len(special)] = special
    return m


def byte_image(W, H, seed):
    """uint8 [H, W]: every byte value as far as the image has texels, then random."""
    rng = np.random.default_rng(seed + 3000)
    b = rng.integers(0, 256, (H, W), dtype=np.uint64).astype(np.uint8)
    flat = b.reshape(-1)
    k = min(256, len(flat))
    flat[-k:] = np.arange(k, dtype=np.uint8)
    return b


LIGHTS = (("unit", (0.0, -1.0, 0.0)), ("unit oblique", tuple(float(x) for x in (np.array([1.0, -2.0, 0.5]) / np.sqrt(5.25)).astype(F))),
          ("non-unit", (0.3, -2.5, 1.0)), ("zero", (0.0, 0.0, 0.0)), ("NaN", (0.5, float("nan"), -0.5)))
STRENGTHS = (0.0, 1.0, 1.0e4, float("inf"))
SIZES = ((1, 1), (16, 16), (67, 35), (129, 3))
SENTINEL = 0xDEADBEEF
