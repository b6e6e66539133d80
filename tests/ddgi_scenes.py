"""Seeded inputs of the DDGI tests (tests/test_ddgi_ref.py on the CPU, tests/test_gpu_ddgi.py on the GPU): two probe volumes in
front of the lighting tests' camera, and a depth image whose surfaces lie inside, at the faded rim of and outside them."""
import numpy as np

from toyrenderer_amd import ddgi
from toyrenderer_amd import interop as I

import lighting_scenes as LS

F = np.float32
W, H = 64, 32                                   # the synthetic G-buffer's size (one tile row of 64 and more than one block)
NEAR = F(0.1)                                   # synth.make_view's near plane: depth = near / view-space z


def centre(clip_to_world, z=2.2):
    """World position of the image centre at view depth z (float64 from the float32 matrix)."""
    h = np.array([0.0, 0.0, float(NEAR) / z, 1.0]) @ np.asarray(clip_to_world, np.float64).reshape(4, 4)
    return h[:3] / h[3]


def depth_image(seed):
    """float32 [H, W]: surfaces at view depth 0.6 .. 4.5 in front of the camera, a few unwritten texels (0, -0, NaN, -1) and a
    few so far away that they are outside any volume."""
    rng = np.random.default_rng(seed + 500)
    z = rng.uniform(0.6, 4.5, (H, W))
    d = (NEAR / z.astype(F)).astype(F)
    flat = d.reshape(-1)
    flat[4:8] = np.array([0.0, -0.0, np.nan, -1.0], F)
    flat[8:12] = np.array([1e-4, 3e-5, 1e-6, 1e-40], F)
    return d


# name -> (counts, spacing, offset of the volume's origin from the image centre at depth 2.2, in units of the spacing)
VOLUMES = {"2x2x2": ((2, 2, 2), (1.3, 1.1, 1.2), (0.11, -0.07, 0.13)),
           "3x2x4": ((3, 2, 4), (0.83, 1.17, 0.71), (-0.09, 0.12, 0.07))}


def volume(name, clip_to_world, seed=7):
    """Random irradiance (borders filled), distances around the true probe-to-surface distances (so the Chebyshev test goes both
    ways), relocation offsets on about 40 % of the probes, 30 % inactive probes; in "3x2x4" the eight probes of cell (0, 0, 0) are
    all inactive, so that surfaces in it find no probe at all."""
    counts, spacing, shift = VOLUMES[name]
    rng = np.random.default_rng(seed + sum(counts))
    origin = centre(clip_to_world) + np.asarray(shift) * np.asarray(spacing)
    v = ddgi.Volume(origin, spacing, counts, normal_bias=0.02, view_bias=0.1, gamma=5.0, relocation=True, classification=True)
    cx, cy, cz = counts
    v.irradiance[...] = ddgi.pack_unorm10(rng.uniform(0.15, 1.0, v.irradiance.shape + (3,)))
    mean = rng.uniform(0.25, 1.3, v.distance.shape[:-1]) * float(np.mean(spacing))
    v.distance[..., 0] = (mean * 0.5).astype(np.float16)
    v.distance[..., 1] = (mean * mean * rng.uniform(1.0, 1.6, mean.shape) * 0.5).astype(np.float16)
    moved = rng.random((cy, cz, cx)) < 0.4
    v.data[..., :3] = np.where(moved[..., None], rng.uniform(-0.3, 0.3, (cy, cz, cx, 3)), 0.0).astype(np.float16)
    inactive = rng.random((cy, cz, cx)) < 0.3
    if name == "3x2x4":
        inactive[0:2, 0:2, 0:2] = True
    v.data[..., 3] = inactive.astype(np.float16)
    return v.fill_borders()


def images(seed=11):
    """(clip_to_world, eye, gbuffer, depth, motion, ssao, shadow) of the synthetic G-buffer."""
    m, eye = LS.camera((W, H))
    return m, eye, LS.gbuffer_image(W, H, seed), depth_image(seed), LS.motion_image(W, H, seed), LS.byte_image(W, H, seed), LS.byte_image(W, H, seed + 1)
