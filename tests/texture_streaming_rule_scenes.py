"""The rule scenes of texture streaming (tests/test_texture_streaming_rule_scenes.py proves on the CPU that they tell a wrong feedback
or clamp rule apart; tests/test_gpu_texture_streaming_rules.py runs them on the GPU): six scenes of two quads over six texture shapes
whose regions are not 8 x 8, not square, and on textures whose sides are no powers of two.

Every scene is rendered at 80 x 56 and has two quads side by side over ONE texture, the left one through the wrap sampler (material 0)
and the right one through the clamp sampler (material 1), so that 8 x 8 pixel waves along the seam hold lanes of both.  The min-mip
map of a case is random in 0 .. levels + 2, with three bytes set to mips - 2, mips - 1 and mips: below, at and above mips - 1 in every
map.  Not a test module."""
import numpy as np

import bc_blocks as B
import material_texture_scenes as S
import texture_streaming_scenes as X

# (width, height, format, region): a full mip chain each
SHAPES = [(24, 40, S.RGBA8, (8, 4)), (24, 40, B.BC3, (4, 8)), (64, 32, S.SRGBA8, (16, 4)), (48, 16, B.BC1, (4, 16)), (32, 32, S.RGBA8, (4, 4)),
          (64, 64, S.RGBA8, (8, 4))]
SCENES = ("window", "far window", "tilted", "partial floor", "even taps", "aligned taps")
PIXELS_PER_UNIT = 40.0 / (np.tan(np.radians(22.5)) * (80.0 / 56.0) * 4.0)    # of S.view() at z = -4: 16.9 pixels per world unit


def shape_id(shape):
    w, h, fmt, (rw, rh) = shape
    return f"{w}x{h} format {fmt} regions {rw}x{rh}"


def _pair(make):
    """The quads of make(side, material) for the left (wrap) and the right (clamp) half."""
    return [make(-1.0, 0), make(1.0, 1)]


def quads(name):
    if name == "window":
        # magnified and rotated, uv inside (0.30, 0.62): the regions under the window and the ring a bilinear footprint reaches are
        # marked, the rest stay NEVER
        return _pair(lambda s, m: S.facing(z=-1.2, half=0.3, uv_lo=0.30, uv_hi=0.62, material=m, centre=(0.33 * s, 0.02 * s), world=X.turn(0.3)))
    if name == "far window":
        # minified: levels 1 and up are wanted, so a level texel's mip-0 origin x << level is not x
        return _pair(lambda s, m: S.facing(z=-6.0, half=0.85, uv_lo=0.1, uv_hi=0.8, material=m, centre=(0.95 * s, 0.1 * s), world=X.turn(0.25)))
    if name == "tilted":
        # two walls of constant height from z = -12 on the left to z = -2 on the right: the lod runs across the regions and falls along
        # the lanes of a wave's rows, so the first lane on a word is seldom the one with the lowest level
        return [S.quad((x0, -0.45, -12.0), (x0, 0.45, -12.0), (x1, -0.45, -2.0), (x1, 0.45, -2.0), (0.94, 0.06), (0.94, 0.94), (0.06, 0.06), (0.06, 0.94), m, grid=4,
                       normal=(1.0, 0.0, 0.2)) for x0, x1, m in ((-6.0, -0.1, 0), (0.4, 1.1, 1))]
    if name == "partial floor":
        # the grazing floor of S.floor over a part of the texture: the taps run far from the pixel's own uv
        return _pair(lambda s, m: S.quad((1.5 * s - 1.5, -0.6, -1.0), (1.5 * s + 1.5, -0.6, -1.0), (1.5 * s - 1.5, -0.6, -40.0), (1.5 * s + 1.5, -0.6, -40.0),
                                         (0.22, 0.07), (0.71, 0.07), (0.22, 0.9), (0.71, 0.9), m, grid=6, normal=(0.0, 1.0, 0.0)))
    if name == "even taps":
        # minified and denser in v than in u: an even number of taps on either side of uv and none at it, at a lod of 3 or more.  The
        # mip-0 origins of level-3 texels are multiples of 8, so on regions 4 texels wide or high every other region is reached by the
        # mark under uv alone.
        return _pair(lambda s, m: S.quad((1.3 * s - 1.2, -1.6, -4.0), (1.3 * s + 1.2, -1.6, -4.0), (1.3 * s - 1.2, 1.6, -4.0), (1.3 * s + 1.2, 1.6, -4.0),
                                         (-9.2, 39.0), (12.4, 39.0), (-9.2, -18.0), (12.4, -18.0), m, grid=2, world=X.turn(0.1)))
    assert name == "aligned taps", name
    # 24 x 32 whole pixels each, uv moving by 1 / 3 and 1 / 4 of the texture per pixel: two taps 4 / 3 level texels apart on the 32 x 32
    # and 64 x 64 textures (lod 2.4 and 3.4), six to a repeat of the texture, so that every repeat meets the texels in the same phase.
    # In this phase a tap's first level-l0w texel lies in the region its predecessor marked last, with l1w, and no other tap of the
    # scene marks it: the per-lane drop must let the lower level through (Marker::mark in csrc/material_textures.hip.h).
    def aligned(left, m, u0=0.578125, v0=0.203125):
        xl, xr, yt, yb = (left - 40) / PIXELS_PER_UNIT, (left - 16) / PIXELS_PER_UNIT, 16 / PIXELS_PER_UNIT, -16 / PIXELS_PER_UNIT
        return S.quad((xl, yb, -4.0), (xr, yb, -4.0), (xl, yt, -4.0), (xr, yt, -4.0), (u0, v0 + 8.0), (u0 + 8.0, v0 + 8.0), (u0, v0), (u0 + 8.0, v0), m, grid=2)
    return [aligned(12, 0), aligned(44, 1)]


def case(name, shape, seed=0):
    """(scene, materials, table under a random min-mip map, table under the zero map, where, textures) of one scene over one shape."""
    w, h, fmt, region = shape
    i = SHAPES.index(shape)
    textures = [X.texture(100 + 10 * i + seed, w, h, fmt, region=region)]
    levels = X.full_chain(w, h)
    mm = X.random_minmip(200 + 10 * i + SCENES.index(name), w, h, region=region, hi=levels + 3)
    spots = np.random.default_rng([i, SCENES.index(name)]).choice(mm.size, 3, replace=False)
    mm.reshape(-1)[spots] = (levels - 2, levels - 1, levels)                 # a map of 12 bytes may miss one of: below, at, above mips - 1
    table, where = X.with_maps(textures, minmips={0: mm})
    zero, where0 = X.with_maps(textures)
    assert where == where0, "the two tables have the same layout"
    mats = np.concatenate([X.material(where, S.ALBEDO, (0, S.NONE, S.NONE, S.NONE)), X.material(where, S.ALBEDO, (0, S.NONE, S.NONE, S.NONE), wrap=(0, 0, 0, 0))])
    return S.build(quads(name)), mats, table, zero, where, textures


def plain_materials():
    """The two materials without a map index: what the #textured kernel reads."""
    return np.concatenate([S.material(flags=S.ALBEDO, indices=(0, S.NONE, S.NONE, S.NONE)), S.material(flags=S.ALBEDO, indices=(0, S.NONE, S.NONE, S.NONE), wrap=(0, 0, 0, 0))])
