"""Scenes, textures and materials for the alpha-test tests (tests/test_alpha_test_ref.py on the CPU, tests/test_gpu_alpha_test.py on
the GPU): quads of tests/material_texture_scenes.py, each its own instance, mesh and meshlet, in front of synth.make_view()'s
camera at 96 x 80 pixels -- not a multiple of the raster's 64-pixel tile, so there are partial tiles and a tile border inside the
picture.

A scene is a dict with everything both drivers and all references need: instances, meshData (bounding spheres, LOD 0, the global
vertex and index offsets), meshlets (bounding spheres), opaqueIds, alphaMaskIds, vertices, vertexIds, triangles, indices and
index_counts (the ray tracing's index buffer: the meshlet's triangles again), materials, textures, and records / list (one record
per instance, every meshlet visible) for references that draw without a cull."""
import numpy as np

import material_texture_scenes as S
from toyrenderer_amd import interop as I

RENDER = (96, 80)
F = np.float32
CUTOFF = 0.5
CHECKER, NPOT, UNIFORM = 0, 1, 2                   # descriptor indices of textures()
# material indices of materials()
M_WALL, M_CHECKER, M_NPOT_WRAP, M_NPOT_CLAMP, M_UNIFORM, M_CONST_ABOVE, M_CONST_BELOW = range(7)


def checker_image(lo=30, hi=230):
    """8 x 8 texels, cells of 2 x 2 texels with alpha `lo` and `hi`: level 1 is still a checker, level 2 and 3 are its mean."""
    img = np.zeros((8, 8, 4), np.uint8)
    img[..., :3] = (200, 150, 100)
    y, x = np.mgrid[0:8, 0:8]
    img[..., 3] = np.where(((x // 2) + (y // 2)) % 2 == 0, hi, lo)
    return img


def uniform_image(alpha, size=4):
    img = np.full((size, size, 4), 255, np.uint8)
    img[..., 3] = alpha
    return img


def textures(checker=None, npot=None, uniform=200):
    """The table, as (mips, format): 0 the 8 x 8 checker with its full mip chain (sRGB: alpha stays linear), 1 a 5 x 3 texture of
    independent random bytes in each of its three levels (a wrong level shows), 2 a 4 x 4 texture of uniform alpha, one level."""
    c = I.make_mips(checker_image() if checker is None else checker, True)
    n = S.random_mips(21, 5, 3, 3) if npot is None else npot
    return [(c, S.SRGBA8), (n, S.RGBA8), ([uniform_image(uniform)], S.RGBA8)]


def with_uniform_alpha(tex, alpha):
    """The same table with every alpha byte of every level replaced."""
    out = []
    for mips, fmt in tex:
        mips = [m.copy() for m in mips]
        for m in mips:
            m[..., 3] = alpha
        out.append((mips, fmt))
    return out


def materials(cutoff=CUTOFF):
    m = np.concatenate([S.material(),                                                                              # the wall: opaque list
                        S.material(flags=S.ALBEDO, albedo=(0.9, 0.8, 0.7, 1.0), indices=(CHECKER, S.NONE, S.NONE, S.NONE)),
                        S.material(flags=S.ALBEDO, albedo=(0.5, 0.9, 0.6, 1.0), indices=(NPOT, S.NONE, S.NONE, S.NONE), wrap=(1, 1, 1, 1)),
                        S.material(flags=S.ALBEDO, albedo=(0.5, 0.6, 0.9, 1.0), indices=(NPOT, S.NONE, S.NONE, S.NONE), wrap=(0, 1, 1, 1)),
                        S.material(flags=S.ALBEDO, albedo=(0.7, 0.7, 0.7, 0.75), indices=(UNIFORM, S.NONE, S.NONE, S.NONE)),   # 0.75 * 200 / 255 = 0.588
                        S.material(albedo=(0.2, 0.9, 0.2, 0.75)),                                                    # texture-free, above the cutoff
                        S.material(albedo=(0.9, 0.2, 0.2, 0.25))])                                                   # texture-free, below it
    m["m_AlphaCutoff"] = cutoff
    return m


def quads():
    """[(quad, "opaque" | "alpha")].  Pixels per unit at z = -3: 32.2; the screen's centre is (48, 40).
    Through the queue, the bin and the tile launch (bounding boxes above 1024 pixels, straddling x = 64):
      the wall (opaque, the whole screen); a face-on checker of 45 x 45 pixels; a floor strip seen at a grazing angle, of the
      other winding, whose near cells are large and whose far cells are small (anisotropic and minified lookups).
    Drawn in place by the main launch (at most 1024 pixels):
      face-on quads of 19 x 19 pixels with the 5 x 3 texture under the wrap and the clamp sampler (uv beyond [0, 1]), the uniform
      texture, constant alpha above and below the cutoff; a steeply oblique checker of the other winding; the floor's far cells."""
    q = [(S.facing(z=-6.0, half=3.3, uv_lo=0.0, uv_hi=1.0, material=M_WALL, grid=1), "opaque"),
         (S.facing(z=-3.0, half=0.7, uv_lo=0.0, uv_hi=2.0, material=M_CHECKER, grid=1, centre=(0.45, 0.3)), "alpha"),
         # corners given with p10 and p01 exchanged: the other winding
         (S.quad((0.1, -0.6, -1.5), (0.1, -0.6, -12.0), (1.4, -0.6, -1.5), (1.4, -0.6, -12.0), (0.0, 0.0), (0.0, 6.0), (1.0, 0.0), (1.0, 6.0),
                 M_CHECKER, grid=2, normal=(0.0, 1.0, 0.0)), "alpha"),
         (S.facing(z=-3.0, half=0.3, uv_lo=-1.5, uv_hi=2.5, material=M_NPOT_WRAP, grid=1, centre=(-0.9, 0.6)), "alpha"),
         (S.facing(z=-3.0, half=0.3, uv_lo=-1.5, uv_hi=2.5, material=M_NPOT_CLAMP, grid=2, centre=(-0.9, -0.1)), "alpha"),
         (S.facing(z=-3.0, half=0.3, uv_lo=0.0, uv_hi=1.0, material=M_UNIFORM, grid=1, centre=(-0.9, -0.8)), "alpha"),
         (S.facing(z=-3.0, half=0.2, uv_lo=0.0, uv_hi=1.0, material=M_CONST_ABOVE, grid=1, centre=(-0.25, 0.9)), "alpha"),
         (S.facing(z=-3.0, half=0.2, uv_lo=0.0, uv_hi=1.0, material=M_CONST_BELOW, grid=1, centre=(-0.25, 0.4)), "alpha"),
         (S.quad((-0.6, -0.5, -2.5), (-0.6, 0.1, -2.5), (-0.1, -0.5, -5.0), (-0.1, 0.1, -5.0), (0.0, 1.0), (0.0, 0.0), (3.0, 1.0), (3.0, 0.0),
                 M_CHECKER, grid=1, normal=(1.0, 0.0, 0.5)), "alpha"),
         # opaque, behind the face-on checker and seen through its holes: hidden from the next frame's early cull only if the HZB
         # was built from solid cards
         (S.facing(z=-4.0, half=0.25, uv_lo=0.0, uv_hi=1.0, material=M_WALL, grid=1, centre=(0.6, 0.4)), "opaque")]
    return q


BEHIND_THE_CHECKER = 9                             # the instance index of that last quad


def build(placed, mats=None, tex=None):
    """The scene dict of [(quad, "opaque" | "alpha")]."""
    qs = [q for q, _ in placed]
    sc, v, vid, tri, rec, lst = S.build(qs)
    md, ml = sc["meshData"], sc["meshlets"]
    indices, counts = [], np.zeros(len(qs), np.uint32)
    for i in range(len(qs)):
        first, nv = int(ml["m_MeshletVertexIDsBufferIdx"][i]), int(ml["m_VertexAndTriangleCount"][i]) & 0xFF
        nt = (int(ml["m_VertexAndTriangleCount"][i]) >> 8) & 0xFF
        p = v["m_Position"][first:first + nv].astype(np.float64)
        c = 0.5 * (p.min(0) + p.max(0))
        sphere = (*c, 1.01 * np.linalg.norm(p - c, axis=1).max() + 1e-4)
        md["m_BoundingSphere"][i] = ml["m_BoundingSphere"][i] = sphere
        t = tri[int(ml["m_MeshletIndexIDsBufferIdx"][i]):][:nt]
        md["m_GlobalVertexBufferIdx"][i], md["m_GlobalIndexBufferIdx"][i] = first, 3 * sum(len(x) for x in indices)
        counts[i] = 3 * nt
        indices.append(np.stack([t & 0xFF, (t >> 8) & 0xFF, (t >> 16) & 0xFF], 1).astype(np.uint32))
    return dict(instances=sc["instances"], meshData=md, meshlets=ml, vertices=v, vertexIds=vid, triangles=tri, records=rec, list=lst,
                opaqueIds=np.array([i for i, (_, w) in enumerate(placed) if w == "opaque"], np.uint32),
                alphaMaskIds=np.array([i for i, (_, w) in enumerate(placed) if w == "alpha"], np.uint32),
                indices=np.concatenate(indices).reshape(-1), index_counts=counts,
                materials=materials() if mats is None else mats, textures=textures() if tex is None else tex)


def standard(mats=None, tex=None):
    return build(quads(), mats, tex)


def without_alpha_instances(sc):
    out = dict(sc)
    out["alphaMaskIds"] = np.zeros(0, np.uint32)
    return out


def tie_scene(cutoff):
    """The wall and one face-on quad with the uniform texture of alpha byte 128, constant alpha 1 and the given cutoff.  The texture
    has one level, so lod = 0; the quad faces the camera and its texture is square, so the two footprint axes differ by rounding
    alone and N = ceil(Pmax / Pmin) is 1 or 2: a sum of one or two equal values divided by their count is exact, and the sampled
    alpha is (float)128 / 255.0f in every covered sample."""
    m = materials()
    m["m_ConstAlbedo"][M_UNIFORM, 3] = 1.0
    m["m_AlphaCutoff"][M_UNIFORM] = cutoff
    placed = [quads()[0], (S.facing(z=-3.0, half=0.8, uv_lo=0.0, uv_hi=1.0, material=M_UNIFORM, grid=1, centre=(0.3, -0.1)), "alpha")]
    return build(placed, m, textures(uniform=128))


TIE = F(128) / F(255)


def shadow_scene():
    """The checker cut-out above a floor: an opaque floor at y = -0.6 and, one and a half units above it, a horizontal alpha-mask quad with the
    checker (3 x 3 repeats), both in view."""
    floor = S.quad((-3.0, -0.6, -1.0), (3.0, -0.6, -1.0), (-3.0, -0.6, -14.0), (3.0, -0.6, -14.0), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0),
                   M_WALL, grid=2, normal=(0.0, 1.0, 0.0))
    cut = S.quad((-1.6, 0.9, -2.5), (1.6, 0.9, -2.5), (-1.6, 0.9, -9.0), (1.6, 0.9, -9.0), (0.0, 0.0), (3.0, 0.0), (0.0, 3.0), (3.0, 3.0),
                 M_CHECKER, grid=2, normal=(0.0, 1.0, 0.0))
    return build([(floor, "opaque"), (cut, "alpha")])


def view(render=RENDER):
    return S.view(render=render)
