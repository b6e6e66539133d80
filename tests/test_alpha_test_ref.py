"""The alpha-test reference against itself and against an independent restatement (tests/alpha_test_ref.c): no GPU.

What is checked here are properties the definition must have whatever its arithmetic (an opaque texture changes nothing, a
transparent one removes the instances, the comparison is `alpha < cutoff` exactly), the sampler against numpy, and a CONDITION ON
THE SCENES of tests/alpha_test_scenes.py: the discard fires on a good share of the samples and spares a good share, on the main
path and on the tile path separately -- a test whose discard never fires, or always fires, shows nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import alpha_test_ref as AT  # noqa: E402
import alpha_test_scenes as A  # noqa: E402
import material_textures_ref as MT  # noqa: E402
from suite_support import at, vr  # noqa: E402, F401
import visibility_ref as VR  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import consts  # noqa: E402

F = np.float32


def render(at, sc, alpha_test=True, textures="scene", with_alpha_instances=True):
    """(depth words, vis, counts) of the scene drawn without a cull: the opaque instances as slot 0, the alpha-mask ones as slot 2."""
    W, H = A.RENDER
    k = consts(A.view())
    geo = VR.Geometry(sc, sc["vertices"], sc["vertexIds"], sc["triangles"])
    depth, vis, counts = np.zeros((H, W), F), np.zeros((H, W), np.uint64), np.zeros(4, np.uint64)
    tex = sc["textures"] if isinstance(textures, str) else textures
    for slot, ids in ((0, sc["opaqueIds"]), (2, sc["alphaMaskIds"] if with_alpha_instances else [])):
        if len(ids):
            counts += AT.raster(at, k, geo, sc["records"], np.asarray(ids, np.uint32) << 5, slot, depth, vis, sc["materials"], tex, alpha_test and slot == 2)
    return depth.view(np.uint32), vis, counts


def test_without_the_test_the_reference_is_the_visibility_reference(at, vr):
    sc = A.standard()
    W, H = A.RENDER
    k = consts(A.view())
    geo = VR.Geometry(sc, sc["vertices"], sc["vertexIds"], sc["triangles"])
    depth, vis = np.zeros((H, W), F), np.zeros((H, W), np.uint64)
    VR.raster(vr, k, geo, sc["records"], sc["opaqueIds"] << 5, 0, depth, vis)
    VR.raster(vr, k, geo, sc["records"], sc["alphaMaskIds"] << 5, 2, depth, vis)
    d, v, counts = render(at, sc, alpha_test=False)
    assert np.array_equal(d, depth.view(np.uint32)) and np.array_equal(v, vis) and not counts.any()
    _, slot, _, _ = VR.decode(v)
    assert (v != 0).all() and (slot == 2).sum() > 1500, "the wall fills the screen, the alpha-mask quads cover a good part of it"


def test_an_opaque_texture_changes_nothing(at):
    """All alpha bytes 255, constant alpha 1, cutoff 0.5: every word equals the run without the test."""
    mats = A.materials()
    mats["m_ConstAlbedo"][:, 3] = 1.0
    sc = A.standard(mats, A.with_uniform_alpha(A.textures(), 255))
    d0, v0, _ = render(at, sc, alpha_test=False)
    d1, v1, counts = render(at, sc, alpha_test=True)
    assert np.array_equal(d0, d1) and np.array_equal(v0, v1)
    assert counts[0] > 500 and counts[2] > 1000 and counts[1] == counts[3] == 0


def test_a_transparent_texture_removes_the_instances(at):
    """All alpha bytes 0 (and the texture-free materials below the cutoff): every word equals the scene without the alpha-mask
    instances."""
    mats = A.materials()
    mats["m_ConstAlbedo"][[A.M_CONST_ABOVE, A.M_CONST_BELOW], 3] = 0.25
    sc = A.standard(mats, A.with_uniform_alpha(A.textures(), 0))
    d0, v0, _ = render(at, sc, with_alpha_instances=False)
    d1, v1, counts = render(at, sc)
    assert np.array_equal(d0, d1) and np.array_equal(v0, v1)
    assert counts[0] == counts[2] == 0 and counts[3] > 1000, counts      # texture-free triangles are dropped whole and not counted


def test_the_tie_is_kept_and_the_next_cutoff_discards(at):
    """alpha == cutoff is kept (discard iff alpha < cutoff); with the next float above as the cutoff the quad vanishes whole."""
    kept = A.tie_scene(A.TIE)
    gone = A.tie_scene(np.nextafter(A.TIE, F(1)))
    d_solid, v_solid, _ = render(at, kept, alpha_test=False)
    d_wall, v_wall, _ = render(at, kept, with_alpha_instances=False)
    d1, v1, c1 = render(at, kept)
    d2, v2, c2 = render(at, gone)
    assert np.array_equal(d1, d_solid) and np.array_equal(v1, v_solid) and c1[1] == c1[3] == 0 and c1[2] > 2000
    assert np.array_equal(d2, d_wall) and np.array_equal(v2, v_wall) and c2[0] == c2[2] == 0 and c2[3] == c1[2]


@pytest.mark.parametrize("scene", ["standard", "shadow"])
def test_condition_on_the_scenes_the_discard_fires_and_spares(at, scene):
    """At least a tenth of the samples covered by alpha-mask triangles are kept and at least a tenth discarded, on the main path
    (bounding boxes of at most 1024 pixels) and on the tile path separately; both paths are well populated."""
    sc = A.standard() if scene == "standard" else A.shadow_scene()
    _, vis, counts = render(at, sc)
    main, tiles = counts[:2].astype(np.int64), counts[2:].astype(np.int64)
    least = 1000 if scene == "standard" else 250                         # the shadow scene's cut-out is seen from below, at a grazing angle
    assert main.sum() > least and tiles.sum() > least, counts
    assert main.min() * 10 >= main.sum(), counts
    assert tiles.min() * 10 >= tiles.sum(), counts
    if scene == "standard":
        _, slot, pos, _ = VR.decode(vis)
        owners = set(np.unique(sc["alphaMaskIds"][pos[(vis != 0) & (slot == 2)]]).tolist())     # list position -> instance (one meshlet each)
        assert owners == set(sc["alphaMaskIds"].tolist()) - {7}, "every alpha-mask quad shows but the one below the cutoff"
        xs = np.nonzero(((vis != 0) & (slot == 2)).any(0))[0]
        assert xs.min() < 64 <= xs.max()


def test_condition_on_the_scene_the_hzb_shows_whether_the_cards_were_solid(oracle, at):
    """Frame 2 of the standard scene with occlusion culling.  The opaque quad behind the face-on checker passes the early cull
    when the HZB was built from the alpha-tested depth (it is seen through the holes) and only the late cull when the cards were
    solid: its texels carry another pass slot, so a frame whose HZB came from the wrong depth differs from the reference."""
    sc = A.standard()
    drawn_by = []
    for alpha_test in (True, False):
        _, (ref, vis, _) = AT.frames(oracle, at, sc, A.view(), 3, alpha_test)
        lists = [ref.records[s]["instanceConstIdx"][ref.visibleList[s] >> 5].tolist() for s in range(4)]
        drawn_by.append([s for s in range(4) if A.BEHIND_THE_CHECKER in lists[s]])
        if alpha_test:
            _, slot, pos, _ = VR.decode(vis)
            early = (vis != 0) & (slot == 0)
            assert (np.asarray(lists[0])[pos[early]] == A.BEHIND_THE_CHECKER).sum() > 30, "the quad shows through the holes"
    assert drawn_by == [[0], [1]], drawn_by


# ---- the sampler against numpy ----------------------------------------------------------------------------------------------------
_LOG2C = [F(float.fromhex(x)) for x in ("0x1.715476p+0", "-0x1.715470p-1", "0x1.ec70aap-2", "-0x1.715a70p-2", "0x1.277a52p-2",
                                         "-0x1.eab7a8p-3", "0x1.a38c64p-3", "-0x1.87f6aap-3", "0x1.7a63c4p-3", "-0x1.b84fe0p-4")]


def _log2(x):
    """log2Soft of csrc/soft_math.hip.h for a positive finite x."""
    u = int(np.array([x], F).view(np.uint32)[0])
    bias = -127
    if u < 0x00800000:
        u, bias = int(np.array([F(x) * F(2.0 ** 24)], F).view(np.uint32)[0]), -151
    u += 0x3F800000 - 0x3F3504F3
    k = (u >> 23) + bias
    f = np.array([(u & 0x007FFFFF) + 0x3F3504F3], np.uint32).view(F)[0] - F(1)
    p = _LOG2C[9]
    for j in range(8, -1, -1):
        p = I.fmaf(p, f, _LOG2C[j])
    return I.fmaf(f, p, F(k))


def _axis(u, dim, wrap):
    t = F(F(u) * F(dim)) - F(0.5)
    t0 = np.floor(t)
    f = F(t - t0)
    if not wrap:
        return int(min(max(t0, 0), dim - 1)), int(min(max(t0 + 1, 0), dim - 1)), f
    r = int(min(max(t0, -2.0 ** 30), 2.0 ** 30)) % dim
    return r, (r + 1) % dim, f


def _bilinear(level, wrap, u, v):
    h, w = level.shape
    x0, x1, fx = _axis(u, w, wrap)
    y0, y1, fy = _axis(v, h, wrap)
    t = lambda y, x: F(F(level[y, x]) / F(255))                                                  # noqa: E731
    lerp = lambda a, b, s: F(a + F(s * F(b - a)))                                                # noqa: E731
    return lerp(lerp(t(y0, x0), t(y0, x1), fx), lerp(t(y1, x0), t(y1, x1), fx), fy)


def _sample_alpha(mips, wrap, uv, dx, dy):
    """The convention of csrc/material_textures.hip.h on the alpha bytes, in numpy float32 scalars."""
    alpha = [m[..., 3] for m in mips]
    H, W = alpha[0].shape
    ax, ay, bx, by = F(dx[0] * F(W)), F(dx[1] * F(H)), F(dy[0] * F(W)), F(dy[1] * F(H))
    lenA, lenB = np.sqrt(I.fmaf(ay, ay, F(ax * ax))), np.sqrt(I.fmaf(by, by, F(bx * bx)))
    major, pmax, pmin = (dx, lenA, lenB) if lenA >= lenB else (dy, lenB, lenA)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.ceil(F(pmax / pmin))
    N = int(n) if n <= 16 else 16
    x = F(pmax / F(N))
    lod = F(min(max(_log2(x) if x > 0 else F(0), F(0)), F(len(mips) - 1)))
    l0 = int(np.floor(lod))
    f, l1 = F(lod - F(l0)), min(l0 + 1, len(mips) - 1)
    acc = F(0)
    for i in range(N):
        k = F(F(F(i) + F(0.5)) / F(N)) - F(0.5)
        u, v = F(uv[0] + F(major[0] * k)), F(uv[1] + F(major[1] * k))
        b0, b1 = _bilinear(alpha[l0], wrap, u, v), _bilinear(alpha[l1], wrap, u, v)
        acc = F(acc + F(b0 + F(f * F(b1 - b0))))
    return F(acc / F(N)), N, lod


def test_sample_alpha_equals_a_numpy_restatement_on_a_seeded_batch(at):
    """600 lookups over the three textures, both samplers, uv in [-2, 3], footprints from far below a texel to far beyond the
    texture, isotropic to 40 : 1: every bit equal, every tap count from 1 to 16 and every level taken."""
    rng = np.random.default_rng(20)
    tex = [MT.Texture(*t) for t in A.textures()]
    seen_n, seen_l = set(), set()
    for i in range(600):
        t = tex[i % 3]
        wrap = (i // 3) % 2
        uv = rng.uniform(-2, 3, 2).astype(F)
        scale, ratio, ang = 10.0 ** rng.uniform(-2.5, 0.5), rng.uniform(1.0, 40.0) if i % 4 else 1.0, rng.uniform(0, 6.28)
        dx = (np.array([np.cos(ang), np.sin(ang)]) * scale).astype(F)
        dy = (np.array([-np.sin(ang), np.cos(ang)]) * scale / ratio).astype(F)
        if i % 7 == 0:
            dx, dy = dy, dx
        want, N, lod = _sample_alpha(t.mips, wrap, uv, dx, dy)
        got = AT.sample_alpha(at, t, wrap, uv, dx, dy)
        assert got.tobytes() == want.tobytes(), (i, got, want, N, lod)
        level0 = AT.alpha_level0(at, t, wrap, uv[0], uv[1])
        assert level0.tobytes() == _bilinear(t.mips[0][..., 3], wrap, uv[0], uv[1]).tobytes(), i
        seen_n.add(N); seen_l.add(int(np.floor(lod)))
    assert seen_n == set(range(1, 17)) and seen_l >= {0, 1, 2, 3}, (seen_n, seen_l)


def test_alpha_is_linear_in_both_formats(at):
    """The same bytes as RGBA8_UNORM and as SRGBA8_UNORM give the same alpha."""
    mips = A.textures()[A.CHECKER][0]
    a, b = MT.Texture(mips, MT.FORMAT_RGBA8), MT.Texture(mips, MT.FORMAT_SRGBA8)
    uv, dx, dy = np.array([0.3, 0.7], F), np.array([0.11, 0.02], F), np.array([-0.01, 0.05], F)
    assert AT.sample_alpha(at, a, 1, uv, dx, dy) == AT.sample_alpha(at, b, 1, uv, dx, dy) != 0
