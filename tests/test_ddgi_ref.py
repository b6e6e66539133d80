"""CPU tests of tests/ddgi_ref.c, the reference of the DDGI ambient term (csrc/ddgi_irradiance.hip.h), and of toyrenderer_amd/
ddgi.py: the closed form of a uniform volume, the octahedral borders, the float64 restatement, the branches the test scenes
reach, the descriptor's layout and the declarations.  tests/test_gpu_ddgi.py compares the kernel with the same reference."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_ref as DR  # noqa: E402
import ddgi_scenes as DS  # noqa: E402
import lighting_ref as LR  # noqa: E402
from ref_build import layout_probe  # noqa: E402
from suite_support import dg  # noqa: E402, F401
from toyrenderer_amd import ddgi  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# The float64 check's relative bound: twice the maximum measured over the two test scenes (4.51e-5 on "3x2x4", 2.00e-5 on
# "2x2x2").  The pass chains two software transcendental functions, cubes the Chebyshev ratio and cubes a crushed
# weight, so an input rounding reaches the result about tenfold.
FLOAT64_BOUND = 9.1e-5
LEFT_OUT_CAP = 0.01                              # at most 1 % of the lit pixels may decide a branch differently in float64


@pytest.fixture(scope="module")
def scenes(dg):
    """Per volume: the reference's pass over the synthetic G-buffer, computed once."""
    m, eye, g, depth, motion, ssao, shadow = DS.images()
    k = LR.consts(m, eye, (0.3, -2.5, 1.0), 2.0, (DS.W, DS.H))
    k["m_bRTDDGIEnabled"] = 1
    out = {}
    for name in DS.VOLUMES:
        vol = DS.volume(name, m)
        words, extra = DR.lighting(dg, k, vol, g, depth, want=("irr", "traces", "counters"))
        world, normal, _ = DR.inputs(dg, k, g, depth)
        out[name] = dict(vol=vol, words=words, eye=eye, lit=depth > 0, world=world, normal=normal, **extra)
    return out


# ---- closed form ------------------------------------------------------------------------------------------------------------
def _uniform(texel=(600, 900, 300), counts=(3, 2, 4), spacing=(1.0, 0.5, 2.0)):
    v = ddgi.Volume.uniform((0.25, -1.0, 3.0), spacing, counts, normal_bias=0.02, view_bias=0.1)
    v.irradiance[...] = texel[0] | texel[1] << 10 | texel[2] << 20
    return v


def _closed_form(dg, vol, texel, blend):
    e = DR.pow_soft(dg, np.asarray(texel, F) / F(1023.0), F(vol.gamma) * F(0.5)).astype(np.float64)
    return e * e * (2 * math.pi) * 1.0989 * blend


def test_uniform_volume_closed_form(dg):
    """Every irradiance texel stores c and every distance is huge: the result is (c^(gamma/2))^2 * 2 pi * 1.0989 * blend whatever
    the eight weights are (c^(gamma/2) the reference's own pow).  Eight rounded products, their sums and one division, then three
    more products: relative error at most 2^-20."""
    texel = (600, 900, 300)
    vol = _uniform(texel)
    rng = np.random.default_rng(3)
    ext = np.asarray(vol.spacing) * (np.asarray(vol.counts) - 1) * 0.5
    world = (np.asarray(vol.origin) + rng.uniform(-0.999, 0.999, (4096, 3)) * ext).astype(F)
    normal = rng.normal(size=(4096, 3))
    normal = (normal / np.linalg.norm(normal, axis=1)[:, None]).astype(F)
    irr, tr = DR.irradiance(dg, vol, world, normal, (5.0, 2.0, -3.0))
    assert np.all(tr["inside"] == 1) and np.all(tr["chebMask"] == 0)
    want = _closed_form(dg, vol, texel, 1.0)
    rel = np.abs(irr.astype(np.float64) - want) / want
    print("uniform volume, 4096 points inside: max relative error 2^%.2f" % math.log2(rel.max()))
    assert rel.max() <= 2.0 ** -20


def test_uniform_volume_outside_and_fade(dg):
    """Outside the volume: exactly 0 from one spacing past the face on; half a spacing past it, half the inside value."""
    texel = (600, 900, 300)
    vol = _uniform(texel)
    org, sp = np.asarray(vol.origin, np.float64), np.asarray(vol.spacing, np.float64)
    ext = sp * (np.asarray(vol.counts) - 1) * 0.5
    n = np.array([0.0, 1.0, 0.0], F)
    inside = _closed_form(dg, vol, texel, 1.0)
    for axis in range(3):
        for sign in (-1.0, 1.0):
            step = np.zeros(3)
            step[axis] = sign
            for past, blend in ((1.0, 0.0), (1.5, 0.0), (40.0, 0.0), (0.5, 0.5), (0.25, 0.75)):
                world = (org + step * (ext + past * sp)).astype(F)
                irr, tr = DR.irradiance(dg, vol, world, n, (5.0, 2.0, -3.0))
                if blend == 0.0:
                    assert np.all(irr == 0.0) and tr["evaluated"][0] == 0, (axis, sign, past)
                else:
                    assert tr["inside"][0] == 0 and tr["blend"][0] == F(blend)
                    assert np.max(np.abs(irr[0] - inside * blend) / (inside * blend)) <= 2.0 ** -20, (axis, sign, past)
    # two axes outside: the product of the two fades
    world = (org + (ext + 0.5 * sp) * np.array([1.0, -1.0, 0.0])).astype(F)
    irr, tr = DR.irradiance(dg, vol, world, n, (5.0, 2.0, -3.0))
    assert tr["blend"][0] == F(0.25) and np.max(np.abs(irr[0] - inside * 0.25) / (inside * 0.25)) <= 2.0 ** -20


def test_pow_convention(dg):
    """pow(0, e) = 0, pow(1, e) = 1, and the rest within the two software functions' bounds of the real power."""
    x = np.concatenate([[0.0, 1.0, -1.0, np.nan], np.arange(1, 1024) / 1023.0]).astype(F)
    got = DR.pow_soft(dg, x, 2.5)
    assert got[0] == 0 and got[1] == 1 and got[2] == 0 and got[3] == 0
    want = x[4:].astype(np.float64) ** 2.5
    assert np.max(np.abs(got[4:] - want) / want) < 2.0 ** -19


# ---- borders ----------------------------------------------------------------------------------------------------------------
def test_fill_borders_rule():
    """Rows and columns mirror, corners copy the diagonally opposite interior corner; interior texels stay."""
    for interior in (6, 14):
        n = interior + 2
        rng = np.random.default_rng(interior)
        t = rng.integers(1, 1 << 30, (2, 3 * n, 2 * n), dtype=np.int64).astype(np.uint32)
        before = t.copy()
        assert ddgi.fill_borders(t, interior) is t
        for ty in range(3):
            for tx in range(2):
                a, b = t[1, ty * n:(ty + 1) * n, tx * n:(tx + 1) * n], before[1, ty * n:(ty + 1) * n, tx * n:(tx + 1) * n]
                assert np.array_equal(a[1:-1, 1:-1], b[1:-1, 1:-1])
                for x in range(1, n - 1):
                    assert a[0, x] == b[1, n - 1 - x] and a[n - 1, x] == b[n - 2, n - 1 - x]
                    assert a[x, 0] == b[n - 1 - x, 1] and a[x, n - 1] == b[n - 1 - x, n - 2]
                assert a[0, 0] == b[n - 2, n - 2] and a[0, n - 1] == b[n - 2, 1] and a[n - 1, 0] == b[1, n - 2] and a[n - 1, n - 1] == b[1, 1]
    d = np.zeros((1, 16, 32, 2), np.float16)
    d[0, 1:15, 17:31, 1] = 3.0
    ddgi.fill_borders(d, 14)
    assert np.all(d[0, :, 16:, 1] == 3.0) and np.all(d[..., 0] == 0) and np.all(d[0, :, :16, 1] == 0)
    with pytest.raises(ValueError, match="whole number"):
        ddgi.fill_borders(np.zeros((1, 9, 8), np.uint32), 6)


def test_borders_continue_the_octahedron(dg):
    """With filled borders a bilinear fetch at an octahedral coordinate on a tile's edge equals the fetch at the coordinate the
    octahedron identifies it with: (u, +-1) with (-u, +-1) and (+-1, v) with (+-1, -v).  The two fetches weigh the same four
    values with the columns swapped and the weights f and 1 - f.  The texel coordinate (up to 48 here, ulp 2^-18) is rounded about
    four times on its way (the product with interior / 2, two sums, the division by and product with the size), so the two weights
    miss summing to 1 by at most 2^-16; times the spread of the values, at most 1 for irradiance texels and 2 for the distance
    tile's: 2^-16 and 2^-15 absolute."""
    m, _ = DS.images()[:2]
    vol = DS.volume("3x2x4", m)
    rng = np.random.default_rng(5)
    worst = 0.0
    for c in ((0, 0, 0), (2, 1, 3), (1, 0, 2)):
        for u in np.concatenate([rng.uniform(-1, 1, 24), [0.0, 1.0, -1.0, 0.5]]).astype(F):
            for edge in (F(-1.0), F(1.0)):
                for a, b in (((u, edge), (-u, edge)), ((edge, u), (edge, -u))):
                    worst = max(worst, float(np.max(np.abs(DR.fetch_irradiance(dg, vol, c, a) - DR.fetch_irradiance(dg, vol, c, b)))))
                    assert np.max(np.abs(DR.fetch_distance(dg, vol, c, a) - DR.fetch_distance(dg, vol, c, b))) <= 2.0 ** -15
    assert worst <= 2.0 ** -16
    # and without the borders it does not: the check can fail
    bare = DS.volume("3x2x4", m)
    bare.irradiance[:, ::8, :] = 0
    assert np.max(np.abs(DR.fetch_irradiance(dg, bare, (1, 0, 2), (F(0.3), F(-1.0))) - DR.fetch_irradiance(dg, bare, (1, 0, 2), (F(-0.3), F(-1.0))))) > 1e-3


def test_octahedral_encode(dg):
    """oct() inverts the octahedral decode on both hemispheres and stays in [-1, 1]^2."""
    rng = np.random.default_rng(9)
    d = rng.normal(size=(2000, 3)).astype(F)
    uv = DR.oct_encode(dg, d).astype(np.float64)
    assert np.all(np.abs(uv) <= 1.0)
    z = 1 - np.abs(uv).sum(-1)
    x, y = uv[:, 0].copy(), uv[:, 1].copy()
    t = np.clip(-z, 0, 1)
    x += np.where(x >= 0, -t, t)
    y += np.where(y >= 0, -t, t)
    back = np.stack([x, y, z], -1)
    back /= np.linalg.norm(back, axis=1)[:, None]
    assert np.max(np.abs(back - d / np.linalg.norm(d.astype(np.float64), axis=1)[:, None])) < 1e-6


# ---- float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DS.VOLUMES))
def test_reference_against_float64(dg, scenes, name):
    """The C reference against the numpy float64 restatement on the test scenes.  A pixel where a branch decides differently
    in the two precisions (the inside test, the base clamp, a skip, a Chebyshev compare, the 0.2 crush) is left out; at most
    1 % of the lit pixels may be."""
    s = scenes[name]
    lit = s["lit"] & np.isfinite(s["world"]).all(-1)
    irr, tr = s["irr"][lit], s["traces"][lit]
    i64, dec = DR.irradiance64(s["vol"], s["world"][lit], s["normal"][lit], s["eye"])
    ev = tr["evaluated"] == 1
    same = (dec["inside"] == (tr["inside"] == 1)) & (dec["evaluated"] == ev)
    same &= ~ev | ((dec["base"] == tr["base"]).all(-1) & (dec["skip"] == tr["skipMask"]) & (dec["cheb"] == tr["chebMask"]) & (dec["crush"] == tr["crushMask"]))
    left_out = int(np.count_nonzero(~same))
    positive = same & (i64.max(-1) > 0)
    rel = np.abs(irr[positive].astype(np.float64) - i64[positive]) / i64[positive]
    print(f"{name}: {int(lit.sum())} lit pixels, {left_out} left out, {int(positive.sum())} compared, max relative error {rel.max():.3e} (bound {FLOAT64_BOUND:.1e})")
    assert left_out <= LEFT_OUT_CAP * int(s["lit"].sum())
    assert positive.sum() > 1000
    assert np.all(irr[same & ~(i64.max(-1) > 0)] == 0)
    assert rel.max() <= FLOAT64_BOUND


# ---- branches ---------------------------------------------------------------------------------------------------------------
def test_scenes_reach_every_branch(scenes):
    """Summed over the two scenes each branch of the query occurs on at least 16 pixels."""
    total = {}
    for s in scenes.values():
        for name, n in s["counters"].items():
            total[name] = total.get(name, 0) + n
    print(total)
    for name in DR.COUNTERS:
        assert total[name] >= 16, name
    for s in scenes.values():
        for name in ("blend_one", "blend_partial", "skipped_some", "relocated", "cheb_taken", "cheb_not", "crush_taken", "crush_not", "fold_taken", "fold_not", "clamped"):
            assert s["counters"][name] >= 16, name
    assert scenes["3x2x4"]["counters"]["skipped_all"] >= 16
    # every neighbour of the one-cell volume is clamped somewhere; all eight skipped gives exactly 0
    s = scenes["3x2x4"]
    none = s["lit"] & (s["traces"]["evaluated"] == 1) & (s["traces"]["skipMask"] == 0xFF)
    assert np.all(s["irr"][none] == 0)


def test_ambient_is_added_and_ssao_scales_it(dg):
    """PS_Main: the flag adds albedo / pi * irr to the directional light's words; m_SSAOEnabled scales the term by ssao / 255;
    without the flag the words are lighting_ref.c's.  Debug view 10 stores irr itself; unwritten texels keep the sentinel."""
    m, eye, g, depth, motion, ssao, shadow = DS.images()
    vol = DS.volume("3x2x4", m)
    k = LR.consts(m, eye, (0.3, -2.5, 1.0), 2.0, (DS.W, DS.H))
    lr = dg                                                      # ddgi_ref.c includes lighting_ref.c: the same library has lr_lighting
    lr.lr_lighting.argtypes = [DR.C.c_void_p, DR.C.c_int] + [DR.C.c_void_p] * 7
    lr.lr_lighting.restype = None
    init = np.full((DS.H, DS.W), 0xDEADBEEF, np.uint32)
    plain = LR.lighting(lr, k, g, depth, ssao=ssao, shadow=shadow, out_init=init)
    assert np.array_equal(DR.lighting(dg, k, vol, g, depth, ssao=ssao, shadow=shadow, out_init=init), plain)
    k["m_bRTDDGIEnabled"] = 1
    on, ex = DR.lighting(dg, k, vol, g, depth, ssao=ssao, shadow=shadow, out_init=init, want=("rgb", "irr"))
    lit = depth > 0
    assert np.all(on[~lit] == 0xDEADBEEF) and np.count_nonzero(on[lit] != plain[lit]) > 500
    k["m_SSAOEnabled"] = 1
    ao = DR.lighting(dg, k, vol, g, depth, ssao=ssao, shadow=shadow, out_init=init)
    assert np.count_nonzero(ao[lit] != on[lit]) > 500
    assert np.array_equal(DR.lighting(dg, k, vol, g, depth, ssao=None, shadow=shadow, out_init=init), on)      # unbound reads 255
    _, _, albedo = DR.inputs(dg, k, g, depth)
    _, base = LR.lighting(lr, k, g, depth, ssao=ssao, shadow=shadow, want_rgb=True)
    want = base[lit] + (albedo[lit] * F(1.0 / math.pi)) * ex["irr"][lit]
    assert np.array_equal(want, ex["rgb"][lit], equal_nan=True)
    k10 = LR.consts(m, eye, (0.3, -2.5, 1.0), 2.0, (DS.W, DS.H), debug_mode=10)
    dbg, ex10 = DR.lighting(dg, k10, vol, g, depth, motion=motion, out_init=init, want=("rgb", "irr"))
    assert np.array_equal(ex10["rgb"][lit], ex10["irr"][lit]) and np.array_equal(ex10["irr"][lit], ex["irr"][lit]) and np.all(dbg[~lit] == 0xDEADBEEF)


# ---- ddgi.py ----------------------------------------------------------------------------------------------------------------
def test_encode_irradiance_inverts_the_decode(dg):
    rgb = np.array([[0.05, 0.5, 2.0], [1.0, 1.0, 1.0], [0.0, 6.9, 3.0]])
    words = ddgi.encode_irradiance(rgb)
    assert np.all(words >> 30 == 3)
    texels = np.stack([(words >> s) & 1023 for s in (0, 10, 20)], -1).astype(F) / F(1023.0)
    e = DR.pow_soft(dg, texels, 2.5).reshape(-1, 3).astype(np.float64)
    back = e * e * 2 * math.pi * 1.0989
    # one 10-bit step of a texel t moves the decoded value by 5 / (1023 t) of itself
    tol = np.maximum(5.0 / (1023.0 * np.maximum(texels, 1e-3)) * 0.5 + 1e-5, 0) * np.maximum(rgb, 1e-9)
    assert np.all(np.abs(back - rgb) <= tol + (rgb == 0) * 1e-12)
    assert back[2, 0] == 0.0


def test_uniform_volume_gives_its_irradiance(dg):
    vol = ddgi.Volume.uniform((0, 0, 0), (1, 1, 1), (2, 3, 2), irradiance=(0.4, 1.0, 2.5))
    assert vol.desc()["flags"][0] == 0 and vol.data.shape == (3, 2, 2, 4) and vol.irradiance.shape == (3, 16, 16) and vol.distance.shape == (3, 32, 32, 2)
    irr, _ = DR.irradiance(dg, vol, [[0.1, 0.2, -0.3]], [[0, 1, 0]], (3, 3, 3))
    assert np.allclose(irr[0], (0.4, 1.0, 2.5), rtol=6e-3)


def test_volume_for_scene_follows_the_renderer():
    """GIRenderer.cpp:50-108: spacing min(1, 0.22 * extents) but at least extents / 64; counts ceil(2 * extents / spacing)."""
    v = ddgi.Volume.for_scene((0, 1, 0), (1.0, 1.0, 1.0), 1.7)
    assert v.counts == (10, 10, 10) and v.view_bias == 0.1 and v.normal_bias == 0.02 and np.allclose(v.spacing, 0.22)
    v = ddgi.Volume.for_scene((5, 2, -1), (100.0, 10.0, 40.0), 110.0)
    assert v.spacing == (float(F(100.0) / F(64.0)), 1.0, 1.0) and v.counts == (128, 20, 80) and v.view_bias == 0.3 and v.normal_bias == 0.1
    assert v.origin == (5.0, 2.0, -1.0) and v.relocation and v.classification and v.gamma == 5.0
    d = v.desc()
    assert d.nbytes == 64 and d["flags"][0] == 3 and d["numIrradianceInteriorTexels"][0] == 6 and d["numDistanceInteriorTexels"][0] == 14
    for bad in (dict(counts=(0, 1, 1)), dict(counts=(1, 1025, 1)), dict(spacing=(1, 0, 1)), dict(spacing=(1, float("inf"), 1)), dict(spacing=(1, float("nan"), 1))):
        kw = dict(origin=(0, 0, 0), spacing=(1, 1, 1), counts=(2, 2, 2), normal_bias=0.1, view_bias=0.3)
        kw.update(bad)
        with pytest.raises(ValueError):
            ddgi.Volume(**kw)


def test_probe_positions_and_states_order():
    m = DS.images()[0]
    vol = DS.volume("3x2x4", m)
    pos, st = vol.probe_positions_and_states()
    cx, cy, cz = vol.counts
    assert pos.shape == (24, 3) and pos.dtype == F and st.shape == (24,)
    sp, org = np.asarray(vol.spacing, F), np.asarray(vol.origin, F)
    ext = (sp * np.asarray([cx - 1, cy - 1, cz - 1], F)) * F(0.5)
    for x, y, z in ((0, 0, 0), (2, 1, 3), (1, 0, 2)):
        i = y * cx * cz + x + cx * z
        want = (sp * np.asarray([x, y, z], F) - ext) + org + vol.data[y, z, x, :3].astype(F) * sp
        assert np.array_equal(pos[i], want) and st[i] == F(vol.data[y, z, x, 3])


# ---- layout and declarations ------------------------------------------------------------------------------------------------
def test_volume_desc_layout(tmp_path):
    """A g++-compiled probe prints sizeof / offsetof of interop::DDGIVolumeDesc (csrc/ShaderInterop.h): 64 bytes, every field
    where the numpy dtype and tests/ddgi_ref.c have it."""
    fields = list(I.DDGIVolumeDesc.names)
    out = layout_probe(tmp_path, [("sizeof", "sizeof(interop::DDGIVolumeDesc)")] + [(f, f"offsetof(interop::DDGIVolumeDesc, {f})") for f in fields])
    assert int(out["sizeof"]) == 64 == I.DDGIVolumeDesc.itemsize
    want = dict(origin=0, probeNormalBias=12, probeSpacing=16, probeViewBias=28, probeCounts=32, probeIrradianceEncodingGamma=44,
                numIrradianceInteriorTexels=48, numDistanceInteriorTexels=52, flags=56, pad=60)
    for f in fields:
        assert int(out[f]) == I.DDGIVolumeDesc.fields[f][1] == want[f], f


def test_formats_and_array_entry_points_are_declared():
    """The two formats and the array-texture entry points exist in the header, the binding and the library; the ABI version
    stays 1."""
    from toyrenderer_amd import rhi
    text = open(os.path.join(ROOT, "include", "trhip.h")).read()
    assert re.search(r"TRHIP_FORMAT_R10G10B10A2_UNORM\s*=\s*12\b", text) and re.search(r"TRHIP_FORMAT_RGBA16_FLOAT\s*=\s*13\b", text)
    assert re.search(r"#define TRHIP_ABI_VERSION 1\b", text)
    assert rhi.FORMAT_R10G10B10A2_UNORM == 12 and rhi.FORMAT_RGBA16_FLOAT == 13
    lib = rhi.load()
    for name in ("trhip_texture_create_array", "trhip_texture_array_size", "trhip_texture_slice_pitch", "trhip_texture_upload_slice", "trhip_texture_download_slice"):
        assert name in rhi.ABI_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, text), name
    # trhip_texture_desc did not grow
    assert rhi.C.sizeof(rhi.TextureDesc) == 32
