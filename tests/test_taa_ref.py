"""Properties of tests/taa_ref.c, the definition of "taa_CS_TemporalResolve" (csrc/k_taa.hip), and of the host side of temporal
anti-aliasing (toyrenderer_amd/taa.py).  CPU only: what the GPU must equal word for word is tested here for what it means."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import taa_ref as TR  # noqa: E402
from ref_build import layout_probe  # noqa: E402
from suite_support import ref_library, same  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from toyrenderer_amd import taa as T  # noqa: E402

F = np.float32
ta = ref_library(TR)


def _f16(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(F)


def _rgb(words):
    return _f16(TR.history_of(words, 0))[..., :3]


# ---- 1, 2. the fixed point and the reset ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", [TR.ONE_WORD, 0x3A5 | 0x2C1 << 11 | 0x1F3 << 22, 0])
def test_a_constant_image_is_a_fixed_point(ta, word):
    """Ten frames of one colour with no motion and no jitter: the output is the input on every frame, and the count climbs
    1, 2, ... to the cap (4 here) and stays."""
    W, H = 9, 5
    colour, depth, motion = np.full((H, W), word, np.uint32), np.full((H, W), 0.5, F), TR.motion_of(0.0, 0.0, W, H)
    history = np.full((H, W, 4), 0x7E00, np.uint16)                                  # what a reset must not read
    for f in range(10):
        k = TR.consts(W, H, max_sample_count=4.0, reset=f == 0)
        history, out, path = TR.resolve(ta, k, colour, depth, motion, history)
        same(out, colour, f"frame {f}: output")
        same(history[..., :3], TR.history_of(colour, 0)[..., :3], f"frame {f}: history colour")
        assert np.all(_f16(history[..., 3]) == min(f + 1, 4)), (f, _f16(history[0, 0, 3]))
        assert np.all((path & TR.VALID) == (0 if f == 0 else 1)) and not np.any(path & (TR.CLAMPED | TR.DILATED))


def test_a_reset_gives_the_current_colour(ta):
    """m_bResetHistory: every texel's output is its current word, whatever the history and the motion hold, the history is that
    colour with count 1, and the history is not fetched (no weight bit)."""
    W, H = 13, 7
    colour, depth, motion, history = TR.seeded_inputs(W, H, 11)
    new, out, path = TR.resolve(ta, TR.consts(W, H, reset=True), colour, depth, motion, history)
    same(out, TR.repack(ta, colour), "output")                                       # a NaN channel comes back as the one NaN code
    finite = TR.finite_colour(W, H, 12)
    new, out, path = TR.resolve(ta, TR.consts(W, H, reset=True), finite, depth, motion, history)
    same(new, TR.history_of(finite, 1), "history")
    assert not np.any(path & (TR.VALID | TR.CLAMPED | TR.WEIGHTS))


# ---- 3. the clamp ---------------------------------------------------------------------------------------------------------------
def test_history_is_clamped_into_the_neighbourhood(ta):
    W, H = 16, 8
    k, colour, depth, motion, history = TR.constructed_cases(W, H)["clamp"]
    new, out, path = TR.resolve(ta, k, colour, depth, motion, history)
    assert np.all(path & TR.VALID)
    moved = np.zeros((H, W), bool)
    moved[::2, ::2] = True
    # 40 in every channel is brighter than any neighbour (the colours are below 32): the clamp acts exactly there
    assert np.all((path[moved] & TR.CLAMPED) != 0) and not np.any(path[~moved] & TR.CLAMPED)
    rgb = _rgb(colour).astype(np.float64)
    Y = 0.25 * rgb[..., 0] + 0.5 * rgb[..., 1] + 0.25 * rgb[..., 2]
    pad = np.pad(Y, 1, mode="edge")
    box_hi = np.max([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    got = _f16(new[..., :3]).astype(np.float64)
    got_Y = 0.25 * got[..., 0] + 0.5 * got[..., 1] + 0.25 * got[..., 2]
    assert np.all(got_Y[moved] <= box_hi[moved] * (1 + 2.0 ** -9) + 2.0 ** -14), "the blend of the centre and a clamped history lies inside the box"
    # where the history already was the centre's colour, nothing changes
    same(out[~moved], colour[~moved], "unclamped texels")


# ---- 4. reprojection ------------------------------------------------------------------------------------------------------------
def test_whole_pixel_motion_fetches_one_texel(ta):
    """Sizes that are powers of two, where hp / W * W is exact: motion (-2, 1) fetches texel (px - 2, py + 1) alone; motion equal
    to the jitter delta fetches the pixel itself."""
    W, H = 16, 8
    cases = TR.constructed_cases(W, H)
    k, colour, depth, motion, history = cases["shift"]
    new, out, path = TR.resolve(ta, k, colour, depth, motion, history)
    inside = np.zeros((H, W), bool)
    inside[:H - 1, 2:] = True
    assert np.all((path[inside] & TR.WEIGHTS) == TR.W00) and np.all(path[inside] & TR.VALID) and not np.any(path[~inside] & TR.VALID)
    # the same frame with the history image shifted the other way and no motion fetches the same texels: equal words
    shifted = np.zeros_like(history)
    shifted[:H - 1, 2:] = history[1:, :W - 2]
    new0, out0, path0 = TR.resolve(ta, k, colour, depth, TR.motion_of(0.0, 0.0, W, H), shifted)
    same(out[inside], out0[inside], "shifted history")
    same(new[inside], new0[inside], "shifted history: new history")
    k, colour, depth, motion, history = cases["jitter delta"]
    new, out, path = TR.resolve(ta, k, colour, depth, motion, history)
    assert np.all((path & TR.WEIGHTS) == TR.W00) and np.all(path & TR.VALID)
    new0, out0, _ = TR.resolve(ta, TR.consts(W, H), colour, depth, TR.motion_of(0.0, 0.0, W, H), history)
    same(out, out0, "jitter delta cancelled"); same(new, new0, "jitter delta cancelled: history")
    same(out, colour, "a history equal to the image")


# ---- 5. leaving the screen ------------------------------------------------------------------------------------------------------
def test_motion_outside_the_image_resets_the_pixel(ta):
    W, H = 16, 8
    k, colour, depth, motion, history = TR.constructed_cases(W, H)["leaving"]
    new, out, path = TR.resolve(ta, k, colour, depth, motion, history)
    valid = (path & TR.VALID) != 0
    assert np.all(valid[0, 1:]), "hp.x = 0 is inside"
    assert not np.any(valid[1, 1:]), "hp.x = W is outside"
    assert not np.any(valid[2, 1:]), "hp.x = -0.5 is outside"
    assert not np.any(valid[3, 1:]), "hp.y >= H is outside"
    assert not np.any(valid[4:, 0]), "hp.y < 0 is outside"
    assert np.all(valid[4:, 1:])
    same(out[~valid], colour[~valid], "reset texels")
    assert np.all(_f16(new[..., 3])[~valid] == 1) and np.all(_f16(new[..., 3])[valid] == 4)
    assert not np.any(path[~valid] & TR.WEIGHTS), "no fetch outside"


# ---- 6. dilation ----------------------------------------------------------------------------------------------------------------
def test_the_nearest_surface_lends_its_motion(ta):
    W, H = 16, 8
    k, colour, depth, motion, history = TR.constructed_cases(W, H)["dilation"]
    new, out, path = TR.resolve(ta, k, colour, depth, motion, history)
    cy, cx = H // 2, W // 2
    ring = np.zeros((H, W), bool)
    ring[cy - 1:cy + 2, cx - 1:cx + 2] = True
    ring[cy, cx] = False
    assert np.all(path[ring] & TR.DILATED) and not np.any(path[~ring] & TR.DILATED), "the eight neighbours move, the foreground and every tie keep the centre"
    fractional = ring.copy()
    fractional[cy, cx] = True
    assert np.all((path[fractional] & TR.WEIGHTS) == TR.WEIGHTS) and np.all((path[~fractional] & TR.WEIGHTS) == TR.W00)
    # a depth of NaN is never nearer, and a NaN centre keeps itself
    depth2 = depth.copy()
    depth2[cy, cx] = np.nan
    _, _, path2 = TR.resolve(ta, k, colour, depth2, motion, history)
    assert not np.any(path2 & TR.DILATED)


# ---- 7. values that are not finite ----------------------------------------------------------------------------------------------
def test_values_that_are_not_finite(ta):
    W, H = 16, 8
    k, colour, depth, motion, history = TR.constructed_cases(W, H)["not finite"]
    new, out, path = TR.resolve(ta, k, colour, depth, motion, history)
    valid = (path & TR.VALID) != 0
    want = np.ones((H, W), bool)
    for i in range(4):                                                               # +inf, -inf and two NaN, one per channel
        y, x = i % H, (2 * i) % W
        assert not valid[y, x], f"a history channel {i} that is not finite resets the pixel"
        # the sampler's lerps are always evaluated: a texel that is not finite also spoils the fetches that reach it with weight 0
        want[max(y - 1, 0):y + 1, max(x - 1, 0):x + 1] = False
    want[H - 1, W - 1] = want[H - 1, 0] = False                                      # NaN and infinite motion
    same(valid, want, "valid history")
    same(out[~valid], colour[~valid], "reset texels")
    # the stated rule for the current colour: with valid history an infinite channel makes the weight 0 and the output NaN, and a
    # NaN colour stays NaN; the stores keep both as their NaN codes, so the next frame resets the pixel
    for y, x in ((H - 2, 1), (H - 2, W - 2)):
        assert valid[y, x] and out[y, x] == TR.NAN_WORD and np.all(new[y, x, :3] == 0x7E00), (y, x, hex(out[y, x]))
    _, _, path2 = TR.resolve(ta, k, colour, depth, TR.motion_of(0.0, 0.0, W, H), new)
    assert not (path2[H - 2, 1] & TR.VALID) and not (path2[H - 2, W - 2] & TR.VALID)
    # a neighbour's box drops the NaN texel: its output is finite
    assert np.all(np.isfinite(_rgb(out[H - 3:H, W - 3:W - 1][[0, 2]])))


# ---- 8. the smallest images -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (2, 2)], ids=str)
def test_every_neighbour_clamps(ta, size):
    """At 1 x 1 the window is the texel nine times, at 2 x 2 every window clamps on two sides: the words equal the interior of a
    larger image whose border repeats (3 x 3 and 4 x 4: sizes at which the sampler's coordinates are exact as well)."""
    W, H = size
    colour, depth, motion, history = TR.seeded_inputs(W, H, 21, finite_history=True)
    colour = TR.finite_colour(W, H, 22)
    motion[:] = 0
    k = TR.consts(W, H)
    new, out, path = TR.resolve(ta, k, colour, depth, motion, history)
    assert np.all(path & TR.VALID) and np.all((path & TR.WEIGHTS) == TR.W00)
    pad = lambda a: np.pad(a, [(1, 1), (1, 1)] + [(0, 0)] * (a.ndim - 2), mode="edge")             # noqa: E731
    newP, outP, _ = TR.resolve(ta, TR.consts(W + 2, H + 2), pad(colour), pad(depth), pad(motion), pad(history.view(np.uint16)))
    same(out, outP[1:-1, 1:-1], "the padded image's interior"); same(new, newP[1:-1, 1:-1], "the padded image's interior: history")


# ---- 9. the constants -----------------------------------------------------------------------------------------------------------
def test_taa_consts_layout(tmp_path):
    fields = I.TAAConsts.fields
    got = layout_probe(tmp_path, [("size", "sizeof(interop::TAAConsts)")] + [(n, f"offsetof(interop::TAAConsts, {n})") for n in fields])
    assert int(got["size"]) == I.TAAConsts.itemsize == 32 and I.TAAConsts.itemsize % 16 == 0
    for n, (_, off) in fields.items():
        assert int(got[n]) == off, n
    k = T.consts(7, 3, T.check_settings({}), (F(0.25), F(-0.125)), (F(-0.5), F(0.375)), True)
    assert k.tobytes() == TR.consts(7, 3, jitter_delta=(-0.75, 0.5), reset=True).tobytes()


# ---- 10. the jitter -------------------------------------------------------------------------------------------------------------
def _radical_inverse(base, index):
    out, d = Fraction(0), Fraction(1, base)
    while index:
        out += (index % base) * d
        index //= base
        d /= base
    return out


def test_halton_jitter():
    seq = TR.jitter_sequence(24)
    assert len({(float(x), float(y)) for x, y in seq[:8]}) == 8
    assert all(-0.5 <= x < 0.5 and -0.5 <= y < 0.5 for x, y in seq)
    assert [tuple(map(float, s)) for s in seq[:8]] == [tuple(map(float, s)) for s in seq[8:16]] == [tuple(map(float, s)) for s in seq[16:]]
    for i, (x, y) in enumerate(seq[:8]):
        assert Fraction(float(x)) == _radical_inverse(2, i + 1) - Fraction(1, 2), i
        assert abs(Fraction(float(y)) - (_radical_inverse(3, i + 1) - Fraction(1, 2))) <= Fraction(1, 1 << 23), i
        assert x.dtype == F and y.dtype == F
    # the projection: the offset moves every point by (jx, jy) pixels, x to the right and y down
    P = np.array([[1.5, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 0, -1], [0, 0, 0.1, 0]], F)
    J = T.jittered_view_to_clip(P, (F(0.25), F(-0.375)), 64, 32)
    p = np.array([0.3, -0.2, -2.0, 1.0], F)
    ndc = lambda m: (p @ m)[:2] / (p @ m)[3]                                                          # noqa: E731
    pixel = lambda n: ((n[0] * 0.5 + 0.5) * 64, (-n[1] * 0.5 + 0.5) * 32)                               # noqa: E731
    a, b = pixel(ndc(P)), pixel(ndc(J))
    assert abs((b[0] - a[0]) - 0.25) < 1e-4 and abs((b[1] - a[1]) + 0.375) < 1e-4
    assert np.array_equal(T.jittered_view_to_clip(P, (F(0.0), F(0.0)), 64, 32), P)


def test_settings_are_checked():
    assert T.check_settings({}) == dict(min_blend=0.1, max_sample_count=64.0, jitter=True)
    for bad, text in ((dict(min_blend=1.5), "min_blend"), (dict(max_sample_count=0), "max_sample_count"), (dict(sharpness=1), "unknown")):
        with pytest.raises(ValueError, match=text):
            T.check_settings(bad)


def test_the_entry_is_registered():
    from toyrenderer_amd import rhi
    assert "taa_CS_TemporalResolve" in set(rhi.shader_names())


def test_seeded_words_reach_every_path(ta):
    """The seeded inputs of the GPU test visit every path bit at a size of a few tiles."""
    W, H = 67, 35
    colour, depth, motion, history = TR.seeded_inputs(W, H, 5, finite_history=True)
    _, _, path = TR.resolve(ta, TR.consts(W, H, jitter_delta=(0.25, -0.125)), colour, depth, motion, history)
    for bit in (TR.VALID, TR.CLAMPED, TR.DILATED, TR.W10, TR.W01, TR.W11):
        assert np.count_nonzero(path & bit) > 20, bit
    assert np.count_nonzero((path & TR.VALID) == 0) > 20


# ---- the scene of the GPU's multi-frame test ------------------------------------------------------------------------------------
def test_the_cornell_path_meets_its_condition(oracle, ta, tmp_path):
    """The reference side of tests/test_gpu_taa.py::test_frames_match_the_reference_chain, without a device: the six frames' path
    bytes meet taa_scenes.check_condition, so that run exercises valid history, texels leaving the screen, the clamp, dilation and
    fractional bilinear weights in every frame after the first."""
    import gbuffer_ref as GR
    import lighting_ref as LR
    import taa_scenes as TS
    import visibility_ref as VR
    from suite_support import lit_cornell
    vr, gr, lr = VR.load(tmp_path), GR.load(tmp_path), LR.load(tmp_path)
    s, inst, _, mats, camera = lit_cornell(oracle)
    sc = dict(s.as_oracle()); sc["instances"] = inst
    geo_v = (s.vertices, s.meshletVertexIds, s.meshletTriangles)
    settings = T.check_settings(TS.SETTINGS)
    W, H = TS.RENDER
    last, paths, history = None, [], np.zeros((H, W, 4), np.uint16)
    for f in range(TS.FRAMES):
        view, (current, previous), prev_world_to_clip, last = T.begin_frame(TS.view_at(camera, f), f, settings, last)
        depth, motion, lit = TS.frame_inputs(oracle, vr, gr, lr, sc, geo_v, view, prev_world_to_clip, mats, TS.lighting_consts(view, TS.camera_at(camera, f)[0]))
        assert np.all(depth > 0), "geometry on every texel: none keeps the cleared motion"
        history, out, path = TR.resolve(ta, T.consts(W, H, settings, current, previous, f == 0), lit, depth, motion, history)
        paths.append(path)
    TS.check_condition(paths)
