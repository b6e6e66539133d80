"""Texture streaming on the GPU, on the scenes that tell a wrong mark apart (tests/texture_streaming_rule_scenes.py; the CPU proof that
they do: tests/test_texture_streaming_rule_scenes.py): six scenes of a wrapped and a clamped quad over six texture shapes with regions
of 8 x 4, 4 x 8, 16 x 4, 4 x 16 and 4 x 4 texels, two of them 24 x 40 and one 48 x 16 texels (level sizes that are no powers of two: the
`i % dim` wrap of pointOf and axisOf under #streamed), under min-mip maps with bytes below, at and above mips - 1.  Every word of the
visibility texels, GBufferA, the motion target and every decoded feedback byte against tests/texture_streaming_ref.c, and three
invariants that need no reference.  The kernel's per-lane drop and wave merge (Marker, emitMark in csrc/material_textures.hip.h) have
no counterpart in the reference, which marks mark by mark: these scenes are their check.  Negative controls:
profiles/gbuffer/streaming_mutations.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bc_ref  # noqa: E402
import texture_streaming_ref as TS  # noqa: E402
import texture_streaming_rule_scenes as R  # noqa: E402
import texture_streaming_scenes as X  # noqa: E402
from suite_support import dev, ref_library, same, vr  # noqa: E402, F401

pytestmark = pytest.mark.gpu
ts = ref_library(TS)
COMBINATIONS = [(name, shape) for name in R.SCENES for shape in R.SHAPES]


@pytest.fixture(scope="module")
def bc(tmp_path_factory):
    return bc_ref.load(tmp_path_factory.mktemp("bc_ref"))


@pytest.mark.parametrize("name, shape", COMBINATIONS, ids=[f"{n}-{R.shape_id(s)}" for n, s in COMBINATIONS])
def test_rule_scene_matches_the_reference_and_keeps_the_invariants(dev, vr, ts, bc, name, shape):
    """Four raster and resolve pairs of one scene over one texture shape, each equal to the reference word for word: under the random
    min-mip map, under the zero map, under the random map with m_bWriteSamplerFeedback = 0, and through the #textured kernel on the
    table without maps.  Between them: the feedback does not depend on the min-mip map; with the flag off no feedback word moves and
    GBufferA does not change; #streamed under the zero map writes the words of #textured."""
    scene, mats, table, zero, where, textures = R.case(name, shape)
    what = f"{name}, {R.shape_id(shape)}"
    fb_at = where[0][1]
    vis, g, fb = X.both(dev, vr, ts, bc, scene, mats, table, what)
    _, g0, fb0 = X.both(dev, vr, ts, bc, scene, mats, zero, what + ", min-mip 0")
    same(fb[fb_at], fb0[fb_at], what + ": feedback does not depend on the min-mip map")
    assert np.any(fb[fb_at] != TS.NEVER), what + ": something was sampled"
    _, g_off, fb_off = X.both(dev, vr, ts, bc, scene, mats, table, what + ", flag off", feedback=False)
    assert np.all(fb_off[fb_at] == TS.NEVER), what + ": m_bWriteSamplerFeedback = 0 moves no feedback word"
    same(g_off, g, what + ": GBufferA does not depend on the feedback flag")
    _, g_plain, none = X.both(dev, vr, ts, bc, scene, R.plain_materials(), list(textures), what + ", no maps", names=X.TEXTURED)
    assert none == {}
    same(g0, g_plain, what + ": #streamed under the zero map against #textured")
    assert np.any(g[vis != 0] != g0[vis != 0]), what + ": the min-mip map clamps some pixel"
