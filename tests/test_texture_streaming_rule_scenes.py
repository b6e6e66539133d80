"""The preconditions of tests/test_gpu_texture_streaming_rules.py, on the reference alone (no GPU): the rule scenes
(tests/texture_streaming_rule_scenes.py) leave feedback maps that are not uniform, and they tell every broken rule of the streamed
sampler from the stated one.  The broken rules are the -DTS_REF_MUTATE_* builds of tests/texture_streaming_ref.c: each must change
the decoded feedback or GBufferA of at least two (scene, texture shape) combinations.  The kernel's per-lane drop of repeated marks
(Marker::mark in csrc/material_textures.hip.h) is restated by the -DTS_REF_LANE_DROP build, which must change nothing, and its
broken form (drop on the word index alone) must show too."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bc_ref  # noqa: E402
import material_texture_scenes as S  # noqa: E402
import texture_streaming_ref as TS  # noqa: E402
import texture_streaming_rule_scenes as R  # noqa: E402
import texture_streaming_scenes as X  # noqa: E402
import visibility_ref as VR  # noqa: E402
from visibility_scenes import consts  # noqa: E402

MUTANTS = ["SWAP_REGION_FOOTPRINT", "SWAP_REGION_UNDER", "NO_ORIGIN_SHIFT", "NO_L1W", "NO_L0W_FOOTPRINT", "NO_UNDER", "CLAMPED_LEVELS", "CENTRE_FOOTPRINT",
           "ONE_TEXEL", "UNDER_CLAMP_MODE", "CLAMP_REPLACES", "UNDER_ROUNDS"]
COMBINATIONS = [(name, shape) for name in R.SCENES for shape in R.SHAPES]
_CACHE = {}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(visibility reference, BC decoder, build directory of the streaming reference and its mutants)"""
    d = tmp_path_factory.mktemp("texture_streaming_rule_scenes")
    return VR.load(d), bc_ref.load(d), d


def _run(libs, defines, name, shape, zero=False):
    """(vis, GBufferA, feedback bytes of the texture) of one combination under the build `defines`, computed once."""
    key = (tuple(defines), name, R.SHAPES.index(shape), zero)
    if key not in _CACHE:
        vr, bc, d = libs
        scene, mats, table, zero_table, where, _ = R.case(name, shape)
        vis, g, _, fb = X.reference(vr, TS.load(d, defines), bc, consts(S.view()), scene, mats, zero_table if zero else table)
        _CACHE[key] = (vis, g, fb[where[0][1]])
    return _CACHE[key]


def _kills(libs, defines):
    """The combinations on which the build `defines` differs from the reference: [(scene, shape, feedback bytes, GBufferA words)]."""
    out = []
    for name, shape in COMBINATIONS:
        _, g, fb = _run(libs, defines, name, shape)
        _, g0, fb0 = _run(libs, (), name, shape)
        dfb, dg = int(np.count_nonzero(fb != fb0)), int(np.count_nonzero(g != g0))
        if dfb or dg:
            out.append((name, R.shape_id(shape), dfb, dg))
    return out


def test_scene_conditions(libs):
    """Every scene shows both quads; every min-mip map holds bytes below, at and above mips - 1; every texture shape has a scene whose
    feedback map holds sampled and NEVER regions, neither more than three quarters of it; one map holds three levels or more; the
    feedback does not depend on the min-mip map.
    MEASURED (level: regions; 255 = NEVER), for example: window 24x40 / 8x4 {0: 10, 255: 20}; window 48x16 / 4x16 {0: 5, 255: 7};
    partial floor 64x32 / 16x4 {0: 14, 1: 6, 2: 4, 255: 8}; partial floor 32x32 / 4x4 {0: 32, 1: 1, 2: 3, 255: 28}; partial floor
    64x64 / 8x4 {0: 31, 1: 27, 2: 2, 3: 3, 255: 65}; tilted 64x64 / 8x4 {0: 62, 1: 18, 2: 48}; even taps 64x64 / 8x4 {5: 128}."""
    mixed, levels = collections.Counter(), 0
    for name, shape in COMBINATIONS:
        w, h, _, region = shape
        vis, _, fb = _run(libs, (), name, shape)
        instance = ((vis[vis != 0] & np.uint64(0xFFFFFFFF)) >> np.uint64(7)) & np.uint64(0x7FFFFF)
        assert np.count_nonzero(instance == 0) >= 300 and np.count_nonzero(instance == 1) >= 300, (name, np.bincount(instance.astype(np.int64)))
        mm = R.case(name, shape)[2][1][2]
        top = X.full_chain(w, h) - 1
        assert mm.shape == (h // region[1], w // region[0]) and (mm < top).any() and (mm == top).any() and (mm > top).any(), (name, shape, mm)
        hist = collections.Counter(fb.reshape(-1).tolist())
        print(f"{name:14s} {R.shape_id(shape):36s} {dict(sorted(hist.items()))}")
        never = hist.get(TS.NEVER, 0)
        if 0 < never and 4 * never <= 3 * fb.size and 4 * (fb.size - never) <= 3 * fb.size:
            mixed[R.SHAPES.index(shape)] += 1
        levels = max(levels, len(set(hist) - {TS.NEVER}))
        assert np.array_equal(_run(libs, (), name, shape, zero=True)[2], fb), (name, shape, "feedback under the zero map")
    assert sorted(mixed) == list(range(len(R.SHAPES))), mixed
    assert levels >= 3, levels


@pytest.mark.parametrize("rule", MUTANTS)
def test_the_scenes_tell_a_broken_rule_apart(libs, rule):
    kills = _kills(libs, ("TS_REF_MUTATE_" + rule,))
    print(f"{rule}: {len(kills)} of {len(COMBINATIONS)} combinations (scene, shape, feedback bytes, GBufferA words):", kills)
    assert len(kills) >= 2, (rule, kills)


def test_the_per_lane_drop_changes_no_word_and_its_broken_form_shows(libs):
    """Marking through the kernel's per-lane drop gives the words of marking mark by mark, on every combination.  Dropping on the word
    index alone loses the lower level that follows a higher one: MEASURED 4 feedback bytes of "aligned taps" on each of the 32 x 32
    and 64 x 64 textures, and nothing elsewhere (in the other scenes another pixel marks the same region with the lower level)."""
    assert _kills(libs, ("TS_REF_LANE_DROP",)) == []
    kills = _kills(libs, ("TS_REF_LANE_DROP", "TS_REF_MUTATE_DROP_BY_INDEX"))
    print("DROP_BY_INDEX:", kills)
    assert len(kills) >= 2 and all(k[3] == 0 for k in kills), kills
