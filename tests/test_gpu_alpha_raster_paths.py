"""The alpha-tested compute rasteriser (csrc/k_raster.hip, "basepass_MS_Main_depth ALPHA_MASK_MODE=1" and
"basepass_MS_Main_visibility ALPHA_MASK_MODE=1") on both sides of each raster path switch: kSmallBox, the collect rounds of a tile
(kTileList), kBinCapacity, kQueueCapacity, the "tiles" launch's grid stride and the far-depth early-out under discards; and rules
5 and 6 of the convention (a NaN alpha is kept; a broken chain draws nothing) through both launches, with and without a table.

The scenes are the alpha variants of tests/raster_path_scenes.py; that every kept triangle owns a texel, that the samples lie on
the path a case names and that the discard SHOWS there (the image differs from the no-discard image on texels of the triangles the
case is about) is proven without a GPU in tests/test_raster_path_scenes.py.  Here every depth word of both instantiations and
every texel is compared with tests/alpha_test_ref.c after a direct dispatch into cleared textures: no exclusions, no tolerance.
The kernel exposes no counter: that a case takes the path it names is shown by the mutated builds of
profiles/raster_paths/alpha_mutations.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_path_scenes as S  # noqa: E402
from suite_support import at, dev, raster_dispatch, same, vr  # noqa: E402, F401

pytestmark = pytest.mark.gpu
K = S.K
LOW = np.uint64(0xFFFFFFFF)


def _compare(dev, s, rdepth, rvis, what, alpha=True, table=True):
    """Both instantiations of one dispatch against (rdepth, rvis)."""
    assert np.array_equal((rvis >> np.uint64(32)).astype(np.uint32), rdepth.view(np.uint32)), f"{what}: the reference's images disagree"
    depth, _ = raster_dispatch(dev, s, False, alpha=alpha, table=table, slot=S.SLOT)
    same(depth.view(np.uint32), rdepth.view(np.uint32), f"{what}: depth instantiation")
    depth, vis = raster_dispatch(dev, s, True, alpha=alpha, table=table, slot=S.SLOT)
    same(depth.view(np.uint32), rdepth.view(np.uint32), f"{what}: visibility instantiation's depth")
    same(vis, rvis, f"{what}: texels")


def _check(dev, at, s, what, threads=16):
    """Both alpha instantiations against at_raster; returns the reference (depth, texels, counts)."""
    rdepth, rvis, counts = S.alpha_reference(at, s, threads)
    _compare(dev, s, rdepth, rvis, what)
    return rdepth, rvis, counts.astype(np.int64)


def _owner_case(dev, at, name):
    make, path, _, threads = S.ALPHA_OWNER_SCENES[name]
    s = make(dev.compute_units)
    assert s.queue_length == (0 if path == "main" else s.n_triangles)
    rdepth, rvis, counts = _check(dev, at, s, name, threads)
    assert np.array_equal(np.unique(rvis[rvis != 0] & LOW), np.sort(s.payloads)), "every listed triangle owns a texel"
    assert counts[0 if path == "main" else 2] > 0 and counts[1 if path == "main" else 3] > 0 and counts[2 if path == "main" else 0] == 0
    return s, rdepth, rvis


@pytest.mark.parametrize("kind", ["box1024", "box1025", "box33x32", "edge_clamped"])
def test_small_box_switch(dev, at, kind):
    """(a) Checker-textured boxes of exactly kSmallBox pixels (drawn in place by "main", material from the meshlet's instance)
    beside kSmallBox + 1 and 33x32 (queued: AlphaTriangle and the material resolved again in "tiles"), and 33x32 boxes that the
    clamp to the screen brings back to kSmallBox and below."""
    _owner_case(dev, at, f"a-{kind}")


@pytest.mark.parametrize("count", [K["kTileList"] - K["kBlock"], K["kTileList"], K["kTileList"] + 1, 2 * K["kTileList"] + 1])
def test_tile_rounds(dev, at, count):
    """(b) One tile with exactly `count` textured candidates: from the second round on s_list[k] is not k.  Every triangle loses
    its apex texel to its left neighbour through the discard, so a triangle drawn with another's AlphaTriangle changes the image."""
    s, _, _ = _owner_case(dev, at, f"b-{count}")
    assert s.tile_candidates[1, 1] == count


def test_tile_round_ends_between_chunks(dev, at):
    """(b) 3000 textured candidates of which every third matches tile (0, 0) and the others tile (2, 0)."""
    s, _, _ = _owner_case(dev, at, "b-sparse")
    assert s.tile_candidates[0, 0] == 1000 and s.tile_candidates[0, 2] == 2000 and s.bin_counts[0, 0] == 3000


@pytest.mark.parametrize("extra", [False, True], ids=["full", "over"])
def test_bin_capacity(dev, at, extra):
    """(c) Bin (0, 0) with exactly kBinCapacity textured slivers and with one more (its tiles scan the whole queue, and
    queueAlpha with it).  15 triangles per meshlet: "main" takes a second trip of its stride loop."""
    s, _, _ = _owner_case(dev, at, "c-over" if extra else "c-full")
    assert s.bin_counts[0, 0] == K["kBinCapacity"] + int(extra)
    assert len(s.lst) > K["mainGridPerCU"] * dev.compute_units * (K["kBlock"] // 64)


def test_full_queue_textured_slivers(dev, at):
    """(d) 2^20 + 65 536 textured slivers with boxes above kSmallBox at 4096x1024: the ones that find the queue full are drawn in
    place by "main" through s_atri.  Each sliver's second sample is discarded; without the discard it would hide its right
    neighbour's apex.  The reference: 16 disjoint slices of the list from 16 threads, max-merged."""
    s, _, _ = _owner_case(dev, at, "d-slivers")
    assert s.queue_length >= K["kQueueCapacity"] + 4096


def test_full_queue_constant_alpha(dev, oracle, vr):
    """(d) queue_scene()'s geometry, its 17 instances cycling through constant alpha above the cutoff, below it and a broken
    chain: the image is that of the kept instances alone, from vr_raster / orc_raster_depth over their list positions (that
    at_raster agrees is asserted on the CPU)."""
    s = S.queue_constant_alpha()
    assert s.queue_length >= K["kQueueCapacity"] + 4096
    rdepth, rvis = S.reference(oracle, vr, s, threads=16, positions=s.kept_positions)
    _compare(dev, s, rdepth, rvis, "full queue, constant alpha")
    kept = (np.arange(s.n_triangles) // (s.n_triangles // len(s.sc["instances"]))) % 3 == S.M_ABOVE
    assert np.array_equal(np.unique(rvis[rvis != 0] & LOW), np.sort(s.payloads[kept])), "every triangle of a kept instance owns a texel"


def test_tile_grid_stride(dev, at):
    """(e) More tiles than the "tiles" launch has workgroups, textured: the last tile (one pixel) is drawn by a workgroup's
    second trip and is not empty."""
    s, rdepth, _ = _owner_case(dev, at, "e-stride")
    tx, ty = s.tiles
    assert tx * ty > s.grid == K["tileGridPerCU"] * dev.compute_units and np.all(s.tile_candidates.reshape(-1)[s.grid:] >= 1)
    assert rdepth[-1, -1] > 0 and np.count_nonzero(rdepth[-1]) > 200


@pytest.mark.parametrize("cover", S.EARLY_OUT_COVERS)
def test_early_out_under_discards(dev, oracle, vr, at, cover):
    """(f) 8 tiles of 23 kept slivers, each 2^-10 behind the one before, and 8 cover quads drawn four times and queued first, 0 .. 14
    float32 steps above the first sliver (the factor is about 10 steps).  checker: a tile with holes has far depth 0: nothing may
    be skipped, every sliver shows through the holes, the farthest too.  opaque (every alpha byte 255): every word also equals
    the plain kernels' output.  below (constant alpha below the cutoff): every word also equals the image of the slivers alone."""
    s = S.early_out_alpha(cover)
    assert s.queue_length == s.n_triangles
    rdepth, rvis, _ = _check(dev, at, s, f"early-out, {cover} covers")
    if cover == "opaque":
        for texels in (False, True):
            depth, vis = raster_dispatch(dev, s, texels, slot=S.SLOT)
            same(depth.view(np.uint32), rdepth.view(np.uint32), "opaque covers: the plain kernel's depth")
            if texels:
                same(vis, rvis, "opaque covers: the plain kernel's texels")
    if cover == "below":
        sdepth, svis = S.reference(oracle, vr, s, positions=s.positions[1])
        same(rvis, svis, "covers below the cutoff: the slivers alone"); same(rdepth.view(np.uint32), sdepth.view(np.uint32), "covers below the cutoff: depth")


@pytest.mark.parametrize("table", [True, False], ids=["table", "no table"])
@pytest.mark.parametrize("path", ["main", "tiles"])
def test_rules_5_and_6(dev, at, path, table):
    """(g), (h) One instance per case of S.RULE_CASES through "main" (1024-pixel boxes) and "tiles" (33x32): an index past the
    buffer, a descriptor past the table, an empty entry, an entry of another format, cutoff +inf and the next float above alpha
    draw nothing; NaN alpha, NaN cutoff and alpha == cutoff are kept, textured and texture-free.  No table bound: every
    material with the albedo flag draws nothing."""
    s = S.rules_alpha(path, table)
    assert s.queue_length == (0 if path == "main" else s.n_triangles)
    rdepth, rvis, _ = S.alpha_reference(at, s, 1)
    shown = np.unique(S.triangle_of(s, rvis[rvis != 0] & LOW) // 5)
    assert np.array_equal(shown, np.flatnonzero(s.kept)) and len(shown) == (7 if table else 3), (shown, s.kept)
    _compare(dev, s, rdepth, rvis, f"rules, {path}, table {table}", table=table)
