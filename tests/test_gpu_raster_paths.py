"""The compute rasteriser (csrc/k_raster.hip, "basepass_MS_Main_depth" and "basepass_MS_Main_visibility") on both sides
of each of its path switches: kSmallBox, the collect rounds of a tile (kTileList), kBinCapacity, kQueueCapacity, the
"tiles" launch's grid stride and the far-depth early-out at its margin and at the ends of the range it is proven for.

The scenes and what the kernel's rules predict for them are in tests/raster_path_scenes.py; that they are where they
claim to be, and that every listed triangle owns a texel, is checked without a GPU in tests/test_raster_path_scenes.py.
Here every depth word of both instantiations is compared with orc_raster_depth and every texel with
tests/visibility_ref.c, after a direct dispatch into cleared textures.  The kernel exposes no counter: that a case
takes the path it names is shown by the mutated builds of profiles/raster_paths/mutations.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_path_scenes as S  # noqa: E402
from suite_support import dev, raster_dispatch, vr  # noqa: E402, F401

pytestmark = pytest.mark.gpu
K = S.K


def _dispatch(dev, s, texels):
    """One direct dispatch of the depth (texels=False) or the visibility instantiation into cleared textures: (depth, vis or None)."""
    return raster_dispatch(dev, s, texels, slot=S.SLOT)


def _check(dev, oracle, vr, s, what, threads=1):
    """Both instantiations against the references; returns the reference (depth, texels)."""
    rdepth, rvis = S.reference(oracle, vr, s, threads=threads)
    assert np.array_equal((rvis >> np.uint64(32)).astype(np.uint32), rdepth.view(np.uint32)), f"{what}: the references disagree"
    depth, _ = _dispatch(dev, s, False)
    bad = int(np.count_nonzero(depth.view(np.uint32) != rdepth.view(np.uint32)))
    assert bad == 0, f"{what}: depth instantiation differs in {bad} words"
    depth, vis = _dispatch(dev, s, True)
    bad = int(np.count_nonzero(depth.view(np.uint32) != rdepth.view(np.uint32)))
    assert bad == 0, f"{what}: visibility instantiation's depth differs in {bad} words"
    bad = int(np.count_nonzero(vis != rvis))
    assert bad == 0, f"{what}: {bad} texels differ"
    return rdepth, rvis


def _all_own_a_texel(s, rvis):
    present = np.unique(rvis[rvis != 0] & np.uint64(0xFFFFFFFF))
    assert len(present) == s.n_triangles and np.array_equal(present, np.sort(s.payloads))


@pytest.mark.parametrize("kind", ["box1024", "box1025", "box33x32", "edge_clamped"])
def test_small_box_switch(dev, oracle, vr, kind):
    """(a) Boxes of exactly kSmallBox pixels (drawn in place by "main") beside kSmallBox + 1 and 33x32 (queued), inside a
    tile, across a tile and a bin corner and on the screen's last column and row; and 33x32 boxes that the clamp to the
    screen brings back to kSmallBox and below."""
    s = S.small_box_scene(kind)
    assert s.queue_length == (s.n_triangles if kind in ("box1025", "box33x32") else 0)
    _all_own_a_texel(s, _check(dev, oracle, vr, s, kind)[1])


@pytest.mark.parametrize("count", [K["kTileList"] - K["kBlock"], K["kTileList"], K["kTileList"] + 1, 2 * K["kTileList"] + 1])
def test_tile_rounds(dev, oracle, vr, count):
    """(b) One tile with exactly `count` candidates, all of them matches: a round that never fills, one that fills with
    its last chunk, and one and two full rounds followed by a round of one."""
    s = S.tile_round_scene(count)
    assert s.tile_candidates[1, 1] == count
    _all_own_a_texel(s, _check(dev, oracle, vr, s, f"{count} candidates")[1])


def test_tile_round_ends_between_chunks(dev, oracle, vr):
    """(b) 3000 candidates of which every third matches tile (0, 0) and the others tile (2, 0): their rounds end at counts
    strictly between kTileList - kBlock and kTileList, with a part of the bin's list not yet looked at."""
    s = S.sparse_tile_scene()
    assert s.tile_candidates[0, 0] == 1000 and s.tile_candidates[0, 2] == 2000 and s.bin_counts[0, 0] == 3000
    _all_own_a_texel(s, _check(dev, oracle, vr, s, "sparse tile")[1])


@pytest.mark.parametrize("extra", [False, True], ids=["full", "over"])
def test_bin_capacity(dev, oracle, vr, extra):
    """(c) Bin (0, 0) with exactly kBinCapacity entries (its list is full and still used) and with one more (its tiles
    scan the whole queue).  15 triangles per meshlet: "main" takes a second trip of its stride loop."""
    s = S.bin_scene(extra)
    assert s.bin_counts[0, 0] == K["kBinCapacity"] + int(extra)
    assert len(s.lst) > K["mainGridPerCU"] * dev.compute_units * (K["kBlock"] // 64)
    _all_own_a_texel(s, _check(dev, oracle, vr, s, "bin " + ("over" if extra else "full"), threads=8)[1])


def test_full_queue(dev, oracle, vr):
    """(d) At least kQueueCapacity + 4096 triangles with boxes above kSmallBox at 2048x1024: the ones that find the queue
    full are drawn in place.  References: 16 disjoint slices of the list from 16 threads, max-merged."""
    s = S.queue_scene()
    assert s.queue_length >= K["kQueueCapacity"] + 4096
    _all_own_a_texel(s, _check(dev, oracle, vr, s, "full queue", threads=16)[1])


def test_tile_grid_stride(dev, oracle, vr):
    """(e) More tiles than the "tiles" launch has workgroups: the last tile (one pixel) is drawn by a workgroup's second
    trip.  Partial tiles on both edges."""
    s = S.stride_scene(dev.compute_units)
    tx, ty = s.tiles
    assert tx * ty > s.grid == K["tileGridPerCU"] * dev.compute_units and np.all(s.tile_candidates.reshape(-1)[s.grid:] >= 1)
    rdepth, _ = _check(dev, oracle, vr, s, f"{s.render[0]}x{s.render[1]}")
    assert rdepth[-1, -1] > 0 and np.count_nonzero(rdepth[-1]) > 600


@pytest.mark.parametrize("kind", ["normal", "guard"] + [f"tiny-{s}" for s in S.TINY] + ["no_cover", "small"])
def test_early_out(dev, oracle, vr, kind):
    """(f) Per tile 90 slivers whose samples round above their vertex depths, interleaved with quads that fill the tile at
    a depth just beyond the slivers' max * kSkipFactor.  normal: the cover 0..20 float32 steps above the slivers (both
    sides of the factor).  tiny-*: depths whose products with the weights are subnormal: samples exceed the bound, the
    kernel must not skip (kSkipMinDepth).  guard: both sides of kSkipMinDepth and kSkipMaxDepth.  no_cover / small: the
    tiny slivers with no early-out possible / drawn by "main": the arithmetic alone."""
    s = S.early_out_scene(kind)
    assert s.queue_length == (0 if kind == "small" else s.n_triangles)
    _check(dev, oracle, vr, s, kind)

