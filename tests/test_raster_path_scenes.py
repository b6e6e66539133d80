"""The preconditions of tests/test_gpu_raster_paths.py, on the references alone (no GPU): every listed triangle of every
owner scene owns a texel of the reference image, the predicted counts sit on the stated side of the constants read from
csrc/k_raster.hip, the early-out scenes have their witnesses, and the bound the kernel's early-out relies on (kSkipMinDepth
in k_raster.hip) holds inside its range and fails below it, as the sliver arithmetic shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_path_scenes as S  # noqa: E402
from suite_support import vr  # noqa: E402, F401

K = S.K
MI355X_CUS = 256                                     # the GPU test uses the device's own count
ROUNDS = [K["kTileList"] - K["kBlock"], K["kTileList"], K["kTileList"] + 1, 2 * K["kTileList"] + 1]


OWNER_SCENES = ([(f"a-{kind}", lambda kind=kind: S.small_box_scene(kind), 1) for kind in ("box1024", "box1025", "box33x32", "edge_clamped")]
                + [(f"b-{n}", lambda n=n: S.tile_round_scene(n), 1) for n in ROUNDS]
                + [("b-sparse", S.sparse_tile_scene, 1), ("c-full", lambda: S.bin_scene(False), 8), ("c-over", lambda: S.bin_scene(True), 8),
                   ("d-queue", S.queue_scene, 16)])


@pytest.mark.parametrize("name,make,threads", OWNER_SCENES, ids=[c[0] for c in OWNER_SCENES])
def test_every_listed_triangle_owns_a_texel(oracle, vr, name, make, threads):
    s = make()
    depth, vis = S.reference(oracle, vr, s, threads=threads)
    assert np.array_equal((vis >> np.uint64(32)).astype(np.uint32), depth.view(np.uint32)), "the two references disagree on the depth"
    present = np.unique(vis[vis != 0] & np.uint64(0xFFFFFFFF))
    missing = np.setdiff1d(s.payloads, present)
    assert len(missing) == 0 and len(present) == s.n_triangles, f"{name}: {len(missing)} of {s.n_triangles} listed triangles own no texel"


def test_small_box_counts():
    for kind, queued in (("box1024", False), ("box1025", True), ("box33x32", True)):
        s = S.small_box_scene(kind)
        assert np.all(s.live) and np.all(s.box_pixels == s.unclamped_pixels), kind
        assert (s.unclamped_pixels > K["kSmallBox"]) == queued and s.queue_length == (s.n_triangles if queued else 0), kind
        assert s.tile_candidates.max() >= (2 if queued else 0) and np.count_nonzero(s.tile_candidates) >= (12 if queued else 0)
    assert S.small_box_scene("box1024").unclamped_pixels == K["kSmallBox"] and S.small_box_scene("box1025").unclamped_pixels == K["kSmallBox"] + 1
    s = S.small_box_scene("edge_clamped")
    assert s.unclamped_pixels > K["kSmallBox"] and np.all(s.live) and s.queue_length == 0, "the clamp to the screen decides"
    assert s.box_pixels.max() == K["kSmallBox"] and s.box_pixels.min() < K["kSmallBox"]


def test_tile_round_counts():
    """Tile (1, 1) sees exactly kTileList - kBlock (one round, never "full"), kTileList (one round, full at its end),
    kTileList + 1 (a round of one follows) and 2 kTileList + 1 candidates, every one of them a match."""
    for n in ROUNDS:
        s = S.tile_round_scene(n)
        assert s.queue_length == n and s.bin_counts[0, 0] == n and np.count_nonzero(s.bin_counts) == 1
        assert s.tile_candidates[1, 1] == n and s.tile_candidates[0, 0] == 0
    s = S.sparse_tile_scene()
    assert s.queue_length == 3000 == s.bin_counts[0, 0] and np.count_nonzero(s.bin_counts) == 1
    # a third of the bin's list matches tile (0, 0), two thirds tile (2, 0): a round of either ends, in expectation, after
    # (kTileList - kBlock) * 3 or * 3 / 2 list entries at a count that no whole number of full chunks gives
    assert s.tile_candidates[0, 0] == 1000 and s.tile_candidates[0, 2] == 2000 and 0 < s.tile_candidates[0, 1] < 1000
    assert 1000 > K["kTileList"] - K["kBlock"] and 3000 > 2 * K["kTileList"]


def test_bin_counts():
    full, over = S.bin_scene(False), S.bin_scene(True)
    assert full.bin_counts[0, 0] == K["kBinCapacity"] == full.queue_length, "exactly full: the bin's list is still used"
    assert over.bin_counts[0, 0] == K["kBinCapacity"] + 1 == over.queue_length, "one more: the whole-queue scan"
    for s in (full, over):
        rest = s.bin_counts.copy(); rest[0, 0] = 0
        assert 0 < rest.max() < K["kBinCapacity"] // 4 and np.count_nonzero(rest) == 3
        assert len(s.lst) > K["mainGridPerCU"] * MI355X_CUS * (K["kBlock"] // 64), '"main" takes a second trip of its stride loop'


def test_queue_counts():
    s = S.queue_scene()
    assert s.queue_length >= K["kQueueCapacity"] + 4096 and s.queue_length == s.n_triangles
    assert s.bin_counts[:-1, :-1].max() > K["kBinCapacity"]
    assert len(s.lst) < (1 << 23)


def test_stride_counts():
    s = S.stride_scene(MI355X_CUS)
    tx, ty = s.tiles
    assert ty == 3 and tx * ty > s.grid and (tx - 1) * ty <= s.grid, "the fewest tiles that need a second trip"
    assert s.render[0] % K["kTile"] == 1 and s.render[1] % K["kTile"] == 1
    flat = s.tile_candidates.reshape(-1)
    assert np.all(flat[s.grid:] >= 1) and flat[0] >= 1 and np.count_nonzero(flat[tx:2 * tx]) >= 4 and np.count_nonzero(flat[2 * tx:]) >= 2
    assert s.queue_length == s.n_triangles


def _tile(a, i):
    return a[64 * (i // 8):64 * (i // 8) + 64, 64 * (i % 8):64 * (i % 8) + 64]


def _covers_alone(oracle, s):
    c = S.build(s.render, s.tris[s.is_cover])
    depth = np.zeros(s.render[::-1], np.float32)
    return oracle.raster_depth(c.k, c.sc, c.v, c.vid, c.tri, c.rec, c.lst, depth)


@pytest.mark.parametrize("kind", ["normal", "guard"] + [f"tiny-{s}" for s in S.TINY])
def test_early_out_scene_has_its_witnesses(oracle, vr, kind):
    """Per tile: far = the smallest depth the covers alone leave; the kernel may skip the tile's slivers once
    fl(max * kSkipFactor) < far.  Inside [kSkipMinDepth, kSkipMaxDepth) no sliver sample may then show (the bound holds);
    below it at least 8 texels must show a sliver in front of the covers (the witnesses a skipping kernel would lose)."""
    s = S.early_out_scene(kind)
    assert s.queue_length == s.n_triangles
    ref, _ = S.reference(oracle, vr, s, texels=False)
    cov = _covers_alone(oracle, s)
    witnesses = in_front_near = 0
    for i, (cover, d) in enumerate(s.cases):
        far = _tile(cov, i).min()
        assert far > 0, "the covers fill the tile"
        shows = int(np.count_nonzero(_tile(ref, i) > _tile(cov, i)))
        skippable = S.skip_bound(d) < far
        proven = K["kSkipMinDepth"] <= max(d) < K["kSkipMaxDepth"]
        if skippable and proven:
            assert shows == 0, f"{kind} tile {i}: {shows} samples exceed max * kSkipFactor inside the proven range"
        if skippable and not proven:
            witnesses += shows
        if not skippable:
            in_front_near += shows
    if kind == "normal":
        skippable = [S.skip_bound(d) < _tile(cov, i).min() for i, (_, d) in enumerate(s.cases)]
        assert not skippable[0] and skippable[-1] and in_front_near > 0, "both sides of the factor; a sample that rounds above the cover shows"
    elif kind == "guard":
        assert witnesses == 0                        # normal depths just below kSkipMinDepth still obey the bound: the guard is conservative
    else:
        print(f"{kind}: {witnesses} witness texels")
        assert witnesses >= 8


def test_controls_queue_and_draw_in_place():
    assert S.early_out_scene("no_cover").queue_length == S.early_out_scene("no_cover").n_triangles
    assert S.early_out_scene("small").queue_length == 0


def test_sliver_samples_exceed_the_bound_only_below_its_range(oracle):
    """The sliver (0.5, 0.5) (40.5, 40.5) (20.5 + delta, 20.5 - delta) with vertex depths s * (1.9, 1.9, 1): the number of
    samples above max * kSkipFactor.  None while the products e_i * d_i stay normal; some once they do not."""
    counts = {}
    for delta in (1e-2, 1e-3, 1e-4):
        for name, scale in (("1e-37", 1e-37), ("1e-20", 1e-20), ("min", float(K["kSkipMinDepth"]) / 1.9), *S.TINY.items()):
            d = S.sliver_depths(scale)
            t = np.array([[(0.5, 0.5, d[0]), (40.5, 40.5, d[1]), (20.5 + delta, 20.5 - delta, d[2])]], np.float64)
            s = S.build((512, 512), t, exact=False)
            depth = np.zeros((512, 512), np.float32)
            oracle.raster_depth(s.k, s.sc, s.v, s.vid, s.tri, s.rec, s.lst, depth)
            assert np.count_nonzero(depth) == 41, "the centres on the long edge"
            counts[delta, name] = int(np.count_nonzero(depth > S.skip_bound(d)))
    print(counts)
    for delta in (1e-2, 1e-3, 1e-4):
        assert counts[delta, "1e-37"] == 0 and counts[delta, "1e-20"] == 0 and counts[delta, "min"] == 0
        assert counts[delta, "1e-41"] > 0
    assert counts[1e-3, "1e-39"] > 0 and counts[1e-4, "1e-39"] > 0 and counts[1e-4, "2e-38"] > 0
