"""The preconditions of tests/test_gpu_raster_paths.py and tests/test_gpu_alpha_raster_paths.py, on the references alone (no GPU): every listed triangle of every
owner scene owns a texel of the reference image, the predicted counts sit on the stated side of the constants read from
csrc/k_raster.hip, the early-out scenes have their witnesses, and the bound the kernel's early-out relies on (kSkipMinDepth
in k_raster.hip) holds inside its range and fails below it, as the sliver arithmetic shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import raster_path_scenes as S  # noqa: E402
from suite_support import at, vr  # noqa: E402, F401

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


# ---- the alpha-tested rasters: the preconditions of tests/test_gpu_alpha_raster_paths.py --------------------------------------------
LOW = np.uint64(0xFFFFFFFF)
_IMAGES = {}


def _images(oracle, vr, at, name):
    """(scene, alpha depth, alpha texels, counts, no-discard texels) of one of S.ALPHA_OWNER_SCENES, computed once."""
    if name not in _IMAGES:
        make, _, _, threads = S.ALPHA_OWNER_SCENES[name]
        s = make(MI355X_CUS)
        depth, vis, counts = S.alpha_reference(at, s, threads)
        _, plain = S.reference(oracle, vr, s, threads=threads)
        _IMAGES[name] = (s, depth, vis, counts.astype(np.int64), plain)
    return _IMAGES[name]


def _witnesses(s, vis, plain):
    """The triangles (indices into s.payloads) whose discard shows: the no-discard image's payloads where the two images differ."""
    shows = (vis != plain) & (plain != 0)
    return np.unique(S.triangle_of(s, np.unique(plain[shows] & LOW)))


def test_alpha_reference_slices_merge_to_the_unsliced_call(at):
    """16 disjoint slices of the list into images of their own, max-merged, equal the unsliced call word for word, and their
    counts add up to its counts: on the rule scene (15 instances, 75 triangles, 5 per slice; textured, constant and broken
    materials) through both launches' box sizes."""
    for path in ("main", "tiles"):
        s = S.rules_alpha(path)
        d1, v1, c1 = S.alpha_reference(at, s, 1)
        d16, v16, c16 = S.alpha_reference(at, s, 16)
        assert np.array_equal(d1.view(np.uint32), d16.view(np.uint32)) and np.array_equal(v1, v16) and np.array_equal(c1, c16)
        assert c1.sum() > 20000 and np.count_nonzero(v1) > 5000
        some = np.array([0, 3, 4, 7, 11, 13], np.uint32)                 # a subset: its payloads carry the list's own positions
        _, vs, _ = S.alpha_reference(at, s, 2, positions=some)
        assert set(np.unique((vs[vs != 0] & LOW) >> np.uint64(7) & np.uint64(0x7FFFFF)).tolist()) <= set(some.tolist())
        assert np.all((vs == 0) | (vs == v1) | (vs < v1))


@pytest.mark.parametrize("name", list(S.ALPHA_OWNER_SCENES))
def test_alpha_owner_scene_preconditions(oracle, vr, at, name):
    """For every owner scene of the GPU file, on the references alone: every listed triangle owns a texel of the alpha image;
    the samples were counted on the path the case names; textured: at least a quarter of the covered samples kept and a
    quarter discarded; slivers: every apex texel belongs to its triangle and at least one sample per two triangles is
    discarded; the discard shows (the two images differ) on texels of at least one triangle in eight.
    MEASURED (kept / discarded samples, owners of listed, witness triangles, differing texels):
      a-box1024      6144 /    5760,   24 of   24,   24,  1884 (main)      a-box1025      5760 /    5856,   24 of   24,   24,  1902
      a-box33x32     6144 /    5760,   24 of   24,   24,  1884             a-edge_clamped 4096 /    3823,   16 of   16,   12,  1231 (main)
      b-768        219648 /  185856,  768 of  768,  453,  1834             b-1024       292864 /  247808, 1024 of 1024,  583,  2024
      b-1025       293180 /  248020, 1025 of 1025,  582,  2016             b-2049       586044 /  495828, 2049 of 2049, 1102,  2776
      b-sparse     860160 /  723840, 3000 of 3000, 1614,  4314             e-stride      13337 /   12256,    7 of    7,    7, 11373
      c-full        65536 /   65536, all 65536, 65536, 65536               c-over        65537 /   65537, all 65537, 65536 (the extra entry among them), 65536
      d-slivers   1114112 / 1114112, all 1114112, 1114112, 1114112
    With uv = offset / 16 and no shift, as first specified, the round cases had 75 / 79 / 78 / 94 / 170 witness triangles (the
    block's rim only: under one in eight) and every triangle the same texture coordinates, so they use S.ROUND_PHASE on the
    even rows (raster_path_scenes.py says why)."""
    make, path, flavour, _ = S.ALPHA_OWNER_SCENES[name]
    s, depth, vis, counts, plain = _images(oracle, vr, at, name)
    assert np.array_equal((vis >> np.uint64(32)).astype(np.uint32), depth.view(np.uint32)), "the reference's two images disagree on the depth"
    present = np.unique(vis[vis != 0] & LOW)
    assert np.array_equal(present, np.sort(s.payloads)), f"{name}: {len(np.setdiff1d(s.payloads, present))} of {s.n_triangles} listed triangles own no texel"
    here, other = (counts[:2], counts[2:]) if path == "main" else (counts[2:], counts[:2])
    assert other.sum() == 0 and here.sum() > 0 and s.queue_length == (0 if path == "main" else s.n_triangles), (name, counts)
    kept, gone = int(here[0]), int(here[1])
    wit = _witnesses(s, vis, plain)
    print(f"{name}: kept {kept}, discarded {gone}, owners {len(present)} of {s.n_triangles}, witness triangles {len(wit)}, differing texels {int(np.count_nonzero(vis != plain))}")
    if flavour == "textured":
        assert 4 * kept >= kept + gone and 4 * gone >= kept + gone, (name, counts)
    else:
        tris = s.tris_px
        ax, ay = np.floor(tris[:, 0, 0] + 0.5).astype(np.int64), np.floor(tris[:, 0, 1]).astype(np.int64)      # the first covered centre
        n = len(tris)
        for i, (dx, dy) in enumerate(s.cells):
            assert np.array_equal(vis[ay + dy, ax + dx] & LOW, s.payloads[i * n:(i + 1) * n]), f"{name}: an apex sample of instance {i} is not kept"
        assert 2 * gone >= s.n_triangles and kept >= s.n_triangles
    assert 8 * len(wit) >= s.n_triangles, (name, len(wit))
    # the discard is visible where the path is
    if name in ("b-1025", "b-2049"):
        assert wit.max() >= K["kTileList"] and (name != "b-2049" or wit.max() >= 2 * K["kTileList"])
        assert np.count_nonzero(wit >= K["kTileList"]) >= (1 if name == "b-1025" else K["kTileList"] // 8)
    if name.startswith("b-"):
        n = int(name[2:]) if name != "b-sparse" else None
        assert (s.tile_candidates[1, 1] == n) if n else (s.tile_candidates[0, 0] == 1000 and s.tile_candidates[0, 2] == 2000 and s.bin_counts[0, 0] == 3000)
    if name in ("c-full", "c-over"):
        extra = int(name == "c-over")
        assert s.bin_counts[0, 0] == K["kBinCapacity"] + extra == s.queue_length
        assert len(s.lst) > K["mainGridPerCU"] * MI355X_CUS * (K["kBlock"] // 64), '"main" takes a second trip of its stride loop'
        assert np.count_nonzero(wit < K["kBinCapacity"]) >= K["kBinCapacity"] // 8 and (not extra or wit.max() == K["kBinCapacity"]), "both sides of kBinCapacity"
    if name == "d-slivers":
        assert s.queue_length >= K["kQueueCapacity"] + 4096 and len(s.lst) < (1 << 23)
        assert len(wit) == s.n_triangles, "which triangles find the queue full is not determined: every one is a witness"
    if name == "e-stride":
        tx, ty = s.tiles
        assert tx * ty > s.grid and depth[-1, -1] > 0 and np.count_nonzero(depth[-1]) > 200, "the last one-pixel tile is non-empty"


def test_constant_alpha_queue_scene_equals_the_kept_instances(oracle, vr, at):
    """(d) queue_scene() with its 17 instances cycling through constant alpha above the cutoff, below it and a broken chain:
    at_raster's images equal vr_raster / orc_raster_depth over the list positions of the 6 kept instances, and each of their
    393 216 triangles owns a texel.  MEASURED: 207 618 048 samples kept (6 instances) and as many discarded (the 6 below the cutoff;
    the 5 broken chains are not counted), all on the tile path; queue length 1 114 112 >= 2^20 + 4096."""
    s = S.queue_constant_alpha()
    assert s.queue_length >= K["kQueueCapacity"] + 4096 and len(s.kept_positions) * 3 >= len(s.lst) and len(s.kept_positions) * 2 < len(s.lst)
    depth, vis, counts = S.alpha_reference(at, s, 16)
    rdepth, rvis = S.reference(oracle, vr, s, threads=16, positions=s.kept_positions)
    assert np.array_equal(depth.view(np.uint32), rdepth.view(np.uint32)) and np.array_equal(vis, rvis)
    print("constant alpha queue:", counts.tolist())
    assert counts[0] == counts[1] == 0 and counts[2] == counts[3] == 6 * (s.n_triangles // 17) * 528
    kept = (np.arange(s.n_triangles) // (s.n_triangles // len(s.sc["instances"]))) % 3 == S.M_ABOVE
    assert np.array_equal(np.unique(vis[vis != 0] & LOW), np.sort(s.payloads[kept]))


@pytest.mark.parametrize("cover", S.EARLY_OUT_COVERS)
def test_early_out_alpha_scenes(oracle, vr, at, cover):
    """(f) 8 tiles, the covers listed first (4 instances of 8 quads a tile), 23 kept slivers a tile, each 2^-10 behind the one before.
    checker: every tile shows at least 8 texels of slivers through the covers' holes, and every sliver, the farthest included, owns
    one but at most one per tile (MEASURED: 492 such texels in every tile; 23, 22, 22, ... of 23 slivers own a texel); a quarter of the
    covers' samples kept, a quarter discarded (MEASURED: 524 288 kept, 540 672 discarded).
    opaque: the image equals the no-discard image word for word.  below: it equals the image of the slivers alone.  All queued."""
    s = S.early_out_alpha(cover)
    T, n_sl, n_c = s.n_tiles, s.slivers_per_tile, s.n_cover_triangles
    assert s.queue_length == s.n_triangles and T == 8 and n_c == T * 64
    depth, vis, counts = S.alpha_reference(at, s, 16)
    rdepth, plain = S.reference(oracle, vr, s, threads=4)
    assert counts[0] == counts[1] == 0
    skippable = [S.skip_bound(d) < c for c, d in s.cases]
    assert not skippable[0] and sum(skippable) >= 2, "covers on both sides of the factor"
    if cover == "opaque":
        assert counts[3] == 0 and np.array_equal(vis, plain) and np.array_equal(depth.view(np.uint32), rdepth.view(np.uint32))
    elif cover == "below":
        sdepth, svis = S.reference(oracle, vr, s, positions=s.positions[1])
        assert np.array_equal(vis, svis) and np.array_equal(depth.view(np.uint32), sdepth.view(np.uint32)) and np.count_nonzero(vis) > T * 300
    else:
        covers_kept = int(counts[2]) - T * n_sl * 41
        assert 4 * covers_kept >= n_c * 2048 and 4 * int(counts[3]) >= n_c * 2048, counts
        owner = np.full(vis.shape, -1, np.int64); owner[vis != 0] = S.triangle_of(s, vis[vis != 0] & LOW)
        before = np.full(vis.shape, -1, np.int64); before[plain != 0] = S.triangle_of(s, plain[plain != 0] & LOW)
        through = (owner >= n_c) & (before >= 0) & (before < n_c)          # a sliver where the no-discard image shows a cover
        per_tile = [int(np.count_nonzero(_tile(through, i))) for i in range(T)]
        owners = [len(np.unique(_tile(owner, i)[_tile(owner, i) >= n_c])) for i in range(T)]
        print("slivers through holes per tile:", per_tile, "slivers that own a texel per tile:", owners, counts.tolist())
        assert min(per_tile) >= 8 and min(owners) >= n_sl - 1
        last = n_c + n_sl * np.arange(T) + n_sl - 1
        assert all(np.count_nonzero(_tile(owner, i) == last[i]) >= 1 for i in range(T)), "the farthest sliver of every tile shows"


@pytest.mark.parametrize("path", ["main", "tiles"])
@pytest.mark.parametrize("table", [True, False], ids=["table", "no table"])
def test_rule_scenes_show_the_kept_instances(at, path, table):
    """(g), (h) One instance per case of S.RULE_CASES: the reference shows all five triangles of every instance the convention
    keeps and nothing of the others; without a table the textured ones go too.  MEASURED: with the table 7 of 15 instances (35
    triangles), without it 3 (15 triangles); the samples are counted on the path the case names."""
    s = S.rules_alpha(path, table)
    _, vis, counts = S.alpha_reference(at, s, 1)
    tri = np.unique(S.triangle_of(s, vis[vis != 0] & LOW))
    want = np.flatnonzero(np.repeat(s.kept, 5))
    assert np.array_equal(tri, want), (tri, want)
    assert sum(s.kept) == (7 if table else 3)
    assert (counts[2:].sum() == 0) == (path == "main") and (counts[:2].sum() == 0) == (path == "tiles") and s.queue_length == (0 if path == "main" else 75)
