"""Scenes that put the compute rasteriser (csrc/k_raster.hip) on both sides of each of its path switches, with the
counts the kernel's own rules predict for them (tests/test_raster_path_scenes.py, tests/test_gpu_raster_paths.py), and, in the
file's second half, their variants for the alpha-tested instantiations (tests/test_gpu_alpha_raster_paths.py).

Every scene is authored in pixel space: m_WorldToClip is the identity (w = 1, depth = object-space z), m_NearPlane is 0.5
and a vertex at pixel position (px, py) is stored as x = px / halfW - 1, y = 1 - py / halfH.  With a power-of-two render
size and positions that are multiples of a small power of two the vertex stage returns px, py and z exactly (checked
here, in float64), so bounding boxes, queue lengths, bin counts and candidates per tile are exact numbers.

The OWNER scene: triangle i has its right angle at the pixel corner (X_i, Y_i), legs along +x and +y and the constant
depth 0.25 + (X_i + Y_i) * 2^-14.  It covers the pixel (X_i, Y_i).  Every triangle that covers a pixel p has its corner
up and left of p, so the one whose corner is p is the nearest there (reverse Z: larger is nearer): with distinct corners
every triangle owns at least the texel of its corner, and a rasteriser that drops any triangle changes the image."""
import os
import re
from types import SimpleNamespace

import numpy as np

from toyrenderer_amd import interop as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "toyrenderer_amd", "csrc", "k_raster.hip")

_PATTERNS = {
    "kBlock": r"constexpr uint32_t kBlock = (\d+);",
    "kSmallBox": r"constexpr uint32_t kSmallBox = (\d+);",
    "kTile": r"constexpr uint32_t kTile = (\d+);",
    "kQueueCapacity": r"constexpr uint32_t kQueueCapacity = 1u << (\d+);",
    "kTileList": r"constexpr uint32_t kTileList = (\d+);",
    "kBinShift": r"constexpr uint32_t kBinShift = (\d+);",
    "kBinCapacity": r"constexpr uint32_t kBinCapacity = 1u << (\d+);",
    "mainGridPerCU": r"const uint32_t grid = ctx\.computeUnits\(\) \* (\d+)u;",
    "tileGridPerCU": r"const uint32_t tileGrid = tiles < ctx\.computeUnits\(\) \* (\d+)u \? tiles : ctx\.computeUnits\(\) \* \1u;",
    "kSkipFactor": r"constexpr float kSkipFactor = (0x[0-9a-fp.+-]+)f;",
    "kSkipMinDepth": r"constexpr float kSkipMinDepth = (0x[0-9a-fp.+-]+)f;",
    "kSkipMaxDepth": r"constexpr float kSkipMaxDepth = (0x[0-9a-fp.+-]+)f;",
}
_SHIFTS = {"kQueueCapacity", "kBinCapacity"}
# the rules the predictions restate
_RULES = [
    r"bool big = live && \(uint64_t\)bw \* bh > kSmallBox && a\.queue != nullptr;",
    r"if \(big && slot < kQueueCapacity\) \{",
    r"if \(k < kBinCapacity\) a\.binList\[\(uint64_t\)bin \* kBinCapacity \+ k\] = slot;",
    r"const bool wholeQueue = binned > kBinCapacity;",
    r"const bool full = s_count \+ kBlock > kTileList;",
    r"for \(uint32_t tile = blockIdx\.x; tile < tilesX \* tilesY; tile \+= gridDim\.x\) \{",
    r"for \(uint32_t v = blockIdx\.x \* kWaves \+ wave; v < V; v \+= gridDim\.x \* kWaves\) \{",
    r"if \(far \* kSkipFactor < tileFar && far >= kSkipMinDepth && far < kSkipMaxDepth\) continue;",
    r"if \(\(k & 31u\) == 0u && \(k != 0u \|\| any\)\) \{",
]


def constants():
    """The rasteriser's switches, read from its source so that the cases follow the code."""
    with open(KERNEL) as f:
        text = f.read()
    out = {}
    for key, pat in _PATTERNS.items():
        m = re.search(pat, text)
        assert m, f"k_raster.hip: {key} no longer matches {pat!r}"
        if key.startswith("kSkip"):
            out[key] = np.float32(float.fromhex(m.group(1)))
        else:
            out[key] = (1 << int(m.group(1))) if key in _SHIFTS else int(m.group(1))
    for pat in _RULES:
        assert re.search(pat, text), f"k_raster.hip: the rule {pat!r} is no longer there"
    return out


K = constants()
SLOT = 1                                    # the pass slot of every scene's texels


def _range_count(shape, y0, y1, x0, x1):
    """[shape] counts: how many of the inclusive index boxes [y0, y1] x [x0, x1] contain each cell."""
    d = np.zeros((shape[0] + 1, shape[1] + 1), np.int64)
    np.add.at(d, (y0, x0), 1); np.add.at(d, (y0, x1 + 1), -1); np.add.at(d, (y1 + 1, x0), -1); np.add.at(d, (y1 + 1, x1 + 1), 1)
    return d.cumsum(0).cumsum(1)[:-1, :-1]


def build(render, tris, per_meshlet=21, instances=((0, 0),), exact=True):
    """The scene of `tris` ([n, 3, 3] float64: px, py, z per vertex), `per_meshlet` (<= 21: three vertices each) to a
    meshlet, drawn under one instance per (dx, dy) of `instances`: a translation by whole pixels, and in z by
    (dx + dy) * 2^-14.  Returns the arrays of a direct dispatch and the predictions from the kernel's rules."""
    W, H = render
    halfW, halfH = 0.5 * W, 0.5 * H
    tris = np.asarray(tris, np.float64)
    n = len(tris)
    assert 1 <= per_meshlet <= 21 and n > 0
    v = np.zeros(3 * n, I.RawVertexFormat)
    pos = np.stack([tris[:, :, 0] / halfW - 1.0, 1.0 - tris[:, :, 1] / halfH, tris[:, :, 2]], 2).reshape(-1, 3)
    v["m_Position"] = pos.astype(np.float32)
    inst = np.zeros(len(instances), I.BasePassInstanceConstants)
    inst["m_WorldMatrix"][:] = np.eye(4, dtype=np.float32)
    shift = np.array([(dx / halfW, -dy / halfH, (dx + dy) * 2.0 ** -14) for dx, dy in instances], np.float64)
    inst["m_WorldMatrix"][:, 3, :3] = shift.astype(np.float32)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    # what the vertex stage computes: position + translation (one rounding), then fma(x, half, half): (n_inst, 3n, 3)
    p32 = v["m_Position"].astype(np.float64)[None] + inst["m_WorldMatrix"][:, 3, :3].astype(np.float64)[:, None]
    if exact:
        assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos), "a vertex is not a float32"
        assert np.array_equal(p32.astype(np.float32).astype(np.float64), p32), "a translated vertex is not a float32"
    p32 = p32.astype(np.float32).astype(np.float64)
    sx, sy = p32[..., 0] * halfW + halfW, -p32[..., 1] * halfH + halfH
    if exact:
        want = tris[None] + np.array([(dx, dy, (dx + dy) * 2.0 ** -14) for dx, dy in instances], np.float64)[:, None, None]
        assert np.array_equal(sx.reshape(-1, n, 3), want[..., 0]) and np.array_equal(sy.reshape(-1, n, 3), want[..., 1])
        assert np.array_equal(p32[..., 2].reshape(-1, n, 3), want[..., 2])
        assert np.array_equal(sx.astype(np.float32).astype(np.float64), sx) and np.array_equal(sy.astype(np.float32).astype(np.float64), sy)
    sx, sy = sx.astype(np.float32).reshape(-1, 3), sy.astype(np.float32).reshape(-1, 3)     # (n_inst * n, 3)
    # meshlets, one mesh, one LOD; records of 32 meshlets; the list in instance, meshlet order
    n_meshlets = (n + per_meshlet - 1) // per_meshlet
    meshlets = np.zeros(n_meshlets, I.MeshletData)
    first = np.arange(n_meshlets, dtype=np.uint32) * per_meshlet
    nt = np.minimum(per_meshlet, n - first).astype(np.uint32)
    meshlets["m_MeshletVertexIDsBufferIdx"] = 3 * first
    meshlets["m_MeshletIndexIDsBufferIdx"] = first
    meshlets["m_VertexAndTriangleCount"] = (3 * nt) | (nt << 8)
    local = 3 * (np.arange(n, dtype=np.uint32) % per_meshlet)
    tri = (local | ((local + 1) << 8) | ((local + 2) << 16)).astype(np.uint32)
    vid = np.arange(3 * n, dtype=np.uint32)
    md = np.zeros(1, I.MeshData)
    md["m_NumLODs"] = 1
    md["m_MeshLODDatas"]["m_NumMeshlets"][0][0] = n_meshlets
    groups = (n_meshlets + 31) // 32
    rec = np.zeros(groups * len(instances), I.MeshletAmplificationData)
    rec["m_InstanceConstIdx"] = np.repeat(np.arange(len(instances), dtype=np.uint32), groups)
    rec["m_MeshletGroupOffset"] = np.tile(32 * np.arange(groups, dtype=np.uint32), len(instances))
    m = np.arange(n_meshlets, dtype=np.uint32)
    lst = (((np.arange(len(instances), dtype=np.uint32)[:, None] * groups + m[None] // 32) << 5) | (m[None] % 32)).reshape(-1).astype(np.uint32)
    k = np.zeros(1, I.BasePassConstants)
    k["m_WorldToClip"] = np.eye(4, dtype=np.float32)
    k["m_PrevWorldToClip"] = np.eye(4, dtype=np.float32)
    k["m_NearPlane"] = 0.5
    k["m_OutputResolution"] = (W, H)
    # payload of every listed triangle: list position << 7 | triangle in the meshlet, in instance, triangle order
    t_all = np.tile(np.arange(n, dtype=np.uint64), len(instances))
    pos_all = np.repeat(np.arange(len(instances), dtype=np.uint64), n) * np.uint64(n_meshlets) + t_all // np.uint64(per_meshlet)
    payloads = (np.uint64(SLOT) << np.uint64(30)) | (pos_all << np.uint64(7)) | (t_all % np.uint64(per_meshlet))
    # ---- the kernel's rules, restated: live box, queued, bins, tile candidates ------------------------------------------
    area = ((sx[:, 1] - sx[:, 0]).astype(np.float64) * (sy[:, 2] - sy[:, 0]).astype(np.float64)
            - (sy[:, 1] - sy[:, 0]).astype(np.float64) * (sx[:, 2] - sx[:, 0]).astype(np.float64))
    fminx, fmaxx, fminy, fmaxy = sx.min(1), sx.max(1), sy.min(1), sy.max(1)
    on = (area != 0) & (fmaxx >= 0) & (fmaxy >= 0) & (fminx <= W) & (fminy <= H)
    bx0 = np.maximum(np.floor(fminx), 0).astype(np.int64); bx1 = np.minimum(np.ceil(fmaxx), W - 1).astype(np.int64)
    by0 = np.maximum(np.floor(fminy), 0).astype(np.int64); by1 = np.minimum(np.ceil(fmaxy), H - 1).astype(np.int64)
    live = on & (bx1 >= bx0) & (by1 >= by0)
    pixels = np.where(live, (bx1 - bx0 + 1) * (by1 - by0 + 1), 0)
    queued = live & (pixels > K["kSmallBox"])
    q = np.flatnonzero(queued)
    bs, T = K["kBinShift"], K["kTile"]
    binsX, binsY = (W + (1 << bs) - 1) >> bs, (H + (1 << bs) - 1) >> bs
    tilesX, tilesY = (W + T - 1) // T, (H + T - 1) // T
    bins = _range_count((binsY, binsX), by0[q] >> bs, by1[q] >> bs, bx0[q] >> bs, bx1[q] >> bs)
    cand = _range_count((tilesY, tilesX), by0[q] // T, by1[q] // T, bx0[q] // T, bx1[q] // T)
    return SimpleNamespace(render=(W, H), k=k, sc=dict(instances=inst, meshData=md, meshlets=meshlets), v=v, vid=vid, tri=tri, rec=rec, lst=lst,
                           payloads=payloads, n_triangles=len(payloads), live=live, box_pixels=pixels, queued=queued, queue_length=len(q),
                           bin_counts=bins, tile_candidates=cand, tiles=(tilesX, tilesY))


def owner_tris(apex, legs=(33, 32), z=None):
    """[n, 3, 3]: right angle at the pixel corner apex[i], legs along +x and +y, constant depth z[i] (default: the owner rule's)."""
    apex = np.asarray(apex, np.float64).reshape(-1, 2)
    legs = np.broadcast_to(np.asarray(legs, np.float64), apex.shape)
    if z is None:
        z = 0.25 + (apex[:, 0] + apex[:, 1]) * 2.0 ** -14
    t = np.zeros((len(apex), 3, 3))
    t[:, :, 0] = apex[:, None, 0]; t[:, :, 1] = apex[:, None, 1]
    t[:, 1, 0] += legs[:, 0]; t[:, 2, 1] += legs[:, 1]
    t[:, :, 2] = np.broadcast_to(np.asarray(z, np.float64), (len(apex),))[:, None]
    return t


def _pixels_of(x0, y0, count, width=64):
    """The first `count` pixels of the `width`-wide square at (x0, y0), row by row."""
    i = np.arange(count)
    return np.stack([x0 + i % width, y0 + i // width], 1)


# ---- (a) kSmallBox ---------------------------------------------------------------------------------------------------
def small_box_scene(kind):
    """512x512.  Boxes of bw x bh pixels (legs bw - 1, bh - 1 from a pixel corner) inside a tile, across a tile corner, across
    a bin corner and ending on the last column / row.  "edge_clamped": the 33x32 box one pixel further, so that the clamp
    to the screen brings it back to 32x32 (right) and 33x31 (bottom)."""
    W = H = 512
    bw, bh = {"box1024": (32, 32), "box1025": (41, 25), "box33x32": (33, 32), "edge_clamped": (33, 32)}[kind]
    lx, ly = bw - 1, bh - 1
    if kind == "edge_clamped":
        base = [(W - lx, 100), (W - lx, 300), (200, H - ly), (W - lx, H - ly)]
    else:
        base = [(70, 70), (128 - 16, 128 - 12), (256 - 20, 256 - 9), (W - 1 - lx, 40), (30, H - 1 - ly), (W - 1 - lx, H - 1 - ly)]
    sign = 1 if kind == "edge_clamped" else -1                       # neighbours: further out / further in
    apex = np.array([(x + sign * dx, y + sign * dy) for x, y in base for dx, dy in ((0, 0), (1, 0), (0, 1), (3, 2))], np.float64)
    s = build((W, H), owner_tris(apex, (lx, ly)))
    s.unclamped_pixels = bw * bh
    return s


# ---- (b) tile rounds -------------------------------------------------------------------------------------------------
def tile_round_scene(count):
    """512x512.  `count` corners in tile (1, 1), row by row: every one of them is a candidate of that tile, and of no
    other bin than (0, 0)."""
    return build((512, 512), owner_tris(_pixels_of(64, 64, count)))


def sparse_tile_scene(matching=1000):
    """512x512.  Triangle 3j has its corner in tile (0, 0); 3j + 1 and 3j + 2 have theirs in tile (2, 0) of the same bin
    and do not reach tile (0, 0) or (1, 0)."""
    a, b = _pixels_of(0, 0, matching), _pixels_of(128, 0, 2 * matching)
    apex = np.zeros((3 * matching, 2))
    apex[0::3], apex[1::3], apex[2::3] = a, b[0::2], b[1::2]
    return build((512, 512), owner_tris(apex))


# ---- (c) kBinCapacity ------------------------------------------------------------------------------------------------
def _bin_tris(extra):
    side = 1 << K["kBinShift"]
    assert side * side == K["kBinCapacity"], "one corner per pixel of a bin fills its list exactly"
    t = owner_tris(_pixels_of(0, 0, side * side, side))
    if extra:
        # one more entry of bin (0, 0): its box begins in the bin's last column, its first covered centre is in the next bin;
        # nearer than everything, so it owns what it covers
        e = owner_tris([(side - 0.25, 10.0)], z=np.array([0.25 + 2000 * 2.0 ** -14]))
        t = np.concatenate([t, e])
    return t


def bin_scene(extra=False, per_meshlet=15):
    """512x512.  One corner per pixel of bin (0, 0): 2^16 entries, the bin's capacity.  extra: 2^16 + 1."""
    return build((512, 512), _bin_tris(extra), per_meshlet=per_meshlet)


# ---- (d) kQueueCapacity ----------------------------------------------------------------------------------------------
def queue_scene(per_meshlet=21):
    """2048x1024.  The full bin's geometry under enough instances, a bin apart, to queue at least kQueueCapacity + 4096
    triangles; no instance in the last bin column or row."""
    W, H = 2048, 1024
    side = 1 << K["kBinShift"]
    need = -(-(K["kQueueCapacity"] + 4096) // K["kBinCapacity"])
    cells = [(bx * side, by * side) for by in range(H // side - 1) for bx in range(W // side - 1)]
    assert need <= len(cells)
    return build((W, H), _bin_tris(False), per_meshlet=per_meshlet, instances=cells[:need])


# ---- (e) the tile launch's grid stride -------------------------------------------------------------------------------
def stride_scene(compute_units):
    """The smallest render with three tile rows, the last a pixel high, and more tiles than the "tiles" grid has
    workgroups; the last column is a pixel wide.  100-pixel triangles in the first tiles, in those with the highest
    indices and across the last row and column."""
    T = K["kTile"]
    grid = K["tileGridPerCU"] * compute_units
    tilesX = grid // 3 + 1
    W, H = (tilesX - 1) * T + 1, 2 * T + 1
    assert tilesX * 3 > grid and W <= 0xFFFF
    t = []
    for x, y, z in [(10.0, 5.0, 0.30), (W - 150.0, 20.0, 0.31), (W - 90.0, 60.0, 0.32), (W - 260.0, 70.0, 0.33), (W / 2.0, 90.0, 0.34)]:
        t.append([(x, y, z), (x + 100.0, y + 3.0, z + 0.05), (x + 4.0, y + 100.0, z + 0.11)])
    t.append([(W - 100.0, H + 20.0, 0.40), (W + 20.0, H + 20.0, 0.45), (W + 20.0, H - 100.0, 0.35)])   # covers the last pixel
    t.append([(W - 700.5, H - 1.25, 0.21), (W + 30.0, H - 1.25, 0.22), (W + 30.0, H + 60.0, 0.23)])      # the last row alone
    s = build((W, H), np.array(t), exact=False)
    s.grid = grid
    return s


# ---- (f) the far-depth early-out ------------------------------------------------------------------------------------
def step(x, n):
    """float32 x moved n float32 steps up."""
    return (np.array([x], np.float32).view(np.uint32).astype(np.int64) + n).astype(np.uint32).view(np.float32)[0]


def _tile_content(tx0, ty0, cover, depths, small=False, n_slivers=90, n_quads=8):
    """Slivers whose pixel centres lie exactly on the long edge (x+.5, y+.5) .. (x+L+.5, y+L+.5), third vertex
    (x + L/2 + .5 + delta, y + L/2 + .5 - delta), delta in 2^-7, 2^-10, 2^-13, vertex depths `depths`; every
    n_slivers / n_quads slivers a quad of two triangles that covers the whole tile (small: its 24x24 corner) at depth
    `cover` (None: no quads)."""
    L, S = (12, 24) if small else (40, 64)
    span = S - L - 1
    out, cover_flags = [], []
    every = n_slivers // n_quads
    for j in range(n_slivers):
        x, y = tx0 + (5 * j) % span, ty0 + (7 * j) % span
        d = 2.0 ** -(7 + 3 * (j % 3))
        out.append([(x + 0.5, y + 0.5, depths[0]), (x + L + 0.5, y + L + 0.5, depths[1]), (x + L / 2 + 0.5 + d, y + L / 2 + 0.5 - d, depths[2])])
        cover_flags.append(False)
        if cover is not None and j % every == 0 and j // every < n_quads:
            out.append([(tx0, ty0, cover), (tx0 + S, ty0, cover), (tx0, ty0 + S, cover)])
            out.append([(tx0 + S, ty0 + S, cover), (tx0, ty0 + S, cover), (tx0 + S, ty0, cover)])
            cover_flags += [True, True]
    return out, cover_flags


TINY = {"2e-38": 2e-38, "1e-39": 1e-39, "1e-41": 1e-41}


def sliver_depths(s):
    """Vertex depths s * (1.9, 1.9, 1) as float32: the maximum all along the long edge, where the covered centres are."""
    return tuple(np.float32(s) * np.float32(f) for f in (1.9, 1.9, 1.0))


def skip_bound(depths):
    """fl(max(d) * kSkipFactor): the early-out compares it with the tile's far depth."""
    return np.float32(max(depths)) * K["kSkipFactor"]


def early_out_scene(kind):
    """512x512, one case per 64x64 tile (.cases: tile index -> (cover depth or None, vertex depths)).
    normal:      constant sliver depth 0.3, cover 0 .. 20 float32 steps above it (the factor is about 10 steps there).
    tiny-<s>:    sliver depths s * (1.9, 1.9, 1), cover 1 .. 16 steps above fl(max * kSkipFactor).
    guard:       max depth on either side of kSkipMinDepth and of kSkipMaxDepth, cover 2 and 12 steps above the bound.
    no_cover:    the tiny slivers alone (nothing is ever skipped: the tile is never full).
    small:       the tiny cases at a size "main" draws in place."""
    cases = []
    if kind == "normal":
        z = np.float32(0.3)
        cases = [(step(z, n), (z, z, z)) for n in range(21)]
    elif kind.startswith("tiny-"):
        d = sliver_depths(TINY[kind[5:]])
        cases = [(step(skip_bound(d), n), d) for n in range(1, 17)]
    elif kind == "guard":
        lo, hi = K["kSkipMinDepth"], K["kSkipMaxDepth"]
        for m in (step(lo, -1), lo, step(lo, 1), step(hi, -2), step(hi, -1), hi):
            d = (np.float32(m), np.float32(m), np.float32(m * np.float32(0.5)))
            cases += [(step(skip_bound(d), n), d) for n in (2, 12)]
    elif kind in ("no_cover", "small"):
        for s in TINY.values():
            d = sliver_depths(s)
            cases += [(None if kind == "no_cover" else step(skip_bound(d), n), d) for n in (2, 4, 8)]
    else:
        raise KeyError(kind)
    t, flags = [], []
    for i, (cover, d) in enumerate(cases):
        tt, ff = _tile_content(64 * (i % 8), 64 * (i // 8), cover, d, small=kind == "small")
        t += tt; flags += ff
    t = np.array(t, np.float64)
    s = build((512, 512), t)
    s.cases, s.tris = cases, t
    s.is_cover = np.array(flags)
    return s


# ---- references ------------------------------------------------------------------------------------------------------
def reference(oracle, vr, s, threads=1, texels=True, positions=None):
    """(depth from orc_raster_depth, texels from tests/visibility_ref.c or None).  threads > 1: disjoint slices of the list
    into arrays of their own, from one thread each, max-merged -- exactly the references' semantics, because both
    results are maxima.  positions: the list positions to draw (default: all of them)."""
    import visibility_ref as VR
    from concurrent.futures import ThreadPoolExecutor
    W, H = s.render
    geo = VR.Geometry(s.sc, s.v, s.vid, s.tri)
    lst = np.ascontiguousarray(s.lst, np.uint32)
    positions = np.arange(len(lst), dtype=np.uint32) if positions is None else np.ascontiguousarray(positions, np.uint32)
    bounds = np.linspace(0, len(positions), threads + 1).astype(np.int64)

    def one(i):
        order = np.ascontiguousarray(positions[int(bounds[i]):int(bounds[i + 1])])   # list positions: the payload carries them
        depth = np.zeros((H, W), np.float32)
        oracle.raster_depth(s.k, s.sc, s.v, s.vid, s.tri, s.rec, lst[order], depth)
        vis = None
        if texels:
            vdepth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
            vr.vr_raster(s.k.ctypes.data, *geo.args(), s.rec.ctypes.data, lst.ctypes.data, len(order), order.ctypes.data, SLOT,
                         vdepth.ctypes.data, vis.ctypes.data)
        return depth, vis

    if threads == 1:
        return one(0)
    oracle.lib()
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(one, range(threads)))
    depth = parts[0][0]
    vis = parts[0][1]
    for d, t in parts[1:]:
        np.maximum(depth, d, out=depth)
        if texels:
            np.maximum(vis, t, out=vis)
    return depth, vis


# ---- the alpha-tested rasters: the same geometry with texture coordinates, materials and a table ---------------------------
# (tests/test_raster_path_scenes.py proves what these scenes claim, tests/test_gpu_alpha_raster_paths.py uses them.)
# An alpha scene is a built scene with m_TexCoord filled in, m_MaterialDataIdx per instance, .materials (MaterialData rows)
# and .textures: the table, a list of (mips, format), None (an empty entry) or OTHER_FORMAT; .textures = None: no table bound.
# The scenes have w = 1, so uv is affine in the pixel position: with uv = (offset from the apex) / 16 a pixel is half a texel
# of the 8 x 8 checker (cells of 4 x 4 pixels, lod 0); with uv = offset / 4 a pixel is two texels (one cell a pixel, lod 1,
# where the checker is still a checker).
OTHER_FORMAT = "a texture of a format the sampler does not take"
OWNER_UV, SLIVER_UV = 1.0 / 16.0, 1.0 / 4.0
SLIVER_LEGS = (520.0, 0.5 + 2.0 ** -9)               # box 521 x 2 = 1042 pixels > kSmallBox; the centres at +0.5 and +1.5 are covered


def _scenes():
    import alpha_test_scenes as A
    import material_texture_scenes as MS
    return A, MS


def set_alpha(s, uv, materials, textures, material_of_instance, exact=True):
    """Completes a built scene: uv [n_triangles, 3, 2] per vertex (exact halves unless exact=False)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    h = uv.astype(np.float16)
    assert len(h) == len(s.v) and (not exact or np.array_equal(h.astype(np.float64), uv)), "a texture coordinate is not a half"
    s.v["m_TexCoord"] = h.view(np.uint16)
    s.sc["instances"]["m_MaterialDataIdx"] = np.broadcast_to(np.asarray(material_of_instance, np.uint32), (len(s.sc["instances"]),))
    s.materials, s.textures = materials, textures
    return s


def apex_uv(tris, scale):
    """[n, 3, 2]: (pixel offset from the triangle's first vertex) * scale."""
    t = np.asarray(tris, np.float64)
    return (t[:, :, :2] - t[:, :1, :2]) * scale


# Where owner triangles lie a pixel apart (the round cases), an interior triangle owns its apex texel alone, and with uv = offset / 16
# every apex sample is kept: only the triangles on the block's rim would show their discard, and every triangle would carry the
# same AlphaTriangle, so that one drawn with another's would show nothing.  In these scenes the triangles of the even rows shift
# the checker by (7, 1.5) pixels: their apex sample (0.5, 0.5) then lies a quarter texel inside a cell below the cutoff (alpha
# 80 / 255) and the sample right of it (1.5, 0.5) a quarter texel inside the next cell (180 / 255).  A triangle of an even row
# loses its apex texel to its left neighbour, which keeps it (a witness: a forgotten discard hides that neighbour); a triangle
# of an odd row keeps and owns its apex.  Drawn with the texture coordinates of the other kind, either changes the image.
ROUND_PHASE = (7.0 / 16.0, 1.5 / 16.0)


def _row_phase(tris):
    """[n, 1, 2]: ROUND_PHASE for the triangles whose apex lies in an even pixel row, 0 for the others."""
    even = np.asarray(tris, np.float64)[:, 0, 1] % 2 == 0
    return np.where(even[:, None, None], np.asarray(ROUND_PHASE)[None, None], 0.0)


def textured(s, tris, scale=OWNER_UV, exact=True, phase=(0.0, 0.0)):
    """Every instance draws with the 8 x 8 checker under the wrap sampler (alpha_test_scenes.M_CHECKER, cutoff 0.5)."""
    A, _ = _scenes()
    return set_alpha(s, apex_uv(tris, scale) + np.asarray(phase), A.materials(), A.textures(), A.M_CHECKER, exact)


def sliver_tris(apex):
    """Owner slivers whose depth FALLS with X: z = 0.25 + (Y - X) * 2^-14.  Triangle (X, Y) covers the centres of the pixels
    (X, Y) and (X + 1, Y); under the checker at SLIVER_UV the first is kept and the second discarded.  Without the discard
    triangle X would win pixel X + 1 and hide triangle X + 1; with it every triangle owns its apex."""
    apex = np.asarray(apex, np.float64).reshape(-1, 2)
    return owner_tris(apex, SLIVER_LEGS, z=0.25 + (apex[:, 1] - apex[:, 0]) * 2.0 ** -14)


M_ABOVE, M_BELOW, M_BROKEN = 0, 1, 2                 # constant_alpha()'s cycle


def constant_alpha(s):
    """Instances cycle through a texture-free material above the cutoff, one below it and a broken chain (the albedo flag with
    a descriptor past the table).  .kept_positions: the list positions of the instances the convention keeps."""
    A, MS = _scenes()
    m = np.concatenate([MS.material(albedo=(0.2, 0.9, 0.2, 0.75)), MS.material(albedo=(0.9, 0.2, 0.2, 0.25)),
                        MS.material(flags=MS.ALBEDO, indices=(9, MS.NONE, MS.NONE, MS.NONE))])
    m["m_AlphaCutoff"] = A.CUTOFF
    n_inst = len(s.sc["instances"])
    set_alpha(s, np.zeros((len(s.v) // 3, 3, 2)), m, A.textures(), np.arange(n_inst) % 3)
    per = len(s.lst) // n_inst
    s.kept_positions = np.flatnonzero((np.arange(len(s.lst)) // per) % 3 == M_ABOVE).astype(np.uint32)
    return s


def small_box_alpha(kind):
    s = small_box_scene(kind)
    bw, bh = {"box1024": (32, 32), "box1025": (41, 25), "box33x32": (33, 32), "edge_clamped": (33, 32)}[kind]
    uv = np.zeros((s.n_triangles, 3, 2)); uv[:, 1, 0] = (bw - 1) * OWNER_UV; uv[:, 2, 1] = (bh - 1) * OWNER_UV
    A, _ = _scenes()
    return set_alpha(s, uv, A.materials(), A.textures(), A.M_CHECKER)


def tile_round_alpha(count):
    t = owner_tris(_pixels_of(64, 64, count))
    return textured(build((512, 512), t), t, phase=_row_phase(t))


def sparse_tile_alpha(matching=1000):
    a, b = _pixels_of(0, 0, matching), _pixels_of(128, 0, 2 * matching)
    apex = np.zeros((3 * matching, 2))
    apex[0::3], apex[1::3], apex[2::3] = a, b[0::2], b[1::2]                 # sparse_tile_scene()'s corners
    t = owner_tris(apex)
    return textured(build((512, 512), t), t, phase=_row_phase(t))


def _sliver_bin_tris(extra):
    side = 1 << K["kBinShift"]
    assert side * side == K["kBinCapacity"]
    t = sliver_tris(_pixels_of(0, 0, side * side, side))
    if extra:
        # one more entry of bin (0, 0): its box begins in the bin's last column, its covered centres are in the next bin;
        # nearer than everything there
        e = owner_tris([(side - 0.25, 10.0)], SLIVER_LEGS, z=np.array([0.25 + 2000 * 2.0 ** -14]))
        t = np.concatenate([t, e])
    return t


def sliver_bin_alpha(extra=False, per_meshlet=15):
    """1024 x 512 (wide and high enough that no box is clamped back to kSmallBox): one sliver per pixel of bin (0, 0)."""
    t = _sliver_bin_tris(extra)
    s = textured(build((1024, 512), t, per_meshlet=per_meshlet), t, SLIVER_UV)
    s.tris_px, s.cells = t, [(0, 0)]
    return s


def sliver_queue_alpha(per_meshlet=21):
    """4096 x 1024: the full bin of slivers under enough instances, a bin apart, to queue kQueueCapacity + 4096 triangles;
    no sliver reaches the last column or row."""
    W, H = 4096, 1024
    side = 1 << K["kBinShift"]
    need = -(-(K["kQueueCapacity"] + 4096) // K["kBinCapacity"])
    # every other bin column: the second sample of a row's last sliver is contested by no other instance, so its discard shows too
    cells = [(bx * side, by * side) for by in range(H // side - 1) for bx in range(0, (W - 521) // side, 2)]
    assert need <= len(cells)
    t = _sliver_bin_tris(False)
    s = textured(build((W, H), t, per_meshlet=per_meshlet, instances=cells[:need]), t, SLIVER_UV)
    s.tris_px, s.cells = t, cells[:need]
    return s


def queue_constant_alpha(per_meshlet=21):
    return constant_alpha(queue_scene(per_meshlet))


def stride_alpha(compute_units):
    s = stride_scene(compute_units)
    first = s.v["m_Position"].astype(np.float64).reshape(-1, 3, 3)
    W, H = s.render
    px = np.stack([(first[..., 0] + 1.0) * 0.5 * W, (1.0 - first[..., 1]) * 0.5 * H], 2)
    A, _ = _scenes()
    return set_alpha(s, (px - px[:, :1]) * OWNER_UV, A.materials(), A.textures(), A.M_CHECKER, exact=False)


def merge(a, b):
    """The scene that draws a's list and then b's: two meshes, b's instances, records and list positions after a's.  The
    predictions add up; .part: 0 / 1 per listed triangle."""
    assert a.render == b.render
    nv, nt, nm, ni, nr, nl = len(a.v), len(a.tri), len(a.sc["meshlets"]), len(a.sc["instances"]), len(a.rec), len(a.lst)
    mlb = b.sc["meshlets"].copy()
    mlb["m_MeshletVertexIDsBufferIdx"] += len(a.vid); mlb["m_MeshletIndexIDsBufferIdx"] += nt
    mdb = b.sc["meshData"].copy()
    mdb["m_MeshLODDatas"]["m_MeshletDataBufferIdx"][0][0] = nm
    ib = b.sc["instances"].copy(); ib["m_MeshDataIdx"] = 1
    rb = b.rec.copy(); rb["m_InstanceConstIdx"] += ni
    sc = dict(instances=np.concatenate([a.sc["instances"], ib]), meshData=np.concatenate([a.sc["meshData"], mdb]),
              meshlets=np.concatenate([a.sc["meshlets"], mlb]))
    shift = np.uint64(nl) << np.uint64(7)
    return SimpleNamespace(render=a.render, k=a.k, sc=sc, v=np.concatenate([a.v, b.v]), vid=np.concatenate([a.vid, b.vid + np.uint32(nv)]),
                           tri=np.concatenate([a.tri, b.tri]), rec=np.concatenate([a.rec, rb]),
                           lst=np.concatenate([a.lst, (b.lst + np.uint32(nr << 5)).astype(np.uint32)]),
                           payloads=np.concatenate([a.payloads, b.payloads + shift]), n_triangles=a.n_triangles + b.n_triangles,
                           live=np.concatenate([a.live, b.live]), box_pixels=np.concatenate([a.box_pixels, b.box_pixels]),
                           queued=np.concatenate([a.queued, b.queued]), queue_length=a.queue_length + b.queue_length,
                           bin_counts=a.bin_counts + b.bin_counts, tile_candidates=a.tile_candidates + b.tile_candidates, tiles=a.tiles,
                           part=np.concatenate([np.zeros(a.n_triangles, np.int64), np.ones(b.n_triangles, np.int64)]),
                           positions=(np.arange(nl, dtype=np.uint32), np.arange(nl, nl + len(b.lst), dtype=np.uint32)))


EARLY_OUT_COVERS = ("checker", "opaque", "below")


def early_out_alpha(cover, tiles=8, slivers=23, cover_instances=4):
    """512x512, one case per 64x64 tile as in early_out_scene("normal"): the cover 0, 2 .. 14 float32 steps above the first sliver's
    constant depth 0.3 (both sides of the factor, which is about 10 steps there).  The covers (8 quads a tile) are an instance of
    their own, listed first and drawn `cover_instances` times; the 23 slivers of a tile lie at 23 different places, are texture-free
    and kept, and sliver j lies j * 2^-10 behind the first: whatever order the queue has, a tile's farthest sliver mostly comes after
    32 nearer entries, and a far depth that took the covers' holes for covered would be nearer than it.
    cover: "checker" (uv = offset from the tile's corner / 16: a tile with holes has far depth 0), "opaque" (the same with every
    alpha byte 255) or "below" (constant alpha below the cutoff)."""
    A, MS = _scenes()
    z = np.float32(0.3)
    cases = [(step(z, 2 * i), (z, z, z)) for i in range(tiles)]
    t, flags = [], []
    for i, (cv, d) in enumerate(cases):
        tt, ff = _tile_content(64 * (i % 8), 64 * (i // 8), cv, d, n_slivers=slivers, n_quads=8)
        t += tt; flags += ff
    t, flags = np.array(t, np.float64), np.array(flags)
    c, sl = t[flags], t[~flags]
    sl[:, :, 2] -= (np.arange(len(sl)) % slivers)[:, None] * 2.0 ** -10
    s = merge(build((512, 512), c, instances=((0, 0),) * cover_instances), build((512, 512), sl))
    corner = np.floor(c[:, :, :2].min(1) / 64.0) * 64.0
    uv = np.concatenate([(c[:, :, :2] - corner[:, None]) * OWNER_UV, np.zeros((len(sl), 3, 2))])
    tex = A.textures() if cover != "opaque" else A.with_uniform_alpha(A.textures(), 255)
    set_alpha(s, uv, A.materials(), tex, [A.M_CONST_BELOW if cover == "below" else A.M_CHECKER] * cover_instances + [A.M_CONST_ABOVE])
    s.cases, s.n_tiles, s.slivers_per_tile, s.n_cover_triangles = cases, tiles, slivers, cover_instances * len(c)
    return s


# (g) rules 5 and 6: one instance per material; (name, kept)
RULE_CASES = [("checker", True), ("index past the buffer", False), ("descriptor past the table", False), ("empty entry", False),
              ("another format", False), ("NaN alpha", True), ("NaN alpha, textured", True), ("NaN cutoff", True),
              ("NaN cutoff, textured", True), ("cutoff +inf", False), ("cutoff +inf, textured", False), ("alpha == cutoff", True),
              ("cutoff the next float", False), ("texel == cutoff", True), ("texel below the next cutoff", False)]
RULE_TIE = np.float32(128) / np.float32(255)


def rules_alpha(path, table=True):
    """512 x 512: five owner triangles (legs 31 x 31 = a 1024-pixel box for path "main", 32 x 31 for "tiles"; one of them across
    a tile corner) under one instance per case of RULE_CASES, 80 and 100 pixels apart: no two instances share a pixel.
    table=False: no table is bound, and every material with the albedo flag draws nothing (.kept says which remain)."""
    A, MS = _scenes()
    legs = {"main": (31, 31), "tiles": (32, 31)}[path]
    t = owner_tris([(10, 10), (11, 10), (10, 11), (13, 12), (40, 50)], legs)
    cells = [(80 * (i % 6), 100 * (i // 6)) for i in range(len(RULE_CASES))]
    s = build((512, 512), t, instances=cells)
    nan, inf, nxt = np.float32(np.nan), np.float32(np.inf), np.nextafter(np.float32(0.5), np.float32(1))
    ck = dict(flags=MS.ALBEDO, indices=(A.CHECKER, MS.NONE, MS.NONE, MS.NONE))
    un = dict(flags=MS.ALBEDO, indices=(A.UNIFORM, MS.NONE, MS.NONE, MS.NONE))
    rows = [(MS.material(albedo=(1, 1, 1, 1.0), **ck), 0.5),
            (MS.material(flags=MS.ALBEDO, indices=(9, MS.NONE, MS.NONE, MS.NONE)), 0.5),
            (MS.material(flags=MS.ALBEDO, indices=(3, MS.NONE, MS.NONE, MS.NONE)), 0.5),
            (MS.material(flags=MS.ALBEDO, indices=(4, MS.NONE, MS.NONE, MS.NONE)), 0.5),
            (MS.material(albedo=(1, 1, 1, nan)), 0.5), (MS.material(albedo=(1, 1, 1, nan), **ck), 0.5),
            (MS.material(albedo=(1, 1, 1, 0.25)), nan), (MS.material(albedo=(1, 1, 1, 1.0), **ck), nan),
            (MS.material(albedo=(1, 1, 1, 1.0)), inf), (MS.material(albedo=(1, 1, 1, 1.0), **ck), inf),
            (MS.material(albedo=(1, 1, 1, 0.5)), 0.5), (MS.material(albedo=(1, 1, 1, 0.5)), nxt),
            (MS.material(albedo=(1, 1, 1, 1.0), **un), RULE_TIE), (MS.material(albedo=(1, 1, 1, 1.0), **un), np.nextafter(RULE_TIE, np.float32(1)))]
    mats = np.concatenate([m for m, _ in rows])
    mats["m_AlphaCutoff"] = np.array([c for _, c in rows], np.float32)
    index = [0, len(mats) + 5] + list(range(1, len(mats)))           # case 1 names a row past the buffer
    tex = A.textures(uniform=128) + [None, OTHER_FORMAT]              # descriptors 3 (empty) and 4 (another format) of a table of 5
    set_alpha(s, apex_uv(t, OWNER_UV), mats, tex if table else None, index)
    flagged = [bool(mats["m_MaterialFlags"][i] & MS.ALBEDO) if i < len(mats) else False for i in index]
    s.kept = [k and (table or not f) for (_, k), f in zip(RULE_CASES, flagged)]
    return s


def ref_textures(textures):
    """The table as tests/alpha_test_ref.py takes it: OTHER_FORMAT becomes an entry whose format is neither RGBA8 nor sRGBA8."""
    import material_textures_ref as MT
    if textures is None:
        return None
    return [MT.Texture([np.zeros((4, 4, 4), np.uint8)], 1) if t is OTHER_FORMAT else t for t in textures]


def alpha_reference(at, s, threads=1, alpha_test=True, positions=None):
    """(depth, texels, counts) of tests/alpha_test_ref.c's at_raster: disjoint slices of the list (or of `positions`) into arrays
    of their own, from one thread each, max-merged, the four counts summed."""
    import alpha_test_ref as AT
    import visibility_ref as VR
    from concurrent.futures import ThreadPoolExecutor
    W, H = s.render
    geo = VR.Geometry(s.sc, s.v, s.vid, s.tri)
    tex = ref_textures(s.textures)
    positions = np.arange(len(s.lst), dtype=np.uint32) if positions is None else np.ascontiguousarray(positions, np.uint32)
    bounds = np.linspace(0, len(positions), threads + 1).astype(np.int64)

    def one(i):
        depth, vis = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint64)
        counts = AT.raster(at, s.k, geo, s.rec, s.lst, SLOT, depth, vis, s.materials, tex, alpha_test, order=positions[int(bounds[i]):int(bounds[i + 1])])
        return depth, vis, counts

    if threads == 1:
        return one(0)
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(one, range(threads)))
    depth, vis, counts = parts[0]
    for d, t, c in parts[1:]:
        np.maximum(depth, d, out=depth); np.maximum(vis, t, out=vis)
        counts = counts + c
    return depth, vis, counts


# name -> (maker(compute_units), the launch whose counts the reference must show, flavour, reference threads): the owner scenes
# of tests/test_gpu_alpha_raster_paths.py, whose preconditions tests/test_raster_path_scenes.py proves
ALPHA_OWNER_SCENES = dict(
    [(f"a-{kind}", (lambda cu, kind=kind: small_box_alpha(kind), "main" if kind in ("box1024", "edge_clamped") else "tiles", "textured", 1))
     for kind in ("box1024", "box1025", "box33x32", "edge_clamped")]
    + [(f"b-{n}", (lambda cu, n=n: tile_round_alpha(n), "tiles", "textured", 16))
       for n in (K["kTileList"] - K["kBlock"], K["kTileList"], K["kTileList"] + 1, 2 * K["kTileList"] + 1)]
    + [("b-sparse", (lambda cu: sparse_tile_alpha(), "tiles", "textured", 16)),
       ("c-full", (lambda cu: sliver_bin_alpha(False), "tiles", "sliver", 16)), ("c-over", (lambda cu: sliver_bin_alpha(True), "tiles", "sliver", 16)),
       ("d-slivers", (lambda cu: sliver_queue_alpha(), "tiles", "sliver", 16)),
       ("e-stride", (lambda cu: stride_alpha(cu), "tiles", "textured", 4))])


def triangle_of(s, payloads):
    """The index into s.payloads (instance-major, then triangle) of each payload."""
    order = np.argsort(s.payloads)
    return order[np.searchsorted(s.payloads[order], payloads)]
