"""The visibility path at the list sizes where its kernels switch algorithm, grid or tiling.

Every case sits on one side of one switch -- the last length before it or the first after it, or just past a tile or chunk
edge -- builds a scene whose list length is exactly that number, runs a frame through the C ABI and compares every output
word with the CPU oracle (tests/test_gpu_parity.py::compare_frame: records, masks, visible lists, dispatch and draw
arguments; late count and HZB).  Each case also asserts the path it took: from the "<shader>#<op>" names of the device
profile where the paths are separate launches.  Where they are one launch that branches on the device (binned order and its
guard, short pass, texel vs table kernel) the branch is not observed: the case is put on its side by construction, from the
rule the back end applies (restated below with its constants), and asserts the oracle's words like every other case.

The thresholds are read from the kernel sources, so the cases follow the code; the CPU-only test at the end fails when a
pattern stops matching.  Scenes use one group (at most 32 meshlets) per instance, so that with frustum and occlusion
culling off (flags 4: cone only) the group count of a pass is exactly its instance count."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from suite_support import compare_frame, dev, oracle_hzb, upload_hzb  # noqa: E402, F401
from toyrenderer_amd import synth  # noqa: E402


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyrenderer_amd", "csrc")

# (file, pattern) -> the value of group 1 (an integer, or an exponent where the pattern says "1u << ")
_PATTERNS = {
    "kFusedMaxEntries": ("k_gpuculling.hip", r"constexpr uint32_t kFusedMaxEntries = 1u << (\d+);"),
    "kFusedLateMaxTiles": ("k_gpuculling.hip", r"constexpr uint32_t kFusedLateMaxTiles = (\d+);"),
    "kInstanceBlock": ("k_gpuculling.hip", r"constexpr uint32_t kBlock = (\d+);"),
    "TR_MIN_BINNED": ("k_gpuculling.hip", r"#define TR_MIN_BINNED (\d+)"),
    "TR_BIG_THREADS": ("k_gpuculling.hip", r"#define TR_BIG_THREADS (\d+)"),
    "TR_BIG_PER": ("k_gpuculling.hip", r"#define TR_BIG_PER (\d+)"),
    "kCompactTile": ("k_basepass_as.hip", r"constexpr uint32_t kCompactTile = (\d+);"),
    "kCompactMaxTiles": ("k_basepass_as.hip", r"constexpr uint32_t kCompactMaxTiles = \(1u << (\d+)\) / kCompactTile;"),
    "sideListBuild": ("k_basepass_as.hip", r"emitListBuild\(ctx, a, \"\", a\.recordCapacity >= \(1u << (\d+)\), "),
    "TR_SUPER_SHIFT": ("k_basepass_as.hip", r"#define TR_SUPER_SHIFT (\d+)"),
    "kBatch": ("k_basepass_as.hip", r"constexpr uint32_t kBatch = (\d+);"),
    "TR_SHORT_PASS_ROUNDS": ("k_basepass_as.hip", r"#define TR_SHORT_PASS_ROUNDS (\d+)"),
    "TR_CULL_WAVES": ("k_basepass_as.hip", r"#define TR_CULL_WAVES (\d+)"),
    "TR_CULL_WAVES_PER_EU": ("k_basepass_as.hip", r"#define TR_CULL_WAVES_PER_EU (\d+)"),
    "TR_RING_SLOTS": ("k_basepass_as.hip", r"#define TR_RING_SLOTS (\d+)"),
    "kPackThreads": ("k_basepass_as.hip", r"constexpr uint32_t kPackThreads = (\d+);"),
    "kPackRounds": ("k_basepass_as.hip", r"constexpr uint32_t kPackRounds = (\d+);"),
    "tableMinGroups": ("trhip_internal.h", r"getenv\(\"TRHIP_TABLE_MIN_GROUPS\"\); return e \? \(uint32_t\)strtoul\(e, nullptr, 0\) : \(1u << (\d+)\); \}"),
}
_SHIFTS = {"kFusedMaxEntries", "kCompactMaxTiles", "sideListBuild", "tableMinGroups"}   # (kCompactMaxTiles: 2^19 / kCompactTile)

# The rules the cases restate (host side: which launches are recorded; device side: the branch of one launch).
_RULES = [
    ("k_gpuculling.hip", r"const bool fusedPath = \(nMax <= kFusedMaxEntries \|\| \(LATE && \(nMax \+ kBlock - 1\) / kBlock <= kFusedLateMaxTiles\)\) && !noFused;"),
    ("k_gpuculling.hip", r"const bool binned = n >= kMinBinnedEntries;"),
    ("k_gpuculling.hip", r"a\.permHeader\[0\] = \(n >= kMinBinnedEntries && baseX == 0 && X < a\.maxGroups && X <= a\.permCapacity\) \? 1u : 0u;"),
    ("k_gpuculling.hip", r"constexpr uint32_t kBigChunk = kBigThreads \* kBigPerThread;"),
    ("k_basepass_as.hip", r"if \(!side && a\.recordCapacity <= kCompactMaxTiles \* kCompactTile\) \{"),
    ("k_basepass_as.hip", r"const uint32_t supers = \(a\.maxBatches >> kSuperShift\) \+ 1u;"),
    ("k_basepass_as.hip", r"if \(!TABLE && G <= gridDim\.x \* \(2u \* kCullWaves\) \* a\.shortPassRounds\) \{"),
    ("k_basepass_as.hip", r"uint32_t grid = ctx\.computeUnits\(\) \* blocksPerCU;\s+const uint32_t needBlocks = \(a\.recordCapacity \+ kCullBatch \* kCullWaves - 1\) / \(kCullBatch \* kCullWaves\);"),
    ("k_basepass_as.hip", r"#define TR_CULL_BATCH \(TR_RING_SLOTS == 3 \? 30 : 32\)"),
    ("k_basepass_as.hip", r"const bool useTable = occlusion && ctx\.variant == 0 && records->byteSize / sizeof\(MeshletAmplificationData\) >= trhip::tableMinGroups\(\);"),
    ("k_basepass_as.hip", r"constexpr uint32_t kPackTile = kPackThreads \* kPackRounds;"),
]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _thresholds():
    src, out = {}, {}
    for key, (fname, pat) in _PATTERNS.items():
        text = src.setdefault(fname, _read(fname))
        m = re.search(pat, text)
        assert m, f"{fname}: {key} no longer matches {pat!r}"
        v = int(m.group(1))
        out[key] = (1 << v) if key in _SHIFTS else v
    out["kCompactMaxTiles"] //= out["kCompactTile"]
    out["kBigChunk"] = out["TR_BIG_THREADS"] * out["TR_BIG_PER"]
    out["kCullBatch"] = 30 if out["TR_RING_SLOTS"] == 3 else 32
    out["kPackTile"] = out["kPackThreads"] * out["kPackRounds"]
    out["compactMax"] = out["kCompactMaxTiles"] * out["kCompactTile"]
    return out


T = _thresholds()
FUSED_MAX = T["kFusedMaxEntries"]                         # 2^17 list entries
LATE_FUSED_MAX = T["kFusedLateMaxTiles"] * T["kInstanceBlock"]   # 2^20: the late pass stays fused up to 4096 tiles of 256
MIN_BINNED = T["TR_MIN_BINNED"]                           # 4096
CHUNK = T["kBigChunk"]                                    # 512
SIDE = T["sideListBuild"]                                 # 2^19: list build on the side stream = count / scan / expand
SUPER = 1 << T["TR_SUPER_SHIFT"]                          # 256 batches of kBatch groups
TABLE_MIN = T["tableMinGroups"]                           # 2^17 records of capacity

# parameters of the cases the TRHIP_NO_FUSED_INSTANCE=1 child process reruns (rows 2 and 3)
BINNED_NS = [MIN_BINNED - 1, MIN_BINNED, MIN_BINNED + 1]
BINNED_CAPS = [16384, TABLE_MIN]
GUARD_CAP_MINUS_X = [1, 0, -1]
CHUNK_NS = [k * CHUNK + d for k in (3, 9) for d in (-1, 0, 1)]
CONTINUE_CASES = 1                                        # test_binned_order_guard_when_the_counters_continue

INST = ("gpuculling_CS_GPUCulling LATE_CULL=0", "gpuculling_CS_GPUCulling LATE_CULL=1")
AS = ("basepass_AS_Main LATE_CULL=0", "basepass_AS_Main LATE_CULL=1")
NO_FUSED = os.environ.get("TRHIP_NO_FUSED_INSTANCE") is not None


def _ops(prof, shader):
    return {name.split("#", 1)[1] for name in prof if "#" in name and name.split("#", 1)[0] == shader}


def _assert_instance_path(prof, late, three_kernel):
    ops = _ops(prof, INST[late])
    if three_kernel:
        assert {"classify", "scan", "emit"} <= ops and "fused" not in ops, (late, sorted(ops))
    else:
        assert "fused" in ops and not ({"classify", "scan", "emit"} & ops), (late, sorted(ops))


def _assert_list_path(prof, late, compact):
    ops = _ops(prof, AS[late])
    assert "cull" in ops, (late, sorted(ops))
    if compact:
        assert "compact" in ops and not ({"count", "scan", "expand"} & ops), (late, sorted(ops))
    else:
        assert {"count", "scan", "expand"} <= ops and "compact" not in ops, (late, sorted(ops))


def _instance_three_kernel(n, late=False):
    """recordGPUCulling's fusedPath, negated (n = m_NbInstances: the list's length, also for the late pass)."""
    if NO_FUSED:
        return True
    return not (n <= FUSED_MAX or (late and -(-n // T["kInstanceBlock"]) <= T["kFusedLateMaxTiles"]))


def _spec(n, *, meshlets=32, seed=1, **kw):
    return synth.SceneSpec(num_meshes=16, num_instances=n, meshlets_lod0=meshlets, max_lods=1, seed=seed, **kw)


VIEW = synth.make_view(eye=(0.3, 0.1, 0.5), yaw=0.02, prev_eye=(0.0, 0.0, 0.0), prev_yaw=0.0, render=(640, 360))
D_PREV = synth.gen_depth(VIEW, num_occluders=60, seed=11, scale=3.0)
D_CUR = synth.gen_depth(VIEW, num_occluders=40, seed=12, scale=3.0)


def _frame(dev, oracle, spec, cap, flags, *, depth_prev=None, depth_cur=None, view=VIEW):
    """One frame of `spec` at record capacity `cap`, compared word for word with the oracle.  Returns (got, ref, profile)."""
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    scene = synth.make_scene(spec)
    gs = GpuScene(dev, scene.instances, scene.meshData, scene.meshlets, scene.opaqueIds, scene.alphaMaskIds)
    drv = FrameDriver(dev, gs, view, record_capacity=cap, culling_flags=flags)
    hzb = oracle_hzb(oracle, view, depth_prev)
    try:
        if depth_prev is not None:
            upload_hzb(drv, hzb)
        if depth_cur is not None:
            drv.depth.upload_mip(0, depth_cur)
        dev.profile_reset()
        dev.profile_enable(True)
        try:
            drv.record()
            drv.run()
            got = drv.results()
            prof = dev.profile()
        finally:
            dev.profile_enable(False)
        hzb_got = drv.hzb.download_chain() if flags & 2 and depth_cur is not None else None
    finally:
        drv.release()
        gs.release()
    ref = oracle.frame(scene.as_oracle(), view.as_dict(), hzb, depth_cur, cullingFlags=flags, maxGroups=cap, record_capacity=cap)
    compare_frame(got, ref)
    if flags & 2:
        assert got["lateCount"] == int(ref.lateCount[0])
    if hzb_got is not None:
        assert np.array_equal(hzb_got, hzb.texels), "HZB chain differs"
    return got, ref, prof


# ---- 1. instance pass: one fused launch vs classify / scan / emit -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [FUSED_MAX, FUSED_MAX + 1])
def test_early_instance_pass_at_the_fused_limit(dev, oracle, n):
    """kFusedMaxEntries (2^17 list entries), early pass: n = 2^17 is the last length of the fused launch (its 512-tile
    maximum), 2^17 + 1 the first of classify / scan / emit (no override; 256 chunks of 512 + 1 entry).  Frustum, occlusion
    and cone culling with both phases; capacity 2^18 (footprint-table kernel, one-launch list build)."""
    got, ref, prof = _frame(dev, oracle, _spec(n, seed=n), 1 << 18, 7, depth_prev=D_PREV, depth_cur=D_CUR)
    _assert_instance_path(prof, 0, three_kernel=_instance_three_kernel(n))
    assert NO_FUSED or _instance_three_kernel(n) == (n > FUSED_MAX)
    assert ref.lateCount[0] > 0 and ref.dispatchArgs[0][0] > 0 and ref.dispatchArgs[1][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [LATE_FUSED_MAX, LATE_FUSED_MAX + 1])
def test_late_instance_pass_at_the_fused_tile_limit(dev, oracle, n):
    """kFusedLateMaxTiles (4096 tiles of 256 = 2^20 instances), late pass: the late pass stays fused up to m_NbInstances = 2^20
    and takes classify / scan / emit from 2^20 + 1.  Every instance is deferred (HZB near everywhere, depth far): the late list
    holds all of them (Q1: ceil(n / 64) * 32 are re-tested).  The early pass is three-kernel on both sides (scan: its
    register-resident rows up to 2048 workgroups = 2^20 entries, the looped form from 2^20 + 1); both list builds run
    count / scan / expand (capacity 2^20)."""
    near = np.ones((VIEW.renderH, VIEW.renderW), np.float32)
    far = np.zeros((VIEW.renderH, VIEW.renderW), np.float32)
    spec = _spec(n, meshlets=4, seed=5, z_near=20.0, z_far=60.0, box_x=4.0, box_y=3.0)
    got, ref, prof = _frame(dev, oracle, spec, 1 << 20, 2, depth_prev=near, depth_cur=far)
    assert ref.lateCount[0] == n, "all instances must be deferred to the late pass"
    assert ref.dispatchArgs[1][0] == -(-n // 64) * 32
    _assert_instance_path(prof, 0, three_kernel=True)
    _assert_instance_path(prof, 1, three_kernel=_instance_three_kernel(n, late=True))
    assert NO_FUSED or _instance_three_kernel(n, late=True) == (n > LATE_FUSED_MAX)
    _assert_list_path(prof, 1, compact=False)


# ---- 2. + 3. the three-kernel pass: binned processing order, classify chunks ------------------------------------------
# These run on the fused path in the plain suite and through classify / scan / emit in
# test_three_kernel_pass_at_its_binning_and_chunk_edges (TRHIP_NO_FUSED_INSTANCE=1): both paths must give the oracle's words.
@pytest.mark.gpu
@pytest.mark.parametrize("cap", BINNED_CAPS)
@pytest.mark.parametrize("n", BINNED_NS)
def test_binned_order_at_its_entry_threshold(dev, oracle, n, cap):
    """TR_MIN_BINNED (4096 list entries): n = 4095 keeps the canonical processing order, 4096 and 4097 are the first lengths
    of the tile-binned order (three-kernel path only), which the early meshlet cull then consumes (usePerm: every group
    emitted, the pass started from 0, X < capacity).  Both phases with occlusion; capacity 16384 (texel kernel, G above
    its short-pass limit: the short pass never reads the order) and 2^17 (footprint-table kernel)."""
    got, ref, prof = _frame(dev, oracle, _spec(n, seed=7, meshlets=40, box_x=10.0, box_y=6.0, z_near=30.0, z_far=150.0), cap, 7,
                            depth_prev=D_PREV, depth_cur=D_CUR)
    _assert_instance_path(prof, 0, three_kernel=_instance_three_kernel(n))
    X = int(ref.dispatchArgs[0][0])
    assert 0 < X < cap and ref.validRecords[0] == X
    assert cap >= TABLE_MIN or X > _short_pass_limit(dev, cap), "the meshlet cull must walk the list in batches"


@pytest.mark.gpu
@pytest.mark.parametrize("cap_minus_x", GUARD_CAP_MINUS_X)
def test_binned_order_guard_at_the_group_capacity(dev, oracle, cap_minus_x):
    """permHeader[0] (k_gpuculling.hip instanceScanKernel) at TR_MIN_BINNED entries: X = 4096 groups (cone culling only, one
    group per instance) against a capacity of X + 1 (the order is published: X < capacity, nothing dropped), X (the last
    instance is dropped, Q2: canonical order) and X - 1 (dropped: canonical order).  The meshlet cull reads the published
    order (k_basepass_as.hip usePerm) and falls back to list order otherwise.  The header itself is back-end private memory
    and is not read back: which outcome the GPU took is not observed here, only that the words equal the oracle's on each side
    (a guard that never published would pass; one that published a dropped pass's order fails on the masks)."""
    n = MIN_BINNED
    cap = n + cap_minus_x
    got, ref, prof = _frame(dev, oracle, _spec(n, seed=8), cap, 4)
    _assert_instance_path(prof, 0, three_kernel=_instance_three_kernel(n))
    X = int(ref.dispatchArgs[0][0])
    assert X == n and X > _short_pass_limit(dev, cap), "the meshlet cull must walk the list in batches"
    assert (ref.validRecords[0] == X) == (cap_minus_x == 1), "published iff nothing is dropped"


@pytest.mark.gpu
def test_binned_order_guard_when_the_counters_continue(dev, oracle):
    """permHeader[0]'s baseX == 0 term at >= TR_MIN_BINNED entries: two early instance passes (the opaque list, then the
    alpha-mask list, each >= 4096 entries) into the SAME records and counters with no clear in between, then the meshlet cull
    over all of them.  The second pass starts from X1 != 0: its binned order covers only its own records [X1, X2), so it must
    not be published -- the meshlet cull would then walk [0, X2) through a list that holds X2 - X1 valid entries.  Cone
    culling only (every instance submits one group); capacity 16384: the texel kernel walks the list in batches."""
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    from toyrenderer_amd.rhi import CB, SRV, UAV, SAMPLER
    spec = _spec(2 * MIN_BINNED + 1500, seed=13, alpha_mask_fraction=0.5)
    scene = synth.make_scene(spec)
    lists = [scene.opaqueIds, scene.alphaMaskIds]
    assert all(len(ids) >= MIN_BINNED for ids in lists), [len(ids) for ids in lists]
    cap, flags = 16384, 4
    gs = GpuScene(dev, scene.instances, scene.meshData, scene.meshlets, scene.opaqueIds, scene.alphaMaskIds)
    drv = FrameDriver(dev, gs, VIEW, record_capacity=cap, culling_flags=flags)
    try:
        # oracle: the two instance passes continuing one counter, then the meshlet cull of all records
        recs = np.zeros(cap, oracle.RECORD_DT)
        o_args, o_late, o_ids = np.zeros(3, np.uint32), np.zeros(1, np.uint32), np.zeros(len(scene.instances), np.uint32)
        xs = []
        for ids in lists:
            valid = oracle.instance_cull(drv._cull_consts(len(ids)), False, scene.instances, ids, scene.meshData, None,
                                         recs, o_args, o_late, o_ids, 0, cap)
            xs.append(int(o_args[0]))
        X1, X2 = xs
        assert X1 == len(lists[0]) and X2 == len(scene.instances) and valid == X2 < cap
        assert X2 > _short_pass_limit(dev, cap), "the meshlet cull must walk the list in batches"
        o_mask, o_list, _ = oracle.meshlet_cull(drv._basepass_consts(False), scene.instances, scene.meshData, scene.meshlets,
                                                recs, 0, X2, None)
        assert 0 < len(o_list) < 32 * X2
        # GPU: the same sequence in one command list
        cl = drv.cl
        cl.open()
        cl.clear_buffer_u32(drv.dispatchArgs[0], 0)
        for ids_buf, nb in ((gs.opaqueIds, len(lists[0])), (gs.alphaMaskIds, len(lists[1]))):
            cb = cl.constant_buffer(drv._cull_consts(nb), "GPUCullingPassConstants")
            b = [CB(0, cb), SRV(0, gs.instances), SRV(1, ids_buf), SRV(2, gs.meshData), UAV(0, drv.records[0]),
                 UAV(1, drv.dispatchArgs[0]), UAV(2, drv.dummy), UAV(3, drv.dummy), SAMPLER(0)]
            cl.dispatch("gpuculling_CS_GPUCulling LATE_CULL=0", b, ((nb + 31) // 32, 1, 1))
        drv._render_instances(cl, 0, False, False)
        cl.close()
        dev.profile_reset()
        dev.profile_enable(True)
        try:
            dev.execute(cl)
            dev.wait_idle()
            prof = dev.profile()
        finally:
            dev.profile_enable(False)
        _assert_instance_path(prof, 0, three_kernel=_instance_three_kernel(len(lists[0])))
        args = drv.dispatchArgs[0].download(np.uint32, 4)
        assert list(args[:3]) == [X2, 1, 1] and int(args[3]) == X2, args
        assert np.array_equal(drv.records[0].download(oracle.RECORD_DT, X2).view(np.uint32), recs[:X2].view(np.uint32))
        assert np.array_equal(drv.visMask[0].download(np.uint32, X2), o_mask[:X2]), "visibility masks differ"
        draw = drv.drawArgs[0].download(np.uint32, 3)
        assert list(draw) == [len(o_list), 1, 1], draw
        assert np.array_equal(drv.visibleList[0].download(np.uint32, len(o_list)), o_list), "visible lists differ"
    finally:
        drv.release()
        gs.release()


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHUNK_NS)
def test_classify_chunks_at_their_edges(dev, oracle, n):
    """kBigChunk (TR_BIG_THREADS x TR_BIG_PER = 512 entries per classify / emit workgroup): k * 512 - 1 (last workgroup one
    short), k * 512 (all full) and k * 512 + 1 (a workgroup of one entry) for k = 3 (canonical order) and k = 9 (binned).
    Three-kernel under TRHIP_NO_FUSED_INSTANCE=1, fused (tiles of 256) otherwise.  Cone culling only: X = n exactly.
    Capacity 8192: the texel kernel walks the list in batches (above its short-pass limit), reading the binned order."""
    cap = 8192
    got, ref, prof = _frame(dev, oracle, _spec(n, seed=9), cap, 4)
    _assert_instance_path(prof, 0, three_kernel=_instance_three_kernel(n))
    assert int(ref.dispatchArgs[0][0]) == n and 0 < int(ref.drawArgs[0][0]) < 32 * n
    assert n > _short_pass_limit(dev, cap)


@pytest.mark.gpu
def test_three_kernel_pass_at_its_binning_and_chunk_edges():
    """The cases of rows 2 and 3 through classify / scan / emit (TRHIP_NO_FUSED_INSTANCE=1), in one child process."""
    env = dict(os.environ, TRHIP_NO_FUSED_INSTANCE="1")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_size_boundaries.py"), "-q", "-x", "-m", "gpu",
                        "-k", "binned_order or classify_chunks"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    expect = len(BINNED_NS) * len(BINNED_CAPS) + len(GUARD_CAP_MINUS_X) + len(CHUNK_NS) + CONTINUE_CASES
    assert re.search(rf"\b{expect} passed\b", p.stdout), p.stdout[-2000:]


# ---- 4. + 5. meshlet list build: one-launch compaction vs count / super scan / expand ---------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cap", [SIDE - 1, SIDE])
def test_list_build_at_the_compaction_capacity(dev, oracle, cap):
    """The list build's switch is the record CAPACITY: below 2^19 (recordASMain: side = capacity >= 2^19) one visCompactKernel
    launch of kCompactTile tiles, from 2^19 on count / super scan / expand on the side stream.  (kCompactMaxTiles *
    kCompactTile = 2^19 would still fit the compaction; only the unpack path of the exchange takes it at exactly 2^19.)
    The same scene on both sides, early and late phase."""
    spec = synth.SceneSpec(num_meshes=24, num_instances=3000, meshlets_lod0=70, jitter_meshlets=True, max_lods=3, seed=4)
    got, ref, prof = _frame(dev, oracle, spec, cap, 7, depth_prev=D_PREV, depth_cur=D_CUR)
    assert T["compactMax"] == SIDE
    for late in (0, 1):
        _assert_list_path(prof, late, compact=cap < SIDE)
    assert ref.drawArgs[0][0] > 0 and ref.drawArgs[1][0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [65535, SIDE])
@pytest.mark.parametrize("groups", [T["kCompactTile"] - 1, T["kCompactTile"], T["kCompactTile"] + 1, 2 * T["kCompactTile"]])
def test_list_build_at_tile_edges(dev, oracle, groups, cap):
    """kCompactTile (2048 groups per compaction tile): 2047 (one partial tile), 2048 (one full tile), 2049 (a tile of one group)
    and 4096 (the last tile full) on the one-launch compaction (capacity 65535) and on count / scan / expand (capacity 2^19,
    the same batches of 64 and supers of 256 batches).  Cone culling only: exactly `groups` groups."""
    got, ref, prof = _frame(dev, oracle, _spec(groups, seed=groups), cap, 4)
    assert int(ref.dispatchArgs[0][0]) == groups and ref.validRecords[0] == groups
    _assert_list_path(prof, 0, compact=cap < SIDE)


@pytest.mark.gpu
@pytest.mark.parametrize("cap,n", [(SIDE - 1, SIDE - 2), (SIDE - 1, SIDE - 1), (SIDE, SIDE - 1),
                                   (SIDE - T["kCompactTile"] + 1, SIDE - T["kCompactTile"])])
def test_list_build_with_the_capacity_filled(dev, oracle, cap, n):
    """Groups filling the record capacity (kCompactMaxTiles tiles): n = capacity - 1 groups is the most a pass keeps (Q2: an
    instance is dropped when offset + groups >= capacity); n = capacity drops the last instance.  Capacity 2^19 - 1 (the
    last capacity of the compaction, 256 tiles, the last one short by one group) and 2^19 (the first of count / scan /
    expand); 2^19 - 2047 with 255 full tiles.  The instance pass is three-kernel and binned here."""
    got, ref, prof = _frame(dev, oracle, _spec(n, seed=3, meshlets=20), cap, 4)
    X = int(ref.dispatchArgs[0][0])
    assert X == n and int(ref.validRecords[0]) == min(n, cap - 1)
    _assert_instance_path(prof, 0, three_kernel=_instance_three_kernel(n))
    _assert_list_path(prof, 0, compact=cap < SIDE)


@pytest.mark.gpu
@pytest.mark.parametrize("batches", [32 * SUPER, 33 * SUPER - 1, 65 * SUPER - 1])
def test_super_scan_at_a_whole_number_of_supers(dev, oracle, batches):
    """TR_SUPER_SHIFT (supers of 256 batches of 64 groups; supers = (maxBatches >> TR_SUPER_SHIFT) + 1 workgroups and words of
    super sums): maxBatches = 32 * 256 (capacity 2^19, a whole number of supers) and 33 * 256 - 1 (the last super one batch
    short), with the capacity filled (capacity - 1 groups: every super holds groups).  count / scan / expand only.
    65 * 256 - 1: (maxBatches >> 8) = 64 super-sum words fill their 256-byte scratch allocation exactly, so the + 1 is the
    word the last, partial super is written to.  (Without the + 1 that word lands just past the allocation but inside the
    scratch arena, which nothing later in these frames reuses: outputs do not change.  The grid of the count launch strides
    over all supers whatever its size.  So this case does not catch a missing + 1; it covers the 65-super list build.)"""
    cap = batches * T["kBatch"]
    assert cap >= SIDE
    got, ref, prof = _frame(dev, oracle, _spec(cap - 1, seed=6, meshlets=24), cap, 4)
    assert int(ref.validRecords[0]) == cap - 1
    _assert_list_path(prof, 0, compact=False)


# ---- 6. texel kernel: short pass vs batches ---------------------------------------------------------------------------
def _short_pass_limit(dev, cap):
    """meshletCullKernel's short pass: G <= grid * 2 * TR_CULL_WAVES * TR_SHORT_PASS_ROUNDS, grid = min(CUs * TR_CULL_WAVES_PER_EU,
    ceil(capacity / (kCullBatch * TR_CULL_WAVES)))."""
    per_block = T["kCullBatch"] * T["TR_CULL_WAVES"]
    grid = min(dev.compute_units * T["TR_CULL_WAVES_PER_EU"], -(-cap // per_block))
    return grid * 2 * T["TR_CULL_WAVES"] * T["TR_SHORT_PASS_ROUNDS"]


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1])
def test_texel_kernel_short_pass_limit(dev, oracle, side):
    """TR_SHORT_PASS_ROUNDS x grid x 2 TR_CULL_WAVES half-waves (8192 groups at capacity 65535 on 256 CUs): G at the limit is the
    last pass one half-wave per record evaluates; limit + 1 the first that takes the batch machinery.  The branch is on the
    device (one launch, op name `cull` on both sides) and is not observed: the side is fixed by construction, from the limit
    computed from the device's CU count and the constants read from the sources.  Both sides assert the same thing -- the
    oracle's words.  Cone culling only, so G = n."""
    cap = 65535
    limit = _short_pass_limit(dev, cap)
    n = limit + side
    assert n < cap - 1
    got, ref, prof = _frame(dev, oracle, _spec(n, seed=10), cap, 4)
    assert int(ref.validRecords[0]) == n and 0 < int(ref.drawArgs[0][0]) < 32 * n
    _assert_list_path(prof, 0, compact=True)


# ---- 7. texel vs footprint-table meshlet kernel -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cap", [TABLE_MIN - 1, TABLE_MIN])
def test_texel_and_table_kernels_at_the_table_capacity(dev, oracle, cap):
    """tableMinGroups() (2^17 records of capacity): the early meshlet cull with occlusion takes the texel kernel at 2^17 - 1 and
    the footprint-table kernel (its table rebuilt by extra workgroups of the instance pass) at 2^17.  One launch either way,
    op name `cull` on both sides, so the kernel taken is not observed: the side is fixed by construction, from the capacity
    and the rule restated from the sources.  Both sides assert the same thing -- the oracle's words.  The same scene, both
    phases, all culling on."""
    spec = synth.SceneSpec(num_meshes=24, num_instances=3000, meshlets_lod0=70, jitter_meshlets=True, max_lods=3, seed=12)
    got, ref, prof = _frame(dev, oracle, spec, cap, 7, depth_prev=D_PREV, depth_cur=D_CUR)
    assert ref.lateCount[0] > 0 and 0 < ref.drawArgs[0][0] < ref.meshletsTested[0]
    _assert_instance_path(prof, 0, three_kernel=_instance_three_kernel(3000))
    _assert_list_path(prof, 0, compact=True)


def test_threshold_patterns_still_match_the_sources():
    """CPU only: every threshold and rule this file restates is still where it reads it from, with the values the cases were
    built around (a change of value is fine for the cases; this says which ones to look at)."""
    for fname, pat in _RULES:
        assert re.search(pat, _read(fname)), f"{fname}: rule no longer matches {pat!r}"
    t = _thresholds()
    assert t["kFusedMaxEntries"] == t["kFusedMaxEntries"] // t["kInstanceBlock"] * t["kInstanceBlock"]
    assert t["kCompactMaxTiles"] * t["kCompactTile"] == t["sideListBuild"], "compaction limit and side-stream threshold diverged"
    assert t["kFusedLateMaxTiles"] * t["kInstanceBlock"] > t["kFusedMaxEntries"]
    assert t["TR_MIN_BINNED"] < t["kFusedMaxEntries"] and t["TR_MIN_BINNED"] % t["kBigChunk"] == 0
