"""Every HZB build path (csrc/k_hzb.hip) and the footprint-min table derived from the HZB (csrc/hzb_quad.hip.h), through the
C ABI, bit for bit against the plain numpy reference tests/hzb_ref.py (tied to the oracle by tests/test_hzb_ref.py).

Chain: min (FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1, m_bDownsampleMax = 0) and max (FILTER=2, m_bDownsampleMax = 1) through every
launch sequence recordSPD can emit -- `depth_tile` (+ `tail`), `main` + `tile` (+ `tail`), `main` + `mip`... + `tail`,
`main` + `tail` -- each case asserting the sequence it took by the profile's op names and launch counts; shapes inside and
outside the reference's HZB rule (hzb = next_pow2(render) >> 1) so that every clamp of hzbDepthTileKernel fires; values over
the whole fp32 range (tests/hzb_ref.py hostile_depth).  Every texel of every mip is compared; a NaN compares as "is NaN" (HLSL
leaves its payload open).  -0.0 and signalling NaNs are left out: minNum does not order the zeros and the IEEE mode of the
wave decides what a signalling NaN becomes; neither the HLSL nor the oracle defines them.

Table: read back with the test-only probe (tests/hip/hzb_table_probe.hip in lib/libtrhip_probe.so), every defined entry of
every mip compared with hzb_ref.table() after each of its builders, and after every kind of HZB write (staleness).

Left out, on purpose: trhip_texture_bind_memory as a staleness case -- rhi.Device.create_texture has no virtual textures
and rhi.py no heap binding, so the path is not reachable from the Python ABI binding.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from suite_support import dev  # noqa: E402, F401
from toyrenderer_amd import interop as I  # noqa: E402
from toyrenderer_amd import synth  # noqa: E402

from . import hzb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(ROOT, "toyrenderer_amd", "lib", "libtrhip_probe.so")

MINMAX = "minmaxdownsample_CS_Main"
SPD = ("ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=1", "ffx_spd_downsample_pass_CS FFX_SPD_OPTION_DOWNSAMPLE_FILTER=2")
LATE_ARGS = "gpuculling_CS_BuildLateCullIndirectArgs"
INST0 = "gpuculling_CS_GPUCulling LATE_CULL=0"
AS0 = "basepass_AS_Main LATE_CULL=0"
NO_FUSED = os.environ.get("TRHIP_NO_FUSED_INSTANCE") is not None
TABLE_CAP = 1 << 19                                                     # record capacity of a table-using frame (smoke() uses the same)


def _ops(prof, shader):
    """{op name: launches} of one shader name."""
    return {name.split("#", 1)[1]: cnt for name, (cnt, _ms) in prof.items() if "#" in name and name.split("#", 1)[0] == shader}


# ---- chain ---------------------------------------------------------------------------------------------------------------------
def record_minmax(cl, depth, hzb, maximum, mip=0):
    """BasePassRenderers.cpp:515-536 with either filter, into any mip of the HZB."""
    from toyrenderer_amd.rhi import PUSH, SAMPLER, TEX_SRV, TEX_UAV
    mw, mh = hzb.mip_dims(mip)
    k = np.zeros(1, I.MinMaxDownsampleConsts)
    k["m_OutputDimensions"] = (mw, mh)
    k["m_bDownsampleMax"] = 1 if maximum else 0
    cl.dispatch(MINMAX, [PUSH(0), TEX_SRV(0, depth), TEX_UAV(0, hzb, mip), SAMPLER(0)], ((mw + 7) // 8, (mh + 7) // 8, 1), push=k)


def record_spd(cl, depth, hzb, atomic, maximum):
    """FFXHelpers.cpp:36-115 with either filter."""
    from toyrenderer_amd.rhi import PUSH, TEX_SRV, TEX_UAV, UAV
    cl.clear_buffer_u32(atomic, 0)
    spd = np.zeros(8, np.uint32)
    spd[0] = hzb.mips - 1
    spd[1] = ((hzb.w + 63) // 64) * ((hzb.hgt + 63) // 64)
    b = [PUSH(0), TEX_SRV(0, depth), UAV(0, atomic), TEX_UAV(1, hzb, min(6, hzb.mips - 1)), TEX_UAV(2, hzb, 0)]
    b += [TEX_UAV(3 + i, hzb, i + 1) for i in range(hzb.mips - 1)]
    cl.dispatch(SPD[int(maximum)], b, ((hzb.w + 63) // 64, (hzb.hgt + 63) // 64, 1), push=spd)


class _Chain:
    """A depth image and an HZB of any two sizes, and the two dispatches of GenerateHZB recorded the way a case asks for."""

    def __init__(self, dev, depth_dims, hzb_dims):
        from toyrenderer_amd import rhi
        self.dev = dev
        self.W, self.H = depth_dims
        self.w, self.h = hzb_dims
        self.mips = R.num_mips(self.w, self.h)
        self.hzb = dev.create_texture(self.w, self.h, self.mips, rhi.FORMAT_R16_FLOAT, "HZB")
        self.depth = dev.create_texture(self.W, self.H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
        self.atomic = dev.create_buffer(24, "SPD Global Atomic Buffer", stride=24)
        self.count = dev.buffer_from(np.zeros(1, np.uint32), "count")
        self.args = dev.create_buffer(12, "args", stride=12, indirect=True)
        self.lists = [dev.create_command_list(), dev.create_command_list()]

    def fill(self, word=0x3555):
        """Every mip to a recognisable word, so that a texel no launch wrote is seen."""
        for k in range(self.mips):
            mw, mh = R.mip_dims(self.w, self.h, k)
            self.hzb.upload_mip(k, np.full((mh, mw), word, np.uint16))

    def minmax(self, cl, maximum, mip=0):
        record_minmax(cl, self.depth, self.hzb, maximum, mip)

    def spd(self, cl, maximum):
        record_spd(cl, self.depth, self.hzb, self.atomic, maximum)

    def other_dispatch(self, cl):
        from toyrenderer_amd.rhi import SRV, UAV
        cl.dispatch(LATE_ARGS, [SRV(0, self.count), UAV(0, self.args)], (1, 1, 1))

    def run(self, record):
        """record(list0, list1) records into the two open lists; both are executed in order.  Returns (chain words, profile)."""
        dev = self.dev
        for cl in self.lists:
            cl.open()
        record(*self.lists)
        for cl in self.lists:
            cl.close()
        dev.profile_reset()
        dev.profile_enable(True)
        try:
            dev.execute(*self.lists)
            dev.wait_idle()
            prof = dev.profile()
        finally:
            dev.profile_enable(False)
        return self.hzb.download_chain(), prof

    def build(self, maximum, form="frame"):
        """GenerateHZB: minmaxdownsample, the clear of SPD's counter, SPD.
        frame: as in a frame's list, where a clear launch exists earlier in the recording -- the counter's clear joins it
        (trhip_internal.h: clear hoisting), the two dispatches are consecutive commands and the peephole may fuse them;
        clear_between: the same three calls in an otherwise empty list -- the clear is a launch of its own between the two;
        two_lists: SPD in a list of its own; dispatch_between: another dispatch between the two."""
        def record(a, b):
            if form != "clear_between":
                a.clear_buffer_u32(self.count, 0)
            self.minmax(a, maximum)
            if form == "dispatch_between":
                self.other_dispatch(a)
            self.spd(b if form == "two_lists" else a, maximum)
        return self.run(record)

    def release(self):
        for cl in self.lists:
            cl.release()
        for r in (self.hzb, self.depth, self.atomic, self.count, self.args):
            r.release()


def _spd_ops(w, h, fused):
    """The launch sequence recordSPD documents for an HZB: tiled (both dimensions multiples of 64) -> one `depth_tile` (fused
    with minmaxdownsample) or `tile` launch for mips 1..6; then one `mip` launch per mip while the last mip built is larger than
    64 x 64 texels; then `tail` if mips remain."""
    mips = R.num_mips(w, h)
    ops, first = {}, 0
    if w % 64 == 0 and h % 64 == 0 and mips > 1:
        ops["depth_tile" if fused else "tile"] = 1
        first = min(mips - 1, 6)
    while np.prod(R.mip_dims(w, h, first)) > 64 * 64 and first + 1 < mips:
        ops["mip"] = ops.get("mip", 0) + 1
        first += 1
    if first + 1 < mips:
        ops["tail"] = 1
    return ops


def _assert_chain(got, depth, w, h, maximum, what):
    ref = R.pack(R.build(depth, w, h, maximum))
    same = R.same_words(got, ref)
    bad = np.nonzero(~same)[0]
    assert len(bad) == 0, (what, len(bad), [(int(i), hex(int(got[i])), hex(int(ref[i]))) for i in bad[:8]])


PATHS = {   # name: (depth dims, HZB dims, form, minmaxdownsample ops, SPD ops)
    "depth_tile+tail": ((256, 256), (128, 128), "frame", {}, {"depth_tile": 1, "tail": 1}),
    "depth_tile": ((127, 100), (64, 64), "frame", {}, {"depth_tile": 1}),
    "main+tile+tail/two_lists": ((256, 256), (128, 128), "two_lists", {"main": 1}, {"tile": 1, "tail": 1}),
    "main+tile+tail/dispatch_between": ((256, 256), (128, 128), "dispatch_between", {"main": 1}, {"tile": 1, "tail": 1}),
    "main+tile/two_lists": ((127, 100), (64, 64), "two_lists", {"main": 1}, {"tile": 1}),
    "main+tile+tail/clear_between": ((256, 256), (128, 128), "clear_between", {"main": 1}, {"tile": 1, "tail": 1}),
    "main+mip+mip+tail": ((2048, 64), (1024, 32), "frame", {"main": 1}, {"mip": 2, "tail": 1}),
    "main+mip+tail/two_lists": ((48, 600), (32, 512), "two_lists", {"main": 1}, {"mip": 1, "tail": 1}),
    "main+tail": ((100, 40), (64, 32), "frame", {"main": 1}, {"tail": 1}),
}


@pytest.mark.parametrize("maximum", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_chain_paths_and_filters(dev, path, maximum):
    """Each launch sequence of GenerateHZB for FILTER=1 / m_bDownsampleMax = 0 and FILTER=2 / m_bDownsampleMax = 1; `tile`
    is reached by keeping the peephole from fusing: SPD in its own command list, another dispatch in between, or the clear of
    SPD's counter as a launch of its own in between (what a list that holds nothing but GenerateHZB records)."""
    depth_dims, (w, h), form, mm_ops, spd_ops = PATHS[path]
    assert spd_ops == _spd_ops(w, h, fused=(form == "frame"))
    c = _Chain(dev, depth_dims, (w, h))
    try:
        depth = R.hostile_depth(*depth_dims, seed=len(path) + 100 * maximum)
        c.depth.upload_mip(0, depth)
        c.fill()
        got, prof = c.build(maximum, form)
        assert _ops(prof, MINMAX) == mm_ops and _ops(prof, SPD[int(maximum)]) == spd_ops and _ops(prof, SPD[1 - int(maximum)]) == {}, prof
        assert (_ops(prof, LATE_ARGS) == {"main": 1}) == (form == "dispatch_between")
        _assert_chain(got, depth, w, h, maximum, path)
        assert not np.array_equal(got, R.pack(R.build(depth, w, h, not maximum))), "min and max agree: the image cannot tell them apart"
    finally:
        c.release()


def _clamps(out_dim, src_dim):
    """Which edge clamps the gather of one axis really performs: 'lo' (an index below 0) / 'hi' (an index above src_dim - 1)."""
    raw = R.gather_index_fp32(out_dim, src_dim)
    return ({"lo"} if (raw < 0).any() else set()) | ({"hi"} if (raw + 1 > src_dim - 1).any() else set())


BOTH, HI, NONE = {"lo", "hi"}, {"hi"}, set()
SHAPES = [  # (depth dims, HZB dims, clamps in x, clamps in y).  The reference's rule first (hzb = next_pow2(render) >> 1: the ratio lies in
    # (1, 2] and no index is ever clamped) ...
    ((64, 64), (32, 32), NONE, NONE), ((65, 65), (64, 64), NONE, NONE), ((127, 127), (64, 64), NONE, NONE), ((128, 128), (64, 64), NONE, NONE),
    ((129, 129), (128, 128), NONE, NONE), ((65, 128), (64, 64), NONE, NONE), ((129, 64), (128, 32), NONE, NONE), ((127, 65), (64, 64), NONE, NONE),
    ((129, 65), (128, 64), NONE, NONE), ((65, 129), (64, 128), NONE, NONE),           # the smallest tiled chains: mip 6 is 1x1, 2x1, 1x2
    # the fp32 index differs from the exact one: in the last column (row) it is 4096 instead of 4095, so its upper neighbour IS clamped
    ((4097, 70), (4096, 64), HI, NONE), ((70, 4097), (64, 4096), NONE, HI),
    # ... then pairs outside it (the C ABI takes any pair), all on a tiled HZB through the fused launch.  A ratio below 1 clamps on
    # both sides; equal sizes clamp the upper index only (the index is x itself: this is the case where x0 = W - 1 and the 8-byte
    # load has to step back, `xl = min(x0, W - 2)`); ratios of 2 and above never clamp (kept: the strides change); a dimension of
    # 2 or 1 clamps nearly everywhere, and width 1 is the only way into the `wide == false` path.
    ((40, 23), (64, 64), BOTH, BOTH), ((100, 100), (128, 128), BOTH, BOTH), ((128, 64), (128, 64), HI, HI), ((256, 128), (128, 64), NONE, NONE),
    ((1000, 600), (64, 64), NONE, NONE), ((2, 50), (64, 64), BOTH, BOTH), ((1, 37), (64, 64), BOTH, BOTH), ((300, 1), (128, 64), NONE, BOTH),
    ((1, 1), (64, 128), BOTH, BOTH),
]


@pytest.mark.parametrize("depth_dims,hzb_dims,cx,cy", SHAPES, ids=[f"{d[0]}x{d[1]}-to-{z[0]}x{z[1]}" for d, z, _, _ in SHAPES])
def test_chain_shapes_and_clamps(dev, depth_dims, hzb_dims, cx, cy):
    """Min and max on each shape, recorded as the reference records GenerateHZB.  The clamps a case is listed for are checked
    on the reference's own index set first, so that a case cannot quietly stop exercising them."""
    (W, H), (w, h) = depth_dims, hzb_dims
    assert _clamps(w, W) == cx and _clamps(h, H) == cy, (_clamps(w, W), _clamps(h, H))
    c = _Chain(dev, depth_dims, hzb_dims)
    try:
        depth = R.hostile_depth(W, H, seed=W * 31 + H)
        c.depth.upload_mip(0, depth)
        tiled = w % 64 == 0 and h % 64 == 0
        for maximum in (False, True):
            c.fill()
            got, prof = c.build(maximum)
            assert _ops(prof, MINMAX) == ({} if tiled else {"main": 1}) and _ops(prof, SPD[int(maximum)]) == _spd_ops(w, h, fused=True), prof
            _assert_chain(got, depth, w, h, maximum, (depth_dims, hzb_dims, maximum))
    finally:
        c.release()


def test_clamp_cases_cover_every_clamp_on_the_fused_tiled_path():
    """Not a GPU case by itself: the list above, taken together, reaches lo and hi clamps in both axes on tiled HZBs, a depth
    narrower than 2 texels, and a width at which the fp32 index is not the exact one."""
    tiled = [(d, z, cx, cy) for d, z, cx, cy in SHAPES if z[0] % 64 == 0 and z[1] % 64 == 0]
    assert any(cx == BOTH and cy == BOTH for _, _, cx, cy in tiled) and any(d[0] == 1 for d, _, _, _ in tiled) and any(d[0] == 2 for d, _, _, _ in tiled)
    assert any(d[1] == 1 for d, _, _, _ in tiled)
    assert (R.gather_index_fp32(4096, 4097) != R.gather_index_exact(4096, 4097)).any()


def test_chain_8k_class_odd_render(dev):
    """7681 x 4321 -> 4096 x 4096 (133 MB of depth, 45 MB of HZB: comfortable on this device), min and max."""
    (W, H), (w, h) = (7681, 4321), I.hzb_dims(7681, 4321)
    assert (w, h) == (4096, 4096) and (R.gather_index_fp32(w, W) != R.gather_index_exact(w, W)).any()
    c = _Chain(dev, (W, H), (w, h))
    try:
        depth = R.hostile_depth(W, H, seed=8)
        c.depth.upload_mip(0, depth)
        for maximum in (False, True):
            got, prof = c.build(maximum)
            assert _ops(prof, MINMAX) == {} and _ops(prof, SPD[int(maximum)]) == {"depth_tile": 1, "tail": 1} == _spd_ops(w, h, True), prof
            _assert_chain(got, depth, w, h, maximum, maximum)
    finally:
        c.release()


def _halves_image(w, h, seed):
    """uint16 [h, w]: every finite half and +-inf at least once where the image has room for them (63 489 words: -0.0 left
    out, see the module docstring), else a sample; no two horizontal or vertical neighbours equal."""
    rng = np.random.default_rng(seed)
    halves = R.all_halves()
    n = w * h
    idx = np.concatenate([rng.permutation(len(halves)), rng.integers(0, len(halves), max(n - len(halves), 0))])[:n]
    img = halves[rng.permutation(idx)].reshape(h, w)
    for _ in range(64):
        eq = np.zeros((h, w), bool)
        eq[:, 1:] |= img[:, 1:] == img[:, :-1]
        eq[1:, :] |= img[1:, :] == img[:-1, :]
        if not eq.any():
            break
        if n >= len(halves):                                            # swap with random places: the multiset stays complete
            ys, xs = np.nonzero(eq)
            for y, x in zip(ys, xs):
                y2, x2 = int(rng.integers(0, h)), int(rng.integers(0, w))
                img[y, x], img[y2, x2] = img[y2, x2], img[y, x]
        else:
            img[eq] = halves[rng.integers(0, len(halves), int(eq.sum()))]
    assert not (img[:, 1:] == img[:, :-1]).any() and not (img[1:, :] == img[:-1, :]).any()
    return img


@pytest.mark.parametrize("maximum", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("hzb_dims,spd_ops", [((256, 256), {"tile": 1, "tail": 1}), ((1024, 32), {"mip": 2, "tail": 1}), ((64, 32), {"tail": 1}),
                                              ((64, 64), {"tile": 1})])
def test_spd_alone_on_an_uploaded_mip0(dev, hzb_dims, spd_ops, maximum):
    """An SPD dispatch with no minmaxdownsample in front of it (the `tile` op in its plainest form).  256 x 256 holds all
    63 488 finite halves (but -0.0) and +-inf."""
    w, h = hzb_dims
    c = _Chain(dev, (8, 8), hzb_dims)
    try:
        m0 = _halves_image(w, h, seed=w + h)
        if w * h >= 63489:
            assert len(np.unique(m0)) == 63489
        c.fill()
        c.hzb.upload_mip(0, m0)
        got, prof = c.run(lambda a, b: c.spd(a, maximum))
        assert _ops(prof, MINMAX) == {} and _ops(prof, SPD[int(maximum)]) == spd_ops == _spd_ops(w, h, False), prof
        ref = R.pack(R.chain(m0.view(np.float16), w, h, maximum))
        assert np.array_equal(got, ref), int((got != ref).sum())
    finally:
        c.release()


@pytest.mark.parametrize("maximum", [False, True], ids=["min", "max"])
def test_minmaxdownsample_into_mip1_then_spd(dev, maximum):
    """recordMinMaxDownsample accepts any mip of the HZB as its target: mip 1 gets the downsampled depth, the other mips stay.
    An SPD right behind it must NOT fuse (the note is about mip 1, not mip 0): it runs `tile` on the uploaded mip 0."""
    (W, H), (w, h) = (90, 50), (128, 64)
    c = _Chain(dev, (W, H), (w, h))
    try:
        depth = R.hostile_depth(W, H, seed=77)
        c.depth.upload_mip(0, depth)
        m0 = _halves_image(w, h, seed=5)
        c.fill()
        c.hzb.upload_mip(0, m0)
        got, prof = c.run(lambda a, b: c.minmax(a, maximum, mip=1))
        assert _ops(prof, MINMAX) == {"main": 1} and _ops(prof, SPD[0]) == {} and _ops(prof, SPD[1]) == {}
        mips = R.unpack(got, w, h)
        assert R.same_words(mips[1].view(np.uint16), R.mip0(depth, 64, 32, maximum).view(np.uint16)).all()
        assert np.array_equal(mips[0].view(np.uint16), m0) and all((m.view(np.uint16) == 0x3555).all() for m in mips[2:])

        def record(a, b):
            c.minmax(a, maximum, mip=1)
            c.spd(a, maximum)
        got, prof = c.run(record)
        assert _ops(prof, MINMAX) == {"main": 1} and _ops(prof, SPD[int(maximum)]) == {"tile": 1, "tail": 1}, prof
        assert np.array_equal(got, R.pack(R.chain(m0.view(np.float16), w, h, maximum)))
    finally:
        c.release()


def test_minmaxdownsample_rejects_dimensions_that_are_not_the_target_mips(dev):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import PUSH, SAMPLER, TEX_SRV, TEX_UAV
    c = _Chain(dev, (90, 50), (128, 64))
    try:
        k = np.zeros(1, I.MinMaxDownsampleConsts)
        k["m_OutputDimensions"] = (128, 64)                               # mip 0's, bound to mip 1
        cl = c.lists[0]
        cl.open()
        with pytest.raises(rhi.TrhipError, match="m_OutputDimensions"):
            cl.dispatch(MINMAX, [PUSH(0), TEX_SRV(0, c.depth), TEX_UAV(0, c.hzb, 1), SAMPLER(0)], (16, 8, 1), push=k)
        cl.close()
    finally:
        c.release()


# ---- footprint-min table -----------------------------------------------------------------------------------------------------
class HzbTableInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mips", C.c_uint32), ("format", C.c_uint32), ("quadTotal", C.c_uint32),
                ("hasTable", C.c_uint32), ("quadOffset", C.c_uint32 * 16), ("tableBytes", C.c_uint64), ("builtVersion", C.c_uint64),
                ("version", C.c_uint64)]


TABLE_OK, TABLE_NONE = 0, 3
_probe = None


def probe():
    global _probe
    if _probe is None:
        assert os.path.exists(PROBE_PATH), f"{PROBE_PATH} is missing: `make -C toyrenderer_amd/csrc` builds it beside libtrhip.so"
        lib = C.CDLL(PROBE_PATH)
        lib.hzb_table_info_size.restype = C.c_uint32
        lib.hzb_table_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(HzbTableInfo), C.c_void_p, C.c_uint64]
        assert lib.hzb_table_info_size() == C.sizeof(HzbTableInfo)
        _probe = lib
    return _probe


def _probe_call(tex, info, out):
    from toyrenderer_amd import rhi
    L = rhi.load()
    return probe().hzb_table_probe(tex.h, C.cast(L.trhip_texture_mip_info, C.c_void_p), tex.format, int(L.trhip_texture_size(tex.h)), C.byref(info),
                                   out.ctypes.data if out is not None else None, len(out) if out is not None else 0)


def read_table(dev, tex, want_words=True):
    """(info, words or None) of a texture's footprint-min table.  Synchronises first: side stream joined, device idle."""
    from toyrenderer_amd import rhi
    L = rhi.load()
    assert L.trhip_device_join_side_stream(dev.h) == 0
    dev.wait_idle()
    info = HzbTableInfo()
    rc = _probe_call(tex, info, None)
    assert rc == TABLE_OK, rc
    assert (info.width, info.height, info.mips, info.format) == (tex.w, tex.hgt, tex.mips, tex.format)
    if not want_words:
        return info, None
    words = np.zeros(max(info.quadTotal, 1), np.uint16)
    rc = _probe_call(tex, info, words)
    assert rc == TABLE_OK, rc
    return info, words[:info.quadTotal]


def _assert_table(info, words, chain_words, w, h, what=""):
    """Layout (quadOffset[], quadTotal) against hzb_ref.table_layout, every defined entry against hzb_ref.table()."""
    offs, total = R.table_layout(w, h)
    assert info.hasTable and info.quadTotal == total and list(info.quadOffset[:len(offs)]) == offs and info.tableBytes >= 2 * total, what
    ref, defined = R.table_packed(R.unpack(chain_words, w, h), w, h)
    bad = np.nonzero((words != ref) & defined)[0]
    assert len(bad) == 0, (what, len(bad), [(int(i), hex(int(words[i])), hex(int(ref[i]))) for i in bad[:8]])


class _TableFrame:
    """A small scene and a FrameDriver whose frames use the footprint-min table (record capacity 2^19, occlusion on) and never
    write the HZB themselves (freeze: GenerateHZB is skipped), so the table a frame leaves is the table of what the test put
    into the HZB."""

    def __init__(self, dev, render):
        from toyrenderer_amd.frame import FrameDriver, GpuScene
        self.dev = dev
        self.view = synth.make_view(eye=(0.3, 0.1, 0.5), yaw=0.02, prev_eye=(0.0, 0.0, 0.0), prev_yaw=0.0, render=render)
        scene = synth.make_scene(synth.SceneSpec(num_meshes=24, num_instances=300, meshlets_lod0=70, jitter_meshlets=True, max_lods=5,
                                                 alpha_mask_fraction=0.15, seed=1234))
        self.gs = GpuScene(dev, scene.instances, scene.meshData, scene.meshlets, scene.opaqueIds, scene.alphaMaskIds)
        self.drv = FrameDriver(dev, self.gs, self.view, record_capacity=TABLE_CAP, culling_flags=7, freeze_culling_camera=True)
        self.w, self.h = self.drv.hzb_w, self.drv.hzb_h
        self.hzb = self.drv.hzb

    def upload(self, seed):
        mips = []
        for k in range(self.hzb.mips):
            mw, mh = R.mip_dims(self.w, self.h, k)
            mips.append(_halves_image(mw, mh, seed=seed * 100 + k))
            self.hzb.upload_mip(k, mips[-1])
        return np.concatenate([m.ravel() for m in mips])

    def frame(self):
        """One frame; returns its profile."""
        dev = self.dev
        dev.profile_reset()
        dev.profile_enable(True)
        try:
            self.drv.record()
            self.drv.run()
            dev.wait_idle()
            return dev.profile()
        finally:
            dev.profile_enable(False)

    def release(self):
        self.drv.release()
        self.gs.release()


def _assert_instance_builder(prof):
    ops = set(_ops(prof, INST0))
    if NO_FUSED:
        assert {"classify", "scan", "emit"} <= ops and "fused" not in ops, sorted(ops)
    else:
        assert "fused" in ops and not ({"classify", "scan", "emit"} & ops), sorted(ops)
    assert "cull" in _ops(prof, AS0)


# render -> HZB: 2048x1024, 256x128, 512x512 (blocksPerRow = 32k + 1: a one-block last strip), 128x128, 64x32, 32x2048, 1024x32,
# 4096x64, and 1x1 (render 2x2: the smallest the frame path allows, hzb_dims of anything smaller is 0)
TABLE_RENDERS = [(4096, 2048), (512, 256), (1024, 1024), (256, 256), (128, 64), (64, 4096), (2048, 64), (8192, 128), (2, 2)]
TABLE_HZBS = [(2048, 1024), (256, 128), (512, 512), (128, 128), (64, 32), (32, 2048), (1024, 32), (4096, 64), (1, 1)]


@pytest.mark.parametrize("render,hzb_dims", list(zip(TABLE_RENDERS, TABLE_HZBS)), ids=[f"{w}x{h}" for w, h in TABLE_HZBS])
def test_table_equals_reference_after_the_instance_pass_built_it(dev, render, hzb_dims):
    """The table the early instance pass leaves (extra workgroups of `fused`; of `scan` + `emit` under TRHIP_NO_FUSED_INSTANCE, see
    test_table_through_scan_and_emit) equals table(download_chain()), entry for entry, and lies where the layout formula says."""
    t = _TableFrame(dev, render)
    try:
        assert (t.w, t.h) == hzb_dims
        info, _ = read_table(dev, t.hzb, want_words=False)
        assert not info.hasTable and info.builtVersion == 0
        assert _probe_call(t.hzb, HzbTableInfo(), np.zeros(4, np.uint16)) == TABLE_NONE        # no table yet: an error, not a fault
        up = t.upload(seed=hzb_dims[0] + hzb_dims[1])
        prof = t.frame()
        _assert_instance_builder(prof)
        chain_words = t.hzb.download_chain()
        assert np.array_equal(chain_words, up), "the frame wrote the HZB"
        info, words = read_table(dev, t.hzb)
        assert info.builtVersion == info.version
        _assert_table(info, words, chain_words, t.w, t.h, hzb_dims)
    finally:
        t.release()


@pytest.mark.parametrize("percent", ["0", "37", "100"])
def test_table_through_scan_and_emit(percent):
    """The same cases with the table's strips built by extra workgroups of the three-kernel pass's scan and emit launches, split
    0 / 37 / 100 % (the environment is read once per process: a child process, one at a time)."""
    env = dict(os.environ, TRHIP_NO_FUSED_INSTANCE="1", TRHIP_QUAD_SCAN_PERCENT=percent)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_hzb.py"), "-q", "-x", "-m", "gpu",
                        "-k", "test_table_equals_reference_after_the_instance_pass_built_it"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and f"{len(TABLE_HZBS)} passed" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _cull_only(t):
    """A command list with the early meshlet cull of slot 0 alone -- no instance pass in front of it: a stale table is rebuilt by
    the stand-alone hzbQuadBuildKernel the cull command launches first.  Records and arguments are those of the last frame."""
    dev, drv = t.dev, t.drv
    cl = dev.create_command_list()
    cl.open()
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
    cl.release()
    return prof


@pytest.mark.parametrize("render,hzb_dims", [((4096, 2048), (2048, 1024)), ((512, 256), (256, 128)), ((64, 4096), (32, 2048)), ((128, 64), (64, 32)),
                                             ((2, 2), (1, 1))], ids=["2048x1024", "256x128", "32x2048", "64x32", "1x1"])
def test_table_equals_reference_after_the_stand_alone_build(dev, render, hzb_dims):
    t = _TableFrame(dev, render)
    try:
        t.upload(seed=1)
        t.frame()
        before, old = read_table(dev, t.hzb)
        up = t.upload(seed=2)                                            # the table is stale now
        prof = _cull_only(t)
        assert _ops(prof, INST0) == {} and "cull" in _ops(prof, AS0), prof
        info, words = read_table(dev, t.hzb)
        assert info.builtVersion == info.version > before.builtVersion
        _assert_table(info, words, up, t.w, t.h, hzb_dims)
        assert not np.array_equal(words, old)
    finally:
        t.release()


def test_table_is_rebuilt_after_every_kind_of_hzb_write_and_only_then(dev):
    """One scene, one 256 x 128 HZB.  After each kind of write the next table-using frame leaves the table of the NEW contents;
    a write the back end cannot see leaves it as it was until trhip_texture_mark_written; a frame that wrote nothing to the
    HZB does not rebuild (built.version does not move)."""
    from toyrenderer_amd import rhi
    t = _TableFrame(dev, (512, 256))
    w, h, hzb = t.w, t.h, t.hzb
    other = dev.create_texture(w, h, hzb.mips, rhi.FORMAT_R16_FLOAT, "other HZB")
    seen = []

    def frame_and_check(what, expect_rebuild=True):
        before, _ = read_table(dev, hzb, want_words=False)
        t.frame()
        chain_words = hzb.download_chain()
        info, words = read_table(dev, hzb)
        if expect_rebuild:
            assert info.version > before.builtVersion and info.builtVersion == info.version, what
            _assert_table(info, words, chain_words, w, h, what)
            assert not any(np.array_equal(words, s) for s in seen), f"{what}: the table did not change, the case proves nothing"
            seen.append(words)
        return info, words, chain_words

    try:
        t.upload(seed=3)
        info0, words0, _ = frame_and_check("first upload")
        # a frame that writes nothing to the HZB: no rebuild
        info1, words1, _ = frame_and_check("idle frame", expect_rebuild=False)
        assert info1.builtVersion == info0.builtVersion and info1.version == info0.version and np.array_equal(words1, words0)

        # 1. a dispatch with the texture as UAV: SPD rebuilds mips 1.. from the (random) mip 0
        cl = dev.create_command_list()
        cl.open(); record_spd(cl, t.drv.depth, hzb, t.drv.spdAtomic, False); cl.close()
        dev.execute(cl); dev.wait_idle()
        frame_and_check("SPD rebuild")
        # 2. clear_texture_f32
        cl.open(); cl.clear_texture_f32(hzb, 0.3); cl.close()
        dev.execute(cl); dev.wait_idle()
        _, words, chain_words = frame_and_check("clear_texture_f32")
        assert (chain_words == np.float16(0.3).view(np.uint16)).all()
        # 3. copy_texture into it
        for k in range(other.mips):
            other.upload_mip(k, _halves_image(*R.mip_dims(w, h, k), seed=900 + k))
        cl.open(); cl.copy_texture(hzb, other); cl.close()
        dev.execute(cl); dev.wait_idle()
        _, _, chain_words = frame_and_check("copy_texture")
        assert np.array_equal(chain_words, other.download_chain())
        # 4. trhip_texture_upload of one mip
        hzb.upload_mip(2, _halves_image(*R.mip_dims(w, h, 2), seed=4))
        frame_and_check("upload_mip")
        cl.release()
        # 5. a write through the raw pointer (trhip_texture_device_ptr): invisible to the back end ...
        L = rhi.load()
        raw = dev.wrap_buffer(int(L.trhip_texture_device_ptr(hzb.h)), w * h * 2, "HZB mip 0 through its raw pointer", stride=2)
        raw.upload(_halves_image(w, h, seed=5))
        info_a, words_a, chain_a = frame_and_check("out of band, unmarked", expect_rebuild=False)
        assert np.array_equal(words_a, seen[-1]) and info_a.builtVersion == info_a.version, "the documented contract: an unmarked write is not seen"
        ref, defined = R.table_packed(R.unpack(chain_a, w, h), w, h)
        assert ((words_a != ref) & defined).any(), "the stale table equals the new one: this test cannot see staleness"
        # ... until texture mark_written()
        hzb.mark_written()
        frame_and_check("out of band, then trhip_texture_mark_written")
        raw.release()
    finally:
        other.release()
        t.release()
