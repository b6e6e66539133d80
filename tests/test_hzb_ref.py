"""CPU tests that tie tests/hzb_ref.py (the numpy reference of the HZB build and the footprint-min table, which
tests/test_gpu_hzb.py holds the kernels to) to the oracle every cull test already trusts, and pin the places where a
formula decides: the fp32 gather index and the fp16 conversion."""
import ctypes as C

import numpy as np
import pytest

from toyrenderer_amd import interop as I
from toyrenderer_amd import synth

from . import hzb_ref as R

RENDERS = [(100, 40), (640, 360), (1920, 1080), (3840, 2160), (2560, 1440), (2048, 64), (48, 3000)]      # test_gpu_parity.py::test_hzb_build


def _oracle_chain(oracle, depth, w, h):
    t = oracle.HzbTexture(w, h)
    t.build_from_depth(depth)
    return t


@pytest.mark.parametrize("render", RENDERS)
def test_min_build_equals_the_oracle_on_the_renders_of_test_hzb_build(oracle, render):
    rng = np.random.default_rng(render[0])
    depth = rng.random((render[1], render[0]), np.float32) ** 6
    depth[rng.random(depth.shape) < 0.2] = 0
    w, h = I.hzb_dims(*render)
    ref = _oracle_chain(oracle, depth, w, h)
    assert ref.mips == R.num_mips(w, h)
    assert np.array_equal(R.pack(R.build(depth, w, h, False)), ref.texels)


@pytest.mark.parametrize("depth_dims,hzb", [((129, 65), (128, 64)), ((100, 40), (64, 32)), ((40, 23), (64, 64)), ((1000, 600), (64, 64)),
                                            ((2, 70), (64, 64)), ((1, 1), (64, 128)), ((4097, 70), (4096, 64))])
def test_min_build_equals_the_oracle_on_hostile_values(oracle, depth_dims, hzb):
    """The value classes of hzb_ref.hostile_depth that the oracle defines: all of them; a NaN result is compared as "is NaN"
    (orc_f32_to_f16 keeps a payload, fminf only promises A NaN)."""
    W, H = depth_dims
    w, h = hzb
    depth = R.hostile_depth(W, H, seed=W * 7 + H)
    ref = _oracle_chain(oracle, depth, w, h)
    got = R.pack(R.build(depth, w, h, False))
    assert R.same_words(got, ref.texels).all()
    assert not (got == 0x8000).any(), "-0.0 is outside the reference (hzb_ref.py)"
    if (W, H) == (129, 65):                                              # every class reaches the output: NaN, +inf, -inf, subnormals, negatives
        assert ((got & 0x7FFF) > 0x7C00).any() and (got == 0x7C00).any() and (got == 0xFC00).any()
        assert (((got & 0x7C00) == 0) & ((got & 0x3FF) != 0)).any() and ((got & 0x8000) != 0).any()


def test_max_build_is_the_mirror_image_of_the_min_build():
    """max(x) = -min(-x) on NaN-free data without zeros of either sign: the max variant has no oracle, so it is tied to the min one."""
    rng = np.random.default_rng(5)
    depth = (rng.random((90, 150), np.float32) + np.float32(0.001)) * np.where(rng.random((90, 150)) < 0.5, -1, 1).astype(np.float32)
    mx = R.build(depth, 128, 64, True)
    mn = R.build(-depth, 128, 64, False)
    assert all(np.array_equal(a, -b) for a, b in zip(mx, mn))
    assert not np.array_equal(R.pack(mx), R.pack(R.build(depth, 128, 64, False)))


# The first render widths above 4096 at which the fp32 index differs from the exact one in some column (HZB 4096 wide); 9227
# of the widths 4097 .. 16384 do, in up to 4 columns.  Up to 4096 none does: the fp32 formula is pinned there by accident.
FIRST_FP32_INDEX_DIFFERENCES = [4097, 4098, 4099, 4101, 4103, 4105, 4107, 4109, 4111, 4115, 4117, 4125]


def test_fp32_gather_index_is_the_exact_one_up_to_4096():
    bad = []
    for W in range(2, 4097):
        ow = I.hzb_dims(W, W)[0]
        n = int((R.gather_index_fp32(ow, W) != R.gather_index_exact(ow, W)).sum())
        if n:
            bad.append((W, n))
    assert bad == [], bad[:10]                                           # widths and heights alike: the index is the same function of (dim, out)


def test_fp32_gather_index_differs_above_4096_where_listed():
    got = []
    W = 4097
    while len(got) < len(FIRST_FP32_INDEX_DIFFERENCES):
        ow = I.hzb_dims(W, W)[0]
        if (R.gather_index_fp32(ow, W) != R.gather_index_exact(ow, W)).any():
            got.append(W)
        W += 1
    assert got == FIRST_FP32_INDEX_DIFFERENCES


def test_fp32_gather_index_is_the_scalar_fmaf_formula():
    """The vectorised index against interop.fmaf (the exact scalar fp32 fma the cull tests use), on widths where rounding decides."""
    for W, ow in [(4097, 4096), (4125, 4096), (1000, 64), (40, 64), (2, 64), (1, 64), (7681, 4096)]:
        ref = [int(np.floor(I.fmaf(np.float32(np.float32(x) + np.float32(0.5)) / np.float32(ow), np.float32(W), np.float32(-0.5)))) for x in range(ow)]
        assert np.array_equal(R.gather_index_fp32(ow, W), np.array(ref, np.int64)), (W, ow)


def test_orc_f32_to_f16_is_round_to_nearest_even(oracle):
    """Every fp32 that is a half, its two fp32 neighbours, every midpoint between adjacent halves with its two neighbours
    (subnormals included), both signs, +-65504, 65520 and +-inf."""
    halves = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    halves = halves[(halves & 0x7FFF) <= 0x7C00].view(np.float16).astype(np.float32)
    mid = R.half_midpoints()
    base = np.concatenate([halves, mid, -mid, np.array([65504.0, -65504.0, 65520.0, -65520.0, np.inf, -np.inf], np.float32)])
    x = np.concatenate([base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))]).astype(np.float32)
    x = x[~np.isnan(x)]
    assert len(x) > 6 * 63488 // 2
    with np.errstate(over="ignore"):
        ref = x.astype(np.float16).view(np.uint16)
    fn = oracle.lib().orc_f32_to_f16
    got = np.fromiter((fn(C.c_float(v)) for v in x.tolist()), np.uint16, len(x))
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, [(float(x[i]), hex(int(got[i])), hex(int(ref[i]))) for i in bad[:8]]


@pytest.mark.parametrize("hzb_dims", [(512, 256), (64, 64), (128, 1024)])
def test_table_entry_is_the_footprint_the_oracle_sampler_reads(oracle, hzb_dims):
    """A table() entry (x0 + 1, y0 + 1) of the lookup's level equals the min of the four texels the oracle's min-reduction sampler
    reads for a lookup with origin (x0, y0) and non-zero weights -- and what orc_sample_hzb_min itself returns is not checked
    here but by every cull test; this ties the TABLE's definition to the sampler's footprint."""
    w, h = hzb_dims
    rng = np.random.default_rng(w + h)
    view = synth.make_view(render=(2 * w, 2 * h))
    assert tuple(view.hzb_dims) == (w, h)
    tex = oracle.HzbTexture(w, h)
    tex.texels[:] = rng.permutation(R.all_halves())[rng.integers(0, 63489, tex.total)]
    mips = R.unpack(tex.texels, w, h)
    tab = R.table(mips, w, h)
    n = 200_000
    z = rng.uniform(2, 400, n).astype(np.float32)
    c = np.stack([rng.uniform(-0.9, 0.9, n) * z, rng.uniform(-0.6, 0.6, n) * z, -z], 1).astype(np.float32)
    r = (rng.uniform(0.001, 0.6, n) * z).astype(np.float32)
    fp = oracle.occlusion_footprints(c, r, view.as_dict(), (w, h))
    fp = fp[(fp[:, 3] == 0) & (fp[:, 4] == 0)]                           # both weights per axis non-zero
    assert len(fp) > n // 2 and len(np.unique(fp[:, 0])) >= 6
    seen_border = 0
    for k in np.unique(fp[:, 0]):
        f = fp[fp[:, 0] == k]
        mw, mh = R.mip_dims(w, h, k)
        x0, y0 = f[:, 1], f[:, 2]
        assert (x0 >= -1).all() and (x0 <= mw - 1).all() and (y0 >= -1).all() and (y0 <= mh - 1).all()
        t = tex.mip(k).view(np.float16)
        cx = lambda v: np.clip(v, 0, mw - 1)
        cy = lambda v: np.clip(v, 0, mh - 1)
        four = np.stack([t[cy(y0), cx(x0)], t[cy(y0), cx(x0 + 1)], t[cy(y0 + 1), cx(x0)], t[cy(y0 + 1), cx(x0 + 1)]])
        want = np.fmin.reduce(four.astype(np.float32), axis=0).astype(np.float16)
        got = tab[k][y0 + 1, x0 + 1]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), k
        seen_border += int(((x0 == -1) | (x0 == mw - 1) | (y0 == -1) | (y0 == mh - 1)).sum())
    assert seen_border > 0


def test_table_layout_is_a_bijection_onto_the_defined_entries():
    for w, h in [(2048, 1024), (256, 128), (64, 32), (32, 2048), (1, 1), (8, 8)]:
        offs, total = R.table_layout(w, h)
        words, defined = R.table_packed(R.chain(np.zeros((h, w), np.float16), w, h), w, h)
        assert len(words) == total and total % 64 == 0
        assert int(defined.sum()) == sum((mw + 1) * (mh + 1) for mw, mh in (R.mip_dims(w, h, k) for k in range(R.num_mips(w, h))))
        assert offs[0] == 0 and all(b > a for a, b in zip(offs, offs[1:]))
