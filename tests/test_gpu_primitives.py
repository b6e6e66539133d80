"""The arithmetic the cull kernels are exact by, checked on the GPU against correctly rounded fp64 references.

The scene tests compare whole frames with the CPU oracle, which draws on a tiny part of the operand space.  Here the
instruction sequences of toyrenderer_amd/csrc/cull_math.hip.h -- the real cm:: functions, compiled with the product's
flags into the test-only library lib/libtrhip_probe.so (tests/hip/cull_arith_probe.hip) -- are swept over their whole
domains, exhaustively where the domain is 2^32 patterns or fewer.  The references (tests/hip/fp_ref.h) take an fp64
candidate and settle its rounding exactly at the neighbouring midpoints; tests/test_probe_ref.py checks them against exact
rationals on the CPU.  Each check asserts zero mismatches and names the first failing inputs; each negative control asserts
that the checker does see a failure where one is known to exist.

What this does not prove: the sequences are checked as compiled into the probe.  The product's own compilation of them is
checked by the scene-level parity tests.
"""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from suite_support import PROBE_LAUNCHERS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(ROOT, "toyrenderer_amd", "lib", "libtrhip_probe.so")

# every launcher this file binds (tests/test_probe_ref.py checks that the library exports them)
RSQ, RCP, SQRTSEQ1, SQRTSEQ2, SQRT2, SQRT2_LANE0_OUT = range(6)
BYTES, HZB_LEVEL, FREXP_LEVEL = range(3)

F32_MIN_NORMAL = 0x00800000
F32_INF = 0x7F800000
NO_TOL = 0xFFFFFFFF


class ProbeResult(C.Structure):
    _fields_ = [("tested", C.c_uint64), ("mismatches", C.c_uint64), ("hist", C.c_uint64 * 8), ("aux", C.c_uint64 * 8),
                ("maxUlp", C.c_uint32), ("nfail", C.c_uint32), ("fail", (C.c_uint32 * 4) * 64)]

    def histogram(self):
        return dict(zip(["0", "1", "2", "3", "4", "5", "6-15", ">=16"], [int(h) for h in self.hist]))

    def failures(self, n=8):
        rows = [tuple(f"0x{int(w):08x}" for w in self.fail[i]) for i in range(min(int(self.nfail), 64, n))]
        return f"{int(self.mismatches)} of {int(self.tested)} outside the expectation; first (a, b, got, expected): {rows}"


_LIB = None


def probe():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(PROBE_PATH)
        u32, u64, f32, p = C.c_uint32, C.c_uint64, C.c_float, C.POINTER(ProbeResult)
        lib.probe_result_size.restype = u32
        lib.probe_unary.argtypes = [C.c_int, u64, u64, u32, p]
        lib.probe_div2.argtypes = [C.c_int, u64, u64, C.POINTER(u32), u32, p]
        lib.probe_quotient.argtypes = [C.c_int, u64, u64, C.POINTER(u32), u32, p]
        lib.probe_levels.argtypes = [C.c_int, u64, u64, u32, p]
        lib.probe_step.argtypes = [C.c_int, C.c_int, C.c_int, u64, f32, p]
        lib.probe_filtered.argtypes = [C.c_int, u64, f32, f32, f32, u32, u32, u32, C.POINTER(f32), C.c_int, p]
        for name in PROBE_LAUNCHERS[:-1]:
            getattr(lib, name).restype = C.c_int
        assert lib.probe_result_size() == C.sizeof(ProbeResult)
        _LIB = lib
    return _LIB


def run(name, *args):
    r = ProbeResult()
    rc = getattr(probe(), name)(*args, C.byref(r))
    assert rc == 0, f"{name}: hipError_t {rc}"
    assert r.tested > 0
    return r


def u32s(values):
    return (C.c_uint32 * len(values))(*values)


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ---- A: v_rsq_f32 / v_rcp_f32 within 1 ulp of the correctly rounded value ----------------------------------------------
# the premise of the filtered projection's and the cone test's error bounds (cull_math.hip.h, FILTERED PROJECTION / coneBack)

@pytest.mark.gpu
def test_rsq_within_one_ulp_of_correctly_rounded():
    r = run("probe_unary", RSQ, F32_MIN_NORMAL, F32_INF - F32_MIN_NORMAL, 1)        # every positive normal: result normal
    print(f"\nv_rsq_f32, normal inputs: {r.histogram()}")
    assert r.tested == F32_INF - F32_MIN_NORMAL
    assert r.mismatches == 0, r.failures()
    sub = run("probe_unary", RSQ, 1, F32_MIN_NORMAL - 1, NO_TOL)                   # reported, not asserted
    print(f"v_rsq_f32, subnormal inputs (not asserted): {sub.histogram()}")


@pytest.mark.gpu
def test_rcp_within_one_ulp_of_correctly_rounded():
    hi = 0x7E800000                                                                # 2^126: 1 / x still normal
    hist = np.zeros(8, np.uint64)
    for sign in (0, 0x80000000):
        r = run("probe_unary", RCP, sign | F32_MIN_NORMAL, hi - F32_MIN_NORMAL + 1, 1)
        assert r.tested == hi - F32_MIN_NORMAL + 1
        assert r.mismatches == 0, r.failures()
        hist += np.array(r.hist, np.uint64)
    print(f"\nv_rcp_f32, normal inputs with a normal result, both signs: {dict(zip(ProbeResult().histogram(), hist.tolist()))}")
    sub = run("probe_unary", RCP, 1, F32_MIN_NORMAL - 1, NO_TOL)
    print(f"v_rcp_f32, subnormal inputs (not asserted): {sub.histogram()}")


# ---- B: the 8-operation square root, exhaustively on [2^-96, FLT_MAX] -------------------------------------------------
SQRT_LO = 0x0F800000                                                               # 2^-96
SQRT_N = 0x7F800000 - SQRT_LO                                                      # up to FLT_MAX: 1 879 048 192 floats


@pytest.mark.gpu
@pytest.mark.parametrize("op", [SQRTSEQ1, SQRTSEQ2], ids=["sqrtSeq1", "sqrtSeq2"])
def test_sqrt_sequence_correctly_rounded_on_its_range(op):
    r = run("probe_unary", op, SQRT_LO, SQRT_N, 0)
    assert r.tested == SQRT_N * (2 if op == SQRTSEQ2 else 1)
    assert r.mismatches == 0, r.failures()


@pytest.mark.gpu
def test_sqrt_sequence_negative_control_below_its_range():
    """Below 2^-96 the sequence is not exact (why sqrt2 guards its range): the sweep must see it."""
    r = run("probe_unary", SQRTSEQ1, F32_MIN_NORMAL, SQRT_LO - F32_MIN_NORMAL, 0)
    assert r.mismatches > 0


# ---- C: sqrt2, every bit pattern, with its range guard and the wave fallback ------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("op", [SQRT2, SQRT2_LANE0_OUT], ids=["consecutive", "lane0_out_of_range"])
def test_sqrt2_every_pattern(op):
    """Equal to the reference for all 2^32 patterns: -0 -> -0, negative -> NaN, +inf -> +inf, subnormals kept."""
    r = run("probe_unary", op, 0, 1 << 32, 0)
    assert r.tested == 2 << 32
    assert r.mismatches == 0, r.failures()


# ---- D: div2 ------------------------------------------------------------------------------------------------------------
DIV_SET = [0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x40400000, 0x00800000, 0x80800000, 0x00000001,
           0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x4B3C1F2D]
DIV_RANDOM = [0x1A2B3C4D, 0xC0490FDB, 0x2F800123, 0xE1000007, 0x5E5A0F11, 0x80345678, 0x3EAAAAAB, 0x7E7FFFFF]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["every_denominator", "every_numerator"])
def test_div2_every_pattern_against_a_set(mode):
    for values in (DIV_SET, DIV_RANDOM):
        r = run("probe_div2", mode, 0, 1 << 32, u32s(values), len(values))
        assert r.tested == len(values) << 32
        assert r.mismatches == 0, r.failures()


@pytest.mark.gpu
def test_div2_hashed_pairs_every_exponent_pair_and_midpoints():
    r = run("probe_div2", 2, 0, 1 << 32, None, 0)
    assert r.tested == 2 << 32
    assert r.mismatches == 0, r.failures()
    # every (numerator, denominator) exponent pair incl. subnormal / overflowing quotients and gaps >= 96: 2048 pairs each
    r = run("probe_div2", 3, 0, 1 << 27, None, 0)
    assert r.tested == 2 << 27
    assert r.mismatches == 0, r.failures()
    # quotients within 2^-45 (relative) of a rounding midpoint, exponents anywhere (subnormal and overflowing ones included)
    r = run("probe_div2", 4, 0, 1 << 30, None, 0)
    assert r.tested == 2 << 30
    assert r.mismatches == 0, r.failures()


# ---- E: rcpRefined + quotient (stepQuotients' fast division, stepDeferred's depthSphere) ------------------------------

def _triples():
    """(n exponent + 127, d exponent + 127, n sign | mantissa): the corners of [2^-30, 2^63) and a middle pair."""
    corners = [(-30, -30), (-30, 62), (62, -30), (62, 62), (0, 0), (20, -10), (-17, 41), (5, 5)]
    mants = [0x000000, 0x7FFFFF, 0x80400001, 0x2AAAAB]
    return [(a + 127, b + 127, m) for a, b in corners for m in mants]


@pytest.mark.gpu
def test_quotient_every_denominator_mantissa():
    """All 2^23 d mantissas x 4 n mantissas at 8 exponent pairs (the sequence is scale invariant inside the domain: the
    exponent pairs themselves are covered by the next test)."""
    t = _triples()
    flat = [w for tr in t for w in tr]
    r = run("probe_quotient", 0, 0, len(t) << 23, u32s(flat), len(t))
    assert r.tested == 3 * (len(t) << 23)
    assert r.mismatches == 0, r.failures()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,count", [(1, (93 * 93) << 16), (2, 1 << 30), (3, 1 << 26)],
                         ids=["every_exponent_pair", "near_midpoints", "near_plane"])
def test_quotient_correctly_rounded_in_the_safe_range(mode, count):
    r = run("probe_quotient", mode, 0, count, None, 0)
    assert r.tested == 3 * count
    assert r.mismatches == 0, r.failures()


@pytest.mark.gpu
def test_quotient_negative_control_outside_the_range():
    """d >= 2^126: the reciprocal / quotient is subnormal and the unscaled sequence is not exact -- the check sees it."""
    r = run("probe_quotient", 4, 0, 1 << 20, None, 0)
    assert r.mismatches > 0


# ---- F: stepQuotients' FAST branch against its EXACT branch -------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("occ,cone", [(1, 0), (0, 1), (1, 1)], ids=["occ", "cone", "occ_cone"])
@pytest.mark.parametrize("layout", [0, 1, 2], ids=["all_safe", "unsafe_lane_inactive", "unsafe_lane_active"])
def test_step_quotients_fast_branch(occ, cone, layout):
    """mn, mx, depthSphere bit for bit; tn and lenC within 5 ulp of the exact ones (coneBack's premise).  An unsafe
    lane that is inactive must not send the wave down the exact branch; an active one must."""
    n = 1 << 24
    r = run("probe_step", occ, cone, layout, n, 0.1)
    assert r.mismatches == 0, r.failures()
    if cone:
        assert r.maxUlp <= 5, r.maxUlp
    fast, exact = int(r.aux[0]), int(r.aux[1])
    assert fast + exact == n // 64
    if layout == 2:
        assert fast == 0
    else:
        assert fast > 0.5 * (fast + exact), (fast, exact)                          # the fast branch was exercised


# ---- G: the deferred mode's sure lanes ----------------------------------------------------------------------------------

def _view_rotation(yaw=0.3, pitch=-0.2):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]])
    return (C.c_float * 9)(*(ry @ rx).astype(np.float32).ravel().tolist())


# (P00, P11, HZB width, height, mips): a 16:9 view on a non-square HZB, a square one, a wide one
FILTER_SETTINGS = [(0.974279, 1.732051, 640, 360, 10), (1.0, 1.0, 1024, 1024, 11), (0.5, 0.9, 2048, 1024, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("setting", range(len(FILTER_SETTINGS)))
def test_filtered_projection_and_cone_sure_lanes(setting):
    """For every lane marked sure: the table entry (mip level, footprint origin) equals occTailQuad's from the exact
    quotients, the exact footprint has no zero weight, depthSphere is exact, and the cone decision equals
    coneBackfacingP's."""
    P00, P11, w, h, mips = FILTER_SETTINGS[setting]
    n = 340_000_000                                                                # > 10^9 spheres over the three settings
    r = run("probe_filtered", 1, n, P00, P11, 0.1, w, h, mips, _view_rotation(), 0)
    assert r.mismatches == 0, r.failures()
    matters, sure, cone, cone_sure = int(r.aux[0]), int(r.tested), int(r.aux[3]), int(r.aux[4])
    print(f"\nsetting {setting}: sure {sure}/{matters} projections, {cone_sure}/{cone} cone decisions")
    assert sure > 0.3 * matters, (sure, matters)
    assert cone_sure > 0.3 * cone, (cone_sure, cone)


@pytest.mark.gpu
def test_filtered_projection_without_cone():
    P00, P11, w, h, mips = FILTER_SETTINGS[0]
    r = run("probe_filtered", 0, 1 << 26, P00, P11, 0.1, w, h, mips, _view_rotation(), 0)
    assert r.mismatches == 0, r.failures()
    assert r.tested > 0.3 * r.aux[0]


@pytest.mark.gpu
def test_filtered_projection_negative_control_without_bands():
    """Bands zeroed (K = 0, mipDelta = 0) in the probe: sure lanes that disagree with the exact quotients appear."""
    P00, P11, w, h, mips = FILTER_SETTINGS[0]
    r = run("probe_filtered", 0, 1 << 26, P00, P11, 0.1, w, h, mips, _view_rotation(), 1)
    assert r.mismatches > 0


# ---- H: byte decode, hzbLevel, the frexp level choice -------------------------------------------------------------------

@pytest.mark.gpu
def test_byte_decode_all_256():
    """u8Unorm, coneTableEntry = RN(x / 255); coneAxisCutoff's axis = fma(q, 2, -1), its cutoff = q of the top byte."""
    r = run("probe_levels", BYTES, 0, 256, 0)
    assert r.tested == 256 * 7
    assert r.mismatches == 0, r.failures()


@pytest.mark.gpu
@pytest.mark.parametrize("mips", [1, 10, 16])
def test_hzb_level_every_pattern(mips):
    """floor(log2(max(w, h))) clamped to the mip count; below 1 and NaN -> 0 (Q6), +inf -> the last mip."""
    r = run("probe_levels", HZB_LEVEL, 0, 1 << 32, mips)
    assert r.tested == 2 << 32
    assert r.mismatches == 0, r.failures()


@pytest.mark.gpu
@pytest.mark.parametrize("mips", [1, 10, 16])
def test_frexp_level_choice_every_finite_m(mips):
    """occTailQuad's e = v_frexp_exp(m) clamped to [1, mips] is floor(log2 m) + 1 for every finite m >= 1.  v_frexp_exp
    returns 0 for inf and NaN; the clamps in front of it (w, h <= the HZB size, max(., 1)) keep m finite, so no level is
    asserted for them."""
    lo = bits(1.0)
    r = run("probe_levels", FREXP_LEVEL, lo, F32_INF - lo, mips)
    assert r.tested == F32_INF - lo
    assert r.mismatches == 0, r.failures()
