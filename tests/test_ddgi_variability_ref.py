"""tests/ddgi_variability_ref.c, the definition of probe variability, and the convergence rule of csrc/host/DDGIVariability.h, on
the CPU: the reference's blend equals tests/ddgi_update_ref.c's word for word and takes every branch of the variability value; its
average agrees with a float64 mean; its tree is the stated one; and the host library's rule and ddgi.VariabilityTracker agree bit for
bit, converge on the 18th call at the earliest, store 0 for what is not normal, decide as < says, and freeze once converged."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_update_ref as DU  # noqa: E402
import ddgi_variability_ref as DV  # noqa: E402
import ddgi_variability_scenes as VS  # noqa: E402
from suite_support import ref_library  # noqa: E402
from toyrenderer_amd import ddgi  # noqa: E402

F = np.float32
dv = ref_library(DV)


# ---- the value ------------------------------------------------------------------------------------------------------------------------------
# {case: rule -> texels} of VS.blend_volume() / VS.blend_rays(), counted by test_the_blend_cases_take_every_branch
# (at_floor: lumMean == 2^-10 exactly with lumS2 > 0, the texels at which <= and < at the floor give different values)
BRANCHES = {"default": dict(left_alone_probes=3, cleared=6, floor=22, cap=30, darker=289, mean_floor=35, s2_negative=0, s2_zero=6, positive=504, at_floor=0),
            "settled": dict(left_alone_probes=3, cleared=6, floor=0, cap=24, darker=280, mean_floor=36, s2_negative=14, s2_zero=506, positive=20, at_floor=0),
            "floor": dict(left_alone_probes=0, cleared=0, floor=0, cap=0, darker=0, mean_floor=36, s2_negative=0, s2_zero=0, positive=0, at_floor=14)}


def branch_counts(rules, var):
    c = lambda bit: int(np.count_nonzero(rules & bit))  # noqa: E731
    return dict(left_alone_probes=c(DU.R_LEFT_ALONE) // 36, cleared=c(DU.R_PREV_ZERO), floor=c(DU.any_channel(DU.R_FLOOR)), cap=c(DU.any_channel(DU.R_CAP)), darker=c(DU.R_DARKER),
                mean_floor=c(DV.MEAN_FLOOR), s2_negative=c(DV.S2_NEGATIVE), s2_zero=c(DV.S2_ZERO), positive=int(np.count_nonzero(var > 0)),
                at_floor=c(DV.MEAN_AT_FLOOR))


@pytest.mark.parametrize("name", list(VS.BLEND_CONSTS))
def test_the_blend_cases_take_every_branch(dv, name):
    """Every case: the irradiance equals du_blend_radiance's (res, prev and out are that file's), the left-alone probes (in the
    seeded volume two inactive and one with 25 back faces) keep the sentinel, no NaN is born, and the branch counts are BRANCHES'.
    Between them the cases hold cleared texels, texels the darker-step floor moves, lumMean below the floor, lumMean EXACTLY at the
    floor with positive lumS2 (14 texels of "floor": 0 by <=) and negative lumS2."""
    vol, rays, k = VS.blend_volume(name), VS.blend_rays(name), VS.blend_consts(name)
    init = np.full(DV.variability_shape(vol), VS.SENTINEL, F)
    irr, var, rules = DV.blend_radiance(dv, k, vol, rays, init)
    want, _ = DU.blend(dv, k, vol, rays)
    assert np.array_equal(irr, want)
    assert not np.isnan(var).any() and np.isfinite(var).all()
    assert np.count_nonzero(var == VS.SENTINEL) == VS.LEFT_ALONE[name] * 36 and np.all((var >= 0) | (var == VS.SENTINEL))
    assert branch_counts(rules, var) == BRANCHES[name]
    together = {key: sum(b[key] for b in BRANCHES.values()) for key in BRANCHES["default"]}
    assert all(v > 0 for v in together.values()), together
    if name == "floor":
        at = (rules & DV.MEAN_AT_FLOOR) != 0
        assert not var.reshape(rules.shape)[at].any(), "at the floor the value is 0: <=, not <"


def test_the_value_at_its_guards(dv):
    """lumMean one ulp above the floor passes, at the floor it gives 0 (<=); a negative and a zero lumS2 give 0, never a NaN."""
    one = np.ones(3, F)
    floor = F(1.0 / 1024.0)
    # search the floats around the floor for an `out` whose reference luminance is <= floor and one whose luminance is just above
    at, above = None, None
    m = floor
    for _ in range(64):
        v = DV.texel(dv, one, np.zeros(3, F), m * one)
        if v == 0 and at is None:
            at = m
        if v > 0:
            above = m
            break
        m = np.nextafter(m, F(1.0))
    assert at is not None and above is not None and DV.texel(dv, one, np.zeros(3, F), above * one) > 0
    assert DV.texel(dv, one, np.zeros(3, F), at * one) == 0
    res, prev = np.array([0.5, 0.5, 0.5], F), np.array([0.25, 0.25, 0.25], F)
    assert DV.texel(dv, res, prev, np.array([0.75, 0.75, 0.75], F)) == 0          # out beyond res: every product negative
    assert DV.texel(dv, res, prev, res) == 0                                       # out == res: lumS2 == 0
    v = DV.texel(dv, res, prev, np.array([0.375, 0.375, 0.375], F))                # s2 = 0.25 * 0.125 per channel
    assert v > 0 and abs(float(v) - np.sqrt(0.03125) / 0.375) < 1e-6
    assert DV.texel(dv, np.full(3, np.nan, F), prev, res) == 0                     # a NaN estimate: !(lumS2 > 0)


# ---- the reductions ------------------------------------------------------------------------------------------------------------------------
# |reference average - float64 mean over the weight-1 texels|, measured on VS.REDUCTION_CASES (profiles/ddgi/README.md)
MEASURED = {"1x1x1": 5.290e-09, "3x2x3": 2.618e-08, "3x5x1": 1.582e-08, "43x1x1": 1.704e-08, "all inactive": 0.0, "stale": 2.618e-08, "tree": 3.449e-11}
PASSES = {"1x1x1": 1, "3x2x3": 2, "3x5x1": 2, "43x1x1": 3, "all inactive": 2, "stale": 2, "tree": 1}


@pytest.mark.parametrize("name", list(VS.REDUCTION_CASES))
def test_the_average_agrees_with_a_float64_mean(dv, name):
    """dv_average against numpy's float64 mean over the weight-1 texels: within the measured difference plus one ulp of the
    average.  The pass count, the weight (the number of weight-1 texels, exact) and the pass-by-pass wrapper agree with it."""
    vol, var = VS.reduction_case(name)
    a, w, n = DV.average(dv, vol, var)
    act = DV.active_texels(dv, vol)
    mean = float(var.astype(np.float64)[act].mean()) if act.any() else 0.0
    diff = abs(float(a) - mean)
    print(f"{name}: average {a!r}, float64 mean {mean!r}, difference {diff:.3e}, ulp {float(np.spacing(a)):.3e}")
    assert np.isfinite(a) and diff <= MEASURED[name] * 1.0005 + float(np.spacing(a))
    assert w == F(np.count_nonzero(act)) and n == PASSES[name]
    ps = DV.passes(dv, vol, var)
    assert len(ps) == n and ps[-1].shape == (1, 1, 1, 2) and ps[-1].reshape(-1).view(np.uint32).tolist() == [a.view(np.uint32), w.view(np.uint32)]
    assert not any(np.isnan(p).any() for p in ps)
    if name == "all inactive":
        assert a == 0 and w == 0 and all(not p.any() for p in ps)


def test_the_tree_is_the_stated_one(dv):
    """2^24 at thread 0, 1 at thread 1, -2^24 at thread 64: strides 64, 32, ..., 1 cancel the large pair first and give 1; strides
    ascending, or the threads in sequence, round 2^24 + 1 back to 2^24 and give 0.  Through dv_tree and through the first pass."""
    p = np.zeros(128, F)
    p[0], p[1], p[64] = 2.0 ** 24, 1.0, -(2.0 ** 24)
    assert DV.tree(dv, p) == 1.0
    ascending = p.copy()
    stride = 1
    while stride < 128:
        for t in range(0, 128, 2 * stride):
            ascending[t] = F(ascending[t] + ascending[t + stride])
        stride *= 2
    sequential = F(0.0)
    for v in p:
        sequential = F(sequential + v)
    assert ascending[0] == 0.0 and sequential == 0.0
    vol, var = VS.reduction_case("tree")
    a, w, n = DV.average(dv, vol, var)
    assert (a, w, n) == (F(1.0) / F(216.0), F(216.0), 1)


# ---- the host rule -------------------------------------------------------------------------------------------------------------------------
def _sequences():
    rng = np.random.default_rng(31)
    out = []
    for i in range(6):
        n = 80
        a = (rng.uniform(0.0, 0.05, n) * np.exp(-np.arange(n) / rng.uniform(3, 30))).astype(F) + F(0.003)
        a += (rng.normal(0, 2e-4 * (i + 1), n)).astype(F)
        out.append(a.astype(F))
    return out


def test_the_host_rule_and_the_tracker_agree_bit_for_bit():
    """trhost_ddgi_variability_run (csrc/host/DDGIVariability.h; the host library loads without a device) against
    ddgi.VariabilityTracker on seeded decaying sequences: verdict and standard deviation after every Update."""
    from toyrenderer_amd import host
    hit = 0
    for a in _sequences():
        for threshold in (0.001, 0.0003, 0.0):
            c1, d1 = host.ddgi_variability_run(a, threshold)
            c2, d2 = ddgi.VariabilityTracker.run(a, threshold)
            assert np.array_equal(c1, c2) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))
            hit += int(c1.any())
            assert not c1[:17].any()
    assert hit >= 6


def test_a_constant_sequence_converges_on_the_18th_call():
    from toyrenderer_amd import host
    for run in (host.ddgi_variability_run, ddgi.VariabilityTracker.run):
        c, d = run(np.full(30, 0.25, F), 0.001)
        assert not c[:17].any() and c[17:].all(), "the 18th call, not the 17th"
        assert d[0] == 0 and d[16] == 0 and d[8] == F(0.125)                 # the ring full of 0.25 at the 17th Update already: the count decides


def test_what_is_not_normal_is_stored_as_zero():
    """One NaN, one inf and one denormal: three zeros in the ring; the standard deviation is that of the sequence with zeros."""
    from toyrenderer_amd import host
    a = np.full(16, 0.5, F)
    a[3], a[7], a[11] = np.nan, np.inf, F(1e-40)
    t = ddgi.VariabilityTracker(0.001)
    for v in a:
        t.update(); t.set(v)
    assert np.count_nonzero(t.ring == 0) == 3 and np.count_nonzero(t.ring == F(0.5)) == 13 and np.isfinite(t.ring).all()
    clean = np.where(np.isin(np.arange(16), (3, 7, 11)), F(0.0), a).astype(F)
    for run in (host.ddgi_variability_run, ddgi.VariabilityTracker.run):
        c1, d1 = run(np.concatenate([a, a[:1]]), 0.001)
        c2, d2 = run(np.concatenate([clean, clean[:1]]), 0.001)
        assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32)) and np.isfinite(d1).all() and d1[16] > 0.1


def test_the_threshold_decides_as_less_than_says():
    """The standard deviation of a settled ring, and thresholds one ulp to either side of it: below and at it nothing converges,
    one ulp above it the 18th call does."""
    from toyrenderer_amd import host
    a = np.tile(np.array([0.25, 0.2501], F), 20)
    _, d = host.ddgi_variability_run(a, 0.0)
    s = d[20]
    assert s > 0 and np.all(d[17:] == s)
    for run in (host.ddgi_variability_run, ddgi.VariabilityTracker.run):
        assert not run(a, float(np.nextafter(s, F(0))))[0].any()
        assert not run(a, float(s))[0].any(), "stddev < threshold, not <="
        c, _ = run(a, float(np.nextafter(s, F(1))))
        assert not c[:17].any() and c[17:].all()


def test_after_convergence_the_state_does_not_change():
    """Once converged the ring is frozen (no sample is stored): whatever follows, the verdict stays and the deviation is the same
    word; only the cursor and the count move on.  reset() re-arms: 17 more calls before the next verdict."""
    from toyrenderer_amd import host
    a = np.concatenate([np.full(20, 0.25, F), np.array([100.0, np.nan, 0.0, 7.0, -3.0] * 4, F)])
    for run in (host.ddgi_variability_run, ddgi.VariabilityTracker.run):
        c, d = run(a, 0.001)
        assert c[17:].all() and np.all(d[17:].view(np.uint32) == d[17].view(np.uint32))
    t = ddgi.VariabilityTracker(0.001)
    for v in a[:20]:
        if not t.update():
            t.set(v)
    assert t.converged
    ring, cursor, samples = t.ring.copy(), t.cursor, t.samples
    assert t.update() and np.array_equal(t.ring, ring) and t.cursor == (cursor + 1) % 16 and t.samples == samples + 1
    t.reset()
    assert not t.converged and t.samples == 0 and t.cursor == 0 and not t.ring.any() and t.stddev == F(1e10)
    assert [t.update() or t.set(0.25) for _ in range(17)] == [None] * 17 and t.update()
