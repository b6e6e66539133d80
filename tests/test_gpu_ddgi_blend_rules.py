"""The two DDGI probe blends ("ProbeBlendingCS_DDGIProbeBlendingCS"; csrc/k_giprobeblend.hip) on the GPU on both sides of every rule
they apply: the cases of tests/ddgi_blend_scenes.py BLEND_CASES, every word of both textures after every chained update against
tests/ddgi_update_ref.c, borders included, NaN halves as bit patterns.  tests/test_gpu_ddgi_update.py feeds the same kernels uniform
random numbers; here the previous codes straddle both thresholds one code apart, estimates pass 1 and fall below 0, gamma, the
hysteresis, the thresholds and the distance exponent leave their defaults, records hold NaN, infinities and both zeros, distance texels
leave binary16's normal range at both ends, and the blends run behind the traces of two TRACE_CASES under a strong light.  Only values
are hostile: every address still comes from the descriptor.  tests/test_ddgi_update_ref.py holds the preconditions (which rule the
reference took how often in each case); profiles/ddgi/blend_mutations.txt the negative controls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_blend_scenes as BS  # noqa: E402
import ddgi_update_ref as DU  # noqa: E402
from ddgi_passes import RAY_SENTINEL, Update, trace_case  # noqa: E402
from suite_support import bare_gpu_scene, dev, ref_library, same, sm  # noqa: E402, F401

pytestmark = pytest.mark.gpu
F = np.float32
du = ref_library(DU)


def _left_alone_tiles_kept(name, step, vol, rules, n, got, before):
    """The tiles of probes the reference left alone equal their previous contents word for word, border included."""
    for p in np.flatnonzero(rules.reshape(len(rules), -1)[:, 0] & 1):
        x, y, z = BS._coords(vol, int(p))
        assert np.array_equal(got[y, z * n:(z + 1) * n, x * n:(x + 1) * n], before[y, z * n:(z + 1) * n, x * n:(x + 1) * n]), f"{name}, update {step}: probe {p} is left alone"


@pytest.mark.parametrize("name", list(BS.BLEND_CASES))
def test_blends_match_the_reference_on_both_sides_of_every_rule(dev, du, name):
    """Both blends from the case's ray records, update after update on what the device textures hold: after each, every word of
    the irradiance and of the distance texture equals the reference's, and the tiles of left-alone probes equal what they held."""
    c = BS.blend_case(du, name)
    u = Update(dev, c.vol)
    try:
        for step, (k, rays, want_irr, want_dist, rr, dr) in enumerate(c.steps):
            irr, dist = u.run_blends(k, rays)
            same(irr, want_irr, f"{name}, update {step}: irradiance")
            same(dist.view(np.uint16), want_dist.view(np.uint16), f"{name}, update {step}: distance")
            before = c.before(step)
            _left_alone_tiles_kept(name, step, c.vol, rr, 8, irr, before.irradiance)
            _left_alone_tiles_kept(name, step, c.vol, dr, 16, dist.view(np.uint16).view(np.uint32)[..., 0], np.ascontiguousarray(before.distance).view(np.uint16).view(np.uint32)[..., 0])
    finally:
        u.release()


@pytest.mark.parametrize("name", BS.TRACED)
def test_blends_behind_the_traces(dev, sm, du, name):
    """Three chained updates over the case's scene under a light of strength 8: the trace, then both blends of the trace's own
    records, on the device textures.  After each update the records, the irradiance and the distance equal DU.update's."""
    c = trace_case(sm, du, name)
    state = c.volume()
    gs = bare_gpu_scene(dev, c.sc)
    u = Update(dev, state, gs)
    try:
        for step in range(BS.TRACED_UPDATES):
            k = BS.traced_consts(name, step)
            got = u.run_trace(k)
            irr, dist = u.run_blends(k, got)
            want = DU.update(du, k, state, c.scene, np.full(got.shape, RAY_SENTINEL, F))
            same(got.view(np.uint32), want.view(np.uint32), f"{name}, update {step}: ray records")
            same(irr, state.irradiance, f"{name}, update {step}: irradiance")
            same(dist.view(np.uint16), state.distance.view(np.uint16), f"{name}, update {step}: distance")
    finally:
        u.release(); gs.release()
