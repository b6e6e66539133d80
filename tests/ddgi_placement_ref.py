"""ctypes wrapper of tests/ddgi_placement_ref.c, the definition of "giprobetrace_CS_ProbeTraceFixedRays",
"ProbeRelocationCS_DDGIProbeRelocationCS" and "ProbeClassificationCS_DDGIProbeClassificationCS" (csrc/k_giprobeplacement.hip).  The
library holds tests/ddgi_update_ref.c too, so one handle serves a whole update: ddgi_update_ref's functions take it as well.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C

import numpy as np

import ddgi_update_ref as DU
import shadowmask_ref as SR
from ref_build import compile_ref
from toyrenderer_amd import interop as I

F = np.float32
FIXED = I.kDDGIFixedRays
MISS_DISTANCE = F(1e27)
A_TAKEN, A_REFUSED, B_TAKEN, B_REFUSED, B_NO_FAR, C_TAKEN, C_REFUSED, C_ZERO_OFFSET, NO_MOVE = range(9)
ACTIVE, OFF_BACKFACES, OFF_NOTHING_NEAR = range(3)


def _declare(lib):
    DU._declare(lib)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.dp_fixed_direction.argtypes = [u32, vp]
    lib.dp_trace_fixed.argtypes = [vp, C.POINTER(SR._Scene), vp, C.c_int, vp]
    lib.dp_relocate.argtypes = [vp] * 4
    lib.dp_classify.argtypes = [vp] * 4
    lib.dp_round_trip.argtypes = [C.c_uint16, C.c_float]
    lib.dp_round_trip.restype = C.c_uint16
    for n in ("dp_fixed_direction", "dp_trace_fixed", "dp_relocate", "dp_classify"):
        getattr(lib, n).restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "ddgi_placement_ref", _declare)


def consts(min_frontface_distance=0.3, fixed_ray_backface_threshold=0.25, **kw) -> np.ndarray:
    """ddgi_update_ref.consts with the two placement fields (the reference's values for a scene radius of 3 or more)."""
    k = DU.consts(**kw)
    k["probeMinFrontfaceDistance"], k["probeFixedRayBackfaceThreshold"] = min_frontface_distance, fixed_ray_backface_threshold
    return k


def fixed_directions(lib) -> np.ndarray:
    out = np.zeros((FIXED, 3), F)
    for i in range(FIXED):
        lib.dp_fixed_direction(i, out[i].ctypes.data)
    return out


def trace_fixed(lib, k, vol, scene: DU.Scene, mode=DU.WALK) -> np.ndarray:
    """The fixed-ray trace: float32 [numProbes, 32]."""
    b = DU.block(k, vol)
    out = np.zeros((int(np.prod(vol.counts)), FIXED), F)
    lib.dp_trace_fixed(DU._p(b), C.byref(scene.c), DU._p(DU._data16(vol)), mode, DU._p(out))
    return out


def _placed(fn, k, vol, distances):
    b = DU.block(k, vol)
    n = int(np.prod(vol.counts))
    d = np.ascontiguousarray(distances, F)
    assert d.size == n * FIXED
    data, why = np.ascontiguousarray(vol.data, np.float16).copy(), np.zeros(n, np.uint32)
    fn(DU._p(b), DU._p(d), DU._p(data.view(np.uint16)), DU._p(why))
    return data, why


def relocate(lib, k, vol, distances):
    """(data float16 [cy, cz, cx, 4] after relocation, branch uint32 [numProbes]) from the volume's data and `distances`."""
    return _placed(lib.dp_relocate, k, vol, distances)


def classify(lib, k, vol, distances):
    """(data after classification, reason uint32 [numProbes])."""
    return _placed(lib.dp_classify, k, vol, distances)


def update(lib, k, vol, scene: DU.Scene, relocate_on=True, classify_on=True, rays_init=None):
    """One whole update of `vol` in place in the product's order: trace, both blends, fixed-ray trace, relocation, classification.
    Returns (ray records, fixed-ray distances)."""
    rays = DU.update(lib, k, vol, scene, rays_init)
    fixed = trace_fixed(lib, k, vol, scene)
    if relocate_on:
        vol.data, _ = relocate(lib, k, vol, fixed)
    if classify_on:
        vol.data, _ = classify(lib, k, vol, fixed)
    return rays, fixed
