"""ctypes wrapper of tests/ddgi_update_ref.c, the definition of "giprobetrace_CS_ProbeTrace" and of the two
"ProbeBlendingCS_DDGIProbeBlendingCS" passes (csrc/k_giprobetrace.hip, csrc/k_giprobeblend.hip, csrc/ray_walk.hip.h), and a numpy
float64 restatement of the two blends for the precision check.  blend_rules() also returns the rule the reference took at every
interior texel (du_blend_radiance_rules, du_blend_distance_rules: the R_* and D_* bits below).

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C
import math

import numpy as np

import shadowmask_ref as SR
from ref_build import compile_ref
from toyrenderer_amd import interop as I

F = np.float32
RAYS = I.kDDGIRaysPerProbe
BRUTE, WALK = 0, 1
MISS = 0xFFFFFFFF
Hit = np.dtype([("inst", np.uint32), ("tri", np.uint32), ("t", np.float32), ("b1", np.float32), ("b2", np.float32), ("front", np.uint32)])
KIND_MISS, KIND_BACK, KIND_LIT, KIND_SHADOWED = 0, 1, 2, 3
Block = np.dtype([("k", I.DDGIUpdateConsts), ("D", I.DDGIVolumeDesc)])
assert Block.itemsize == 160


def _declare(lib):
    vp, u32, u64, f = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    lib.du_ray_direction.argtypes = [vp, u32, vp]
    lib.du_oct_decode.argtypes = [f, f, vp]
    lib.du_texel_direction.argtypes = [u32, u32, u32, vp]
    lib.du_closest_n.argtypes = [C.POINTER(SR._Scene), vp, vp, u64, f, f, C.c_int, vp, vp]
    lib.du_trace.argtypes = [vp, C.POINTER(SR._Scene), vp, vp, vp, C.c_int, vp, vp]
    lib.du_probe_positions.argtypes = [vp, vp, vp, vp]
    lib.du_ease_radiance.argtypes = [vp, vp, vp, C.c_int, vp]
    lib.du_unorm10.argtypes = [f]
    lib.du_unorm10.restype = u32
    lib.du_blend_radiance.argtypes = [vp] * 4
    lib.du_blend_distance.argtypes = [vp] * 4
    lib.du_blend_radiance_rules.argtypes = [vp] * 5
    lib.du_blend_distance_rules.argtypes = [vp] * 5
    lib.dg_oct_n.argtypes = [vp, u64, vp]
    for n in ("du_ray_direction", "du_oct_decode", "du_texel_direction", "du_closest_n", "du_trace", "du_probe_positions", "du_ease_radiance", "du_blend_radiance",
              "du_blend_distance", "du_blend_radiance_rules", "du_blend_distance_rules", "dg_oct_n"):
        getattr(lib, n).restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "ddgi_update_ref", _declare)


def consts(light=((0.0, 1.0, 0.0), 1.0), rotation=None, max_ray_distance=1e10, hysteresis=0.5, distance_exponent=50.0, irradiance_threshold=0.2,
           brightness_threshold=0.1) -> np.ndarray:
    """One DDGIUpdateConsts; the defaults of GIRenderer.cpp:111-118."""
    k = np.zeros(1, I.DDGIUpdateConsts)
    k["m_DirectionalLightVector"], k["m_DirectionalLightStrength"] = light
    k["rayRotation"][0, :, :3] = np.eye(3, dtype=F) if rotation is None else np.asarray(rotation, F)
    k["probeMaxRayDistance"], k["probeHysteresis"], k["probeDistanceExponent"] = max_ray_distance, hysteresis, distance_exponent
    k["probeIrradianceThreshold"], k["probeBrightnessThreshold"] = irradiance_threshold, brightness_threshold
    return k


def block(k, vol) -> np.ndarray:
    """b0 of the three passes: the constants, then the volume's descriptor."""
    b = np.zeros(1, Block)
    b["k"], b["D"] = np.ascontiguousarray(k, I.DDGIUpdateConsts)[0], vol.desc()[0]
    return b


def _p(a):
    return a.ctypes.data if a is not None else None


def _data16(vol):
    return np.ascontiguousarray(vol.data).view(np.uint16)


class Scene:
    """The arrays of one scene dict and its acceleration structure (shadowmask_ref.Accel) as the C side reads them; the TLAS is
    refitted to `instances` (default: the scene's own), as the frame refits it before the trace."""

    def __init__(self, sm_lib, acc: SR.Accel, instances=None):
        sc = acc.scene
        inst = np.ascontiguousarray(sc["instances"] if instances is None else instances, I.BasePassInstanceConstants)
        nodes, records = SR.refit(sm_lib, acc, inst)
        self.acc, self.nodes, self.records = acc, nodes, records
        self.keep = [inst, np.ascontiguousarray(acc.flags, np.uint32), np.ascontiguousarray(sc["vertices"], I.RawVertexFormat), np.ascontiguousarray(sc["materials"], I.MaterialData),
                     np.ascontiguousarray(sc["indices"], np.uint32), np.ascontiguousarray(sc["meshData"], I.MeshData), np.ascontiguousarray(acc.blas["index_counts"], np.uint32),
                     np.ascontiguousarray(nodes, I.AccelNode), np.ascontiguousarray(records, I.TLASInstance), np.ascontiguousarray(acc.blas["headers"]),
                     np.ascontiguousarray(acc.blas["nodes"]), np.ascontiguousarray(acc.blas["tri_order"], np.uint32)]
        p = [a.ctypes.data for a in self.keep]
        k = self.keep
        self.c = SR._Scene(p[0], p[1], len(k[0]), p[2], len(k[2]), p[3], len(k[3]), p[4], len(k[4]), p[5], p[6], len(k[5]), p[7], len(k[7]), p[8], p[9], p[10], len(k[10]),
                           p[11], len(k[11]))
        self.num_triangles = int(sum(int(acc.blas["index_counts"][int(m)]) // 3 for m in inst["m_MeshDataIdx"]))


def ray_directions(lib, k) -> np.ndarray:
    k = np.ascontiguousarray(k, I.DDGIUpdateConsts)
    out = np.zeros((RAYS, 3), F)
    for i in range(RAYS):
        lib.du_ray_direction(_p(k), i, out[i].ctypes.data)
    return out


def texel_directions(lib, interior: int) -> np.ndarray:
    out = np.zeros((interior, interior, 3), F)
    for y in range(interior):
        for x in range(interior):
            lib.du_texel_direction(x, y, interior, out[y, x].ctypes.data)
    return out


def closest(lib, scene: Scene, origins, directions, mode, tmin=0.0, tmax=1e10):
    """(Hit [n], ties): the closest hit of n rays; ties counts the equal-t decisions brute force met."""
    o = np.ascontiguousarray(origins, F).reshape(-1, 3)
    d = np.ascontiguousarray(np.broadcast_to(np.asarray(directions, F), o.shape) if np.ndim(directions) == 1 else directions, F).reshape(-1, 3)
    out, ties = np.zeros(len(o), Hit), np.zeros(1, np.uint64)
    lib.du_closest_n(C.byref(scene.c), _p(o), _p(d), len(o), float(tmin), float(tmax), mode, _p(out), _p(ties))
    return out, int(ties[0])


def probe_positions(lib, vol):
    """(positions float32 [n, 3], inactive bool [n]) in probe-index order."""
    d, data = np.ascontiguousarray(vol.desc()), _data16(vol)
    n = int(np.prod(vol.counts))
    pos, inactive = np.zeros((n, 3), F), np.zeros(n, np.uint32)
    lib.du_probe_positions(_p(d), _p(data), _p(pos), _p(inactive))
    return pos, inactive.astype(bool)


def trace(lib, k, vol, scene: Scene, mode=WALK, rays_init=None):
    """The trace: (records float32 [numProbes, 256, 4], kinds uint32 [numProbes, 256]).  rays_init: what the buffer held."""
    b = block(k, vol)
    n = int(np.prod(vol.counts))
    rays = np.zeros((n, RAYS, 4), F) if rays_init is None else np.ascontiguousarray(rays_init, F).reshape(n, RAYS, 4).copy()
    kinds = np.full((n, RAYS), 0xFF, np.uint32)
    data, irr, dist = _data16(vol), np.ascontiguousarray(vol.irradiance, np.uint32), np.ascontiguousarray(vol.distance).view(np.uint16)
    lib.du_trace(_p(b), C.byref(scene.c), _p(data), _p(irr), _p(dist), mode, _p(rays), _p(kinds))
    return rays, kinds


def blend(lib, k, vol, rays):
    """Both blends of `rays` ([numProbes, 256, 4]) into copies of the volume's textures: (irradiance uint32, distance float16)."""
    b = block(k, vol)
    rays = np.ascontiguousarray(rays, F)
    assert rays.size == int(np.prod(vol.counts)) * RAYS * 4
    irr, dist = np.ascontiguousarray(vol.irradiance, np.uint32).copy(), np.ascontiguousarray(vol.distance, np.float16).copy()
    data = _data16(vol)
    lib.du_blend_radiance(_p(b), _p(data), _p(rays), _p(irr))
    lib.du_blend_distance(_p(b), _p(data), _p(rays), _p(dist.view(np.uint16)))
    return irr, dist


# the rule bits of du_blend_radiance_rules and du_blend_distance_rules (tests/ddgi_update_ref.c: DU_R_*, DU_D_*); the per-channel
# ones are shifted left by the channel
R_LEFT_ALONE, R_PREV_ZERO, R_IRRADIANCE, R_BRIGHTNESS, R_DARKER = 1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4
R_FLOOR, R_CAP, R_SIGN_ZERO, R_CLAMP_ONE, R_CLAMP_ZERO = 1 << 5, 1 << 8, 1 << 11, 1 << 14, 1 << 17
R_NAN, R_MAX_SHIFT, R_SUM_NAN = 1 << 20, 21, 1 << 23
D_LEFT_ALONE, D_PREV_ZERO, D_SUMW_FLOOR, D_STORE_INF, D_STORE_NAN, D_STORE_SUBNORMAL, D_PREV_INF, D_PREV_NAN = (1 << i for i in range(8))
D_CLIPPED_SHIFT = 16


def any_channel(bit):
    return bit | bit << 1 | bit << 2


def blend_rules(lib, k, vol, rays):
    """blend(), and the rule the reference took at every interior texel: (irradiance, distance, radiance rules uint32
    [numProbes, 6, 6], distance rules uint32 [numProbes, 14, 14]).  The same function bodies: the textures equal blend()'s."""
    b = block(k, vol)
    rays = np.ascontiguousarray(rays, F)
    n = int(np.prod(vol.counts))
    assert rays.size == n * RAYS * 4
    irr, dist = np.ascontiguousarray(vol.irradiance, np.uint32).copy(), np.ascontiguousarray(vol.distance, np.float16).copy()
    rr, dr = np.full((n, 6, 6), 0xFFFFFFFF, np.uint32), np.full((n, 14, 14), 0xFFFFFFFF, np.uint32)
    data = _data16(vol)
    lib.du_blend_radiance_rules(_p(b), _p(data), _p(rays), _p(irr), _p(rr))
    lib.du_blend_distance_rules(_p(b), _p(data), _p(rays), _p(dist.view(np.uint16)), _p(dr))
    return irr, dist, rr, dr


def update(lib, k, vol, scene: Scene, rays_init=None):
    """One whole update of `vol` in place (trace, then both blends); returns the ray records."""
    rays, _ = trace(lib, k, vol, scene, WALK, rays_init)
    vol.irradiance, vol.distance = blend(lib, k, vol, rays)
    return rays


def ease_radiance(lib, k, res, prev, floor_rule=True) -> np.ndarray:
    k = np.ascontiguousarray(k, I.DDGIUpdateConsts)
    res, prev, out = np.ascontiguousarray(res, F), np.ascontiguousarray(prev, F), np.zeros(3, F)
    lib.du_ease_radiance(_p(k), _p(res), _p(prev), int(floor_rule), _p(out))
    return out


# ---- the float64 restatement of the two blends -------------------------------------------------------------------------------
def blend64(lib, k, vol, rays, decisions=False):
    """The two blends in float64 from the same float32 inputs (ray records, ray and texel directions as the reference rounds them,
    the previous texels): (irradiance codes float64 [.., 3] before rounding, distance float64 [.., 2] before rounding, touched
    bool per probe).  Texels of probes that are left alone hold NaN.  decisions=True adds two arrays of the irradiance texture's
    shape: the R_IRRADIANCE | R_BRIGHTNESS bits as float64 decides them (uint32), and how far the nearer of the two compared
    quantities is from its threshold (float64; inf where prev == 0 decides nothing)."""
    f8 = np.float64
    k = np.ascontiguousarray(k, I.DDGIUpdateConsts)
    cx, cy, cz = vol.counts
    n = cx * cy * cz
    rays = np.asarray(rays, F).reshape(n, RAYS, 4).astype(f8)
    dirs = ray_directions(lib, k).astype(f8)
    h0 = f8(k["probeHysteresis"][0])
    thr_i, thr_b, expo = f8(k["probeIrradianceThreshold"][0]), f8(k["probeBrightnessThreshold"][0]), f8(k["probeDistanceExponent"][0])
    inv_gamma = 1.0 / f8(F(vol.gamma))
    sp = np.asarray(vol.spacing, F).astype(f8)
    max_d = 1.5 * math.sqrt(float((sp * sp).sum()))
    _, inactive = probe_positions(lib, vol)
    irr_out = np.full(vol.irradiance.shape + (3,), np.nan)
    dist_out = np.full(vol.distance.shape, np.nan)
    taken, margin = np.zeros(vol.irradiance.shape, np.uint32), np.full(vol.irradiance.shape, np.inf)
    touched = np.zeros(n, bool)
    t6, t14 = texel_directions(lib, 6).astype(f8), texel_directions(lib, 14).astype(f8)
    for p in range(n):
        x, y, z = p % cx, p // (cx * cz), (p // cx) % cz
        rec = rays[p]
        if inactive[p] or np.count_nonzero(rec[:, 3] < 0) >= I.kDDGIBackfaceRayLimit:
            continue
        touched[p] = True
        # radiance
        w = np.maximum(0.0, t6 @ dirs.T)                                     # [6, 6, 256]
        w = np.where(rec[:, 3] < 0, 0.0, w)
        s = (w[..., None] * rec[None, None, :, :3]).sum(2)
        res = s / (2 * np.maximum(w.sum(2), 1e-9 * 256))[..., None]
        res = np.where(res > 0, np.power(np.maximum(res, 1e-300), inv_gamma), 0.0)
        old = vol.irradiance[y, z * 8 + 1:z * 8 + 7, x * 8 + 1:x * 8 + 7]
        prev = np.stack([((old >> s_) & 1023).astype(f8) / 1023.0 for s_ in (0, 10, 20)], -1)
        delta = res - prev
        h = np.where(np.abs(delta).max(-1) > thr_i, max(0.0, h0 - 0.75), h0)
        length = np.sqrt((delta * delta).sum(-1))
        eased = ~(prev == 0).all(-1)
        with np.errstate(invalid="ignore"):
            near = np.minimum(np.abs(np.abs(delta).max(-1) - thr_i), np.abs(length - thr_b))
        taken[y, z * 8 + 1:z * 8 + 7, x * 8 + 1:x * 8 + 7] = np.where(eased, (np.abs(delta).max(-1) > thr_i) * R_IRRADIANCE | (length > thr_b) * R_BRIGHTNESS, 0)
        margin[y, z * 8 + 1:z * 8 + 7, x * 8 + 1:x * 8 + 7] = np.where(eased, np.nan_to_num(near, nan=np.inf), np.inf)
        delta = np.where((length > thr_b)[..., None], delta * 0.25, delta)
        step = (1 - h)[..., None] * delta
        darker = (prev + delta).max(-1) < prev.max(-1)
        floored = np.minimum(np.maximum(1.0 / 1024.0, np.abs(step)), np.abs(delta)) * np.sign(step)
        step = np.where(darker[..., None], floored, step)
        out = np.where((prev == 0).all(-1)[..., None], res, prev + step)
        irr_out[y, z * 8 + 1:z * 8 + 7, x * 8 + 1:x * 8 + 7] = np.clip(out, 0, 1) * 1023.0
        # distance
        c = np.maximum(0.0, t14 @ dirs.T)
        w = np.where(c > 0, np.power(np.maximum(c, 1e-300), expo), 0.0)
        d = np.minimum(np.abs(rec[:, 3]), max_d)
        den = 2 * np.maximum(w.sum(2), 1e-9 * 256)
        r = np.stack([(w * d).sum(2) / den, (w * d * d).sum(2) / den], -1)
        oldd = vol.distance[y, z * 16 + 1:z * 16 + 15, x * 16 + 1:x * 16 + 15].astype(f8)
        hd = np.where((oldd == 0).all(-1), 0.0, h0)[..., None]
        dist_out[y, z * 16 + 1:z * 16 + 15, x * 16 + 1:x * 16 + 15] = r + hd * (oldd - r)
    return (irr_out, dist_out, touched, taken, margin) if decisions else (irr_out, dist_out, touched)


def interior_mask(shape_hw, n):
    """bool [H, W]: the interior texels of the n-square tiles."""
    H, W = shape_hw
    yy, xx = np.arange(H) % n, np.arange(W) % n
    return ((yy >= 1) & (yy <= n - 2))[:, None] & ((xx >= 1) & (xx <= n - 2))[None, :]


def seeded_volume(vol, seed, inactive=()):
    """Fills `vol` in place with seeded irradiance codes and distances (borders filled from the interior) and marks the probes of
    `inactive` (probe indices) as state 1; returns vol."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1024, vol.irradiance.shape + (3,), dtype=np.uint32)
    vol.irradiance[...] = q[..., 0] | q[..., 1] << np.uint32(10) | q[..., 2] << np.uint32(20) | np.uint32(3 << 30)
    mean = rng.uniform(0.05, 1.5, vol.distance.shape[:-1])
    vol.distance[..., 0] = mean.astype(np.float16)
    vol.distance[..., 1] = (mean * mean * rng.uniform(1.0, 1.3, mean.shape)).astype(np.float16)
    cx, cy, cz = vol.counts
    for p in inactive:
        vol.data[p // (cx * cz), (p // cx) % cz, p % cx, 3] = 1.0
    return vol.fill_borders()


def unpack10(words):
    w = np.asarray(words, np.uint32)
    return np.stack([(w >> np.uint32(s)) & np.uint32(1023) for s in (0, 10, 20)], -1).astype(np.int64)

