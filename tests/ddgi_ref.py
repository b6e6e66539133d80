"""ctypes wrapper of tests/ddgi_ref.c, the test reference of the DDGI ambient term of "deferredlighting_PS_Main" and of debug
view 10 (csrc/ddgi_irradiance.hip.h), and a numpy float64 restatement of the query for the precision check.

The library is compiled by the test that needs it (gcc -O2 -ffp-contract=off) into a pytest temporary directory."""
import ctypes as C
import math

import numpy as np

from ref_build import compile_ref
from toyrenderer_amd import interop as I


Trace = np.dtype([("inside", np.uint32), ("base", np.int32, (3,)), ("evaluated", np.uint32), ("skipMask", np.uint32), ("chebMask", np.uint32),
                  ("crushMask", np.uint32), ("clampMask", np.uint32), ("relocMask", np.uint32), ("foldMask", np.uint32), ("blend", np.float32)])
COUNTERS = ("blend_one", "blend_partial", "blend_zero", "skipped_some", "skipped_all", "relocated", "cheb_taken", "cheb_not", "crush_taken", "crush_not",
            "fold_taken", "fold_not", "clamped")


def _declare(lib):
    vp = C.c_void_p
    lib.dg_lighting.argtypes = [vp, C.c_int] + [vp] * 14
    lib.dg_irradiance_n.argtypes = [vp] * 7 + [C.c_uint64, vp, vp]
    lib.dg_inputs.argtypes = [vp] * 6
    lib.dg_fetch_irradiance.argtypes = [vp] * 5
    lib.dg_fetch_distance.argtypes = [vp] * 5
    lib.dg_pow_n.argtypes = [vp, C.c_uint64, C.c_float, vp]
    lib.dg_oct_n.argtypes = [vp, C.c_uint64, vp]
    for n in ("dg_lighting", "dg_irradiance_n", "dg_inputs", "dg_fetch_irradiance", "dg_fetch_distance", "dg_pow_n", "dg_oct_n"):
        getattr(lib, n).restype = None


def load(tmpdir) -> C.CDLL:
    return compile_ref(tmpdir, "ddgi_ref", _declare)


def _p(a):
    return a.ctypes.data if a is not None else None


def _textures(vol):
    """The volume's arrays as the C side reads them (dense, slice-major)."""
    return (np.ascontiguousarray(vol.desc()), np.ascontiguousarray(vol.data).view(np.uint16), np.ascontiguousarray(vol.irradiance, np.uint32),
            np.ascontiguousarray(vol.distance).view(np.uint16))


def pow_soft(lib, x, e) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.empty(len(x), np.float32)
    lib.dg_pow_n(_p(x), len(x), float(e), _p(out))
    return out


def oct_encode(lib, d) -> np.ndarray:
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    out = np.empty((len(d), 2), np.float32)
    lib.dg_oct_n(_p(d), len(d), _p(out))
    return out


def fetch_irradiance(lib, vol, c, o) -> np.ndarray:
    d, _, irr, _ = _textures(vol)
    c, o, out = np.asarray(c, np.int32), np.asarray(o, np.float32), np.empty(3, np.float32)
    lib.dg_fetch_irradiance(_p(d), _p(irr), _p(c), _p(o), _p(out))
    return out


def fetch_distance(lib, vol, c, o) -> np.ndarray:
    d, _, _, dist = _textures(vol)
    c, o, out = np.asarray(c, np.int32), np.asarray(o, np.float32), np.empty(2, np.float32)
    lib.dg_fetch_distance(_p(d), _p(dist), _p(c), _p(o), _p(out))
    return out


def irradiance(lib, vol, world, normal, camera_origin):
    """The query at n points: (float32 [n, 3], Trace [n])."""
    d, data, irr, dist = _textures(vol)
    w = np.ascontiguousarray(world, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    cam = np.ascontiguousarray(camera_origin, np.float32)
    out, tr = np.zeros((len(w), 3), np.float32), np.zeros(len(w), Trace)
    lib.dg_irradiance_n(_p(d), _p(data), _p(irr), _p(dist), _p(w), _p(n), _p(cam), len(w), _p(out), _p(tr))
    return out, tr


def inputs(lib, k, gbuffer, depth):
    """(world, normal, albedo) float32 [H, W, 3] of every written pixel (NaN elsewhere)."""
    k = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(k).tobytes()[:112], I.DeferredLightingConsts))
    W, H = (int(x) for x in k["m_LightingOutputResolution"][0])
    g = np.ascontiguousarray(gbuffer, np.uint32).reshape(H, W, 4)
    d = np.ascontiguousarray(depth, np.float32).reshape(H, W)
    out = [np.full((H, W, 3), np.nan, np.float32) for _ in range(3)]
    lib.dg_inputs(_p(k), _p(g), _p(d), *[_p(o) for o in out])
    return out


def lighting(lib, k, vol, gbuffer, depth, *, debug=None, motion=None, ssao=None, shadow=None, out_init=None, want=()):
    """lighting_ref.lighting with the volume.  want: any of "rgb", "irr", "traces", "counters"; returns the uint32 [H, W] words,
    or (words, {name: array}) when something is wanted."""
    k = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(k).tobytes()[:112], I.DeferredLightingConsts))
    W, H = (int(x) for x in k["m_LightingOutputResolution"][0])
    dsc, data, irr, dist = _textures(vol)
    g = np.ascontiguousarray(gbuffer, np.uint32).reshape(H, W, 4)
    d = np.ascontiguousarray(depth, np.float32).reshape(H, W)
    if motion is not None:
        motion = np.ascontiguousarray(motion)
        motion = np.ascontiguousarray(motion.view(np.uint16).reshape(H, W, 2)).view(np.uint32).reshape(H, W) if motion.dtype != np.uint32 else motion.reshape(H, W)
    ssao = None if ssao is None else np.ascontiguousarray(ssao, np.uint8).reshape(H, W)
    shadow = None if shadow is None else np.ascontiguousarray(shadow, np.uint8).reshape(H, W)
    out = np.zeros((H, W), np.uint32) if out_init is None else np.ascontiguousarray(out_init, np.uint32).reshape(H, W).copy()
    extra = {}
    if "rgb" in want:
        extra["rgb"] = np.full((H, W, 3), np.nan, np.float32)
    if "irr" in want:
        extra["irr"] = np.full((H, W, 3), np.nan, np.float32)
    if "traces" in want:
        extra["traces"] = np.zeros((H, W), Trace)
    if "counters" in want:
        extra["counters"] = np.zeros(len(COUNTERS), np.uint64)
    is_debug = bool(k["m_DebugMode"][0] != 0) if debug is None else bool(debug)
    lib.dg_lighting(_p(k), int(is_debug), _p(dsc), _p(data), _p(irr), _p(dist), _p(g), _p(motion), _p(d), _p(ssao), _p(shadow), _p(out),
                    _p(extra.get("rgb")), _p(extra.get("irr")), _p(extra.get("traces")), _p(extra.get("counters")))
    if "counters" in extra:
        extra["counters"] = dict(zip(COUNTERS, (int(x) for x in extra["counters"])))
    return (out, extra) if want else out


# ---- the float64 restatement ----------------------------------------------------------------------------------------------
def _oct64(d):
    l1 = np.abs(d).sum(-1)
    u, v = d[..., 0] / l1, d[..., 1] / l1
    fold = d[..., 2] < 0
    s = lambda x: np.where(x >= 0, 1.0, -1.0)
    return np.where(fold, (1 - np.abs(v)) * s(u), u), np.where(fold, (1 - np.abs(u)) * s(v), v)


def _bilinear64(tex, sl, cx, cz, ou, ov, interior):
    """tex float64 [S, H, W, C]; per point slice sl, probe (cx, cz), octahedral (ou, ov)."""
    n = interior + 2
    H, W = tex.shape[1:3]
    tx = cx * n + n * 0.5 + ou * (interior * 0.5) - 0.5
    ty = cz * n + n * 0.5 + ov * (interior * 0.5) - 0.5
    x0, y0 = np.floor(tx), np.floor(ty)
    fx, fy = (tx - x0)[:, None], (ty - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    t = lambda x, y: tex[sl, y % H, x % W]
    top = t(x0, y0) + fx * (t(x0 + 1, y0) - t(x0, y0))
    bot = t(x0, y0 + 1) + fx * (t(x0 + 1, y0 + 1) - t(x0, y0 + 1))
    return top + fy * (bot - top)


def irradiance64(vol, world, normal, camera_origin):
    """The query in float64 from the same float32 inputs and texels.  Returns (irr float64 [n, 3], decisions): decisions holds
    what each point decided (inside, base, skip / Chebyshev / crush masks, evaluated) for the comparison with the C traces."""
    f8 = np.float64
    w, N, cam = np.asarray(world, np.float32).astype(f8).reshape(-1, 3), np.asarray(normal, np.float32).astype(f8).reshape(-1, 3), np.asarray(camera_origin, np.float32).astype(f8)
    n = len(w)
    origin, sp = np.asarray(vol.origin, np.float32).astype(f8), np.asarray(vol.spacing, np.float32).astype(f8)
    counts = np.asarray(vol.counts, np.int64)
    cx, cy, cz = vol.counts
    last = counts - 1
    ext = sp * last * 0.5
    nb, vb = f8(np.float32(vol.normal_bias)), f8(np.float32(vol.view_bias))
    half_gamma = f8(np.float32(vol.gamma)) * 0.5
    data = vol.data.astype(f8)
    irr = np.stack([((vol.irradiance >> s) & 1023).astype(f8) / 1023.0 for s in (0, 10, 20)], -1)
    dist = vol.distance.astype(f8)

    view = w - cam
    with np.errstate(all="ignore"):
        view = view / np.sqrt((view * view).sum(-1))[:, None]
    delta = np.abs(w - origin) - ext
    inside = (delta < 0).all(-1)
    blend = np.where(inside, 1.0, np.prod(1 - np.clip(delta / sp, 0, 1), -1))
    evaluated = blend > 0
    P = w + (N * nb - view * vb)
    base = np.clip(np.trunc(np.clip(np.nan_to_num((P - origin + ext) / sp, nan=0.0), 0, None)), 0, last).astype(np.int64)   # fmax drops a NaN

    def probe_pos(c):
        p = sp * c - ext + origin
        d = data[c[:, 1], c[:, 2], c[:, 0]]
        if vol.relocation:
            p = p + d[:, :3] * sp
        return p, d[:, 3]

    base_pos, _ = probe_pos(base)
    alpha = np.clip((P - base_pos) / sp, 0, 1)
    nu, nv = _oct64(N)
    total, wsum = np.zeros((n, 3)), np.zeros(n)
    skip = np.zeros(n, np.uint32)
    cheb = np.zeros(n, np.uint32)
    crush = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        for i in range(8):
            off = np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])
            c = np.minimum(base + off, last)
            pp, state = probe_pos(c)
            skipped = (state == 1.0) if vol.classification else np.zeros(n, bool)
            to_w, to_b = pp - w, pp - P
            dir_w = to_w / np.sqrt((to_w * to_w).sum(-1))[:, None]
            d_b = np.sqrt((to_b * to_b).sum(-1))
            tri = np.maximum(0.001, np.where(off == 1, alpha, 1 - alpha))
            wrap = ((dir_w * N).sum(-1) + 1) * 0.5
            wt = wrap * wrap + 0.2
            du, dv = _oct64(-to_b / d_b[:, None])
            m = 2 * _bilinear64(dist, c[:, 1], c[:, 0], c[:, 2], du, dv, I.kDDGIDistanceInteriorTexels)
            var = np.abs(m[:, 0] * m[:, 0] - m[:, 1])
            taken = d_b > m[:, 0]
            v = d_b - m[:, 0]
            ch = np.where(taken, np.maximum((var / (var + v * v)) ** 3, 0), 1.0)
            wt = np.maximum(0.000001, wt * np.maximum(0.05, ch))
            crushed = wt < 0.2
            wt = np.where(crushed, wt * wt * wt / (0.2 * 0.2), wt)
            wt = wt * tri.prod(-1)
            e = _bilinear64(irr, c[:, 1], c[:, 0], c[:, 2], nu, nv, I.kDDGIIrradianceInteriorTexels)
            e = np.where(e > 0, np.power(np.maximum(e, 1e-300), half_gamma), 0.0)
            live = ~skipped
            total += np.where(live[:, None], wt[:, None] * e, 0.0)
            wsum += np.where(live, wt, 0.0)
            skip |= skipped.astype(np.uint32) << np.uint32(i)
            cheb |= (taken & live).astype(np.uint32) << np.uint32(i)
            crush |= (crushed & live).astype(np.uint32) << np.uint32(i)
        r = total / np.where(wsum == 0, 1.0, wsum)[:, None]
        out = r * r * (2 * math.pi) * 1.0989 * blend[:, None]
    out = np.where((evaluated & (wsum != 0))[:, None], out, 0.0)
    return out, dict(inside=inside, base=base, evaluated=evaluated, skip=skip, cheb=cheb, crush=crush, blend=blend)
