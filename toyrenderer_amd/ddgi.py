"""The DDGI probe volume the deferred lighting pass consumes (csrc/ddgi_irradiance.hip.h): descriptor, the three probe
textures as numpy arrays, and the helpers a caller needs to fill them.

A Volume is filled by the caller (an engine's probe update, a bake, or Volume.uniform for a constant ambient) or by the
project's own probe update (FrameDriver(ddgi=volume, ddgi_update={...}): "giprobetrace_CS_ProbeTrace" and the two
"ProbeBlendingCS_DDGIProbeBlendingCS" passes; csrc/k_giprobetrace.hip, csrc/k_giprobeblend.hip), which starts from the volume's arrays
(Volume.reset() for the reference's cleared start).  With ddgi_update=dict(relocate=True, classify=True) the update also moves the
probes off the geometry and switches off the ones that light nothing: it rewrites `data` (csrc/k_giprobeplacement.hip).  Layout, coordinate system 0 (left-handed, Y up):
  irradiance  uint32 [counts.y, counts.z * 8, counts.x * 8]       R10G10B10A2_UNORM words, probe (x, y, z)'s tile at [y, z * 8, x * 8]
  distance    float16 [counts.y, counts.z * 16, counts.x * 16, 2]  (mean distance / 2, mean squared distance / 2)
  data        float16 [counts.y, counts.z, counts.x, 4]            xyz relocation offset in units of the spacing, w state (1 = inactive)
"""
from __future__ import annotations

import math

import numpy as np

from . import interop as I
from . import rhi
from .rhi import CB, PUSH, SAMPLER, SRV, TEX_SRV, TEX_UAV, UAV

VARIABILITY_OFF = "probe variability is off (ddgi_update without variability=True)"
PROBES_OFF = "the probe visualisation is off (probes=None)"
IRRADIANCE_TEXELS = I.kDDGIIrradianceInteriorTexels + 2     # 8: kNumProbeRadianceTexels (GIRenderer.cpp)
DISTANCE_TEXELS = I.kDDGIDistanceInteriorTexels + 2         # 16: kNumProbeDistanceTexels
ENERGY_LOSS = np.float32(1.0989)                            # the 10-bit format's energy loss, multiplied back by the query
DEFAULT_GAMMA = 5.0                                         # probeIrradianceEncodingGamma (GIRenderer.cpp:119)
DEFAULT_SPACING = (1.0, 1.0, 1.0)                           # m_ProbeSpacing (GIRenderer.cpp:215)


def fill_borders(tiles: np.ndarray, interior: int) -> np.ndarray:
    """Fills the one-texel border of every (interior + 2)-square octahedral tile of `tiles` ([..., H, W] or, with a trailing
    channel axis of 2 or 4, [..., H, W, C]; H and W multiples of N = interior + 2) in place from its interior, so that a bilinear
    fetch across a tile's edge continues on the octahedron: rows and columns mirror, (x, 0) <- (N-1-x, 1), (x, N-1) <-
    (N-1-x, N-2), (0, y) <- (1, N-1-y), (N-1, y) <- (N-2, N-1-y) for 1 <= x, y <= N-2, and each corner copies the diagonally
    opposite interior corner.  Returns tiles."""
    n = interior + 2
    t = tiles
    chan = t.ndim >= 3 and t.shape[-1] in (2, 4)        # a width is a multiple of n >= 8, so 2 or 4 is a channel axis
    hw = t.shape[-3:-1] if chan else t.shape[-2:]
    if hw[0] % n or hw[1] % n:
        raise ValueError(f"fill_borders: {hw[1]} x {hw[0]} texels are no whole number of {n} x {n} tiles")
    v = t if chan else t[..., None]
    lead = v.shape[:-3]
    # [..., tileY, y, tileX, x, C]: a view, so the assignments below write into `tiles`
    v = v.reshape(lead + (hw[0] // n, n, hw[1] // n, n, v.shape[-1]))
    inner = slice(1, n - 1)
    rev = slice(n - 2, 0, -1)
    v[..., 0, :, inner, :] = v[..., 1, :, rev, :]
    v[..., n - 1, :, inner, :] = v[..., n - 2, :, rev, :]
    v[..., inner, :, 0, :] = v[..., rev, :, 1, :]
    v[..., inner, :, n - 1, :] = v[..., rev, :, n - 2, :]
    v[..., 0, :, 0, :] = v[..., n - 2, :, n - 2, :]
    v[..., 0, :, n - 1, :] = v[..., n - 2, :, 1, :]
    v[..., n - 1, :, 0, :] = v[..., 1, :, n - 2, :]
    v[..., n - 1, :, n - 1, :] = v[..., 1, :, 1, :]
    return tiles


def encode_irradiance(linear_rgb, gamma: float = DEFAULT_GAMMA) -> np.ndarray:
    """The R10G10B10A2_UNORM word (alpha 3) whose decode -- the query squares pow(texel, gamma / 2) and multiplies by 2 pi and
    by 1.0989 -- gives back linear_rgb ([..., 3], irradiance), up to the 10 bits: texel = (rgb / (2 pi * 1.0989)) ^ (1 / gamma),
    saturated and rounded to nearest."""
    rgb = np.asarray(linear_rgb, np.float64)
    t = np.clip(np.maximum(rgb, 0.0) / (2.0 * math.pi * float(ENERGY_LOSS)), 0.0, 1.0) ** (1.0 / float(gamma))
    q = np.rint(t * 1023.0).astype(np.uint32)
    return q[..., 0] | q[..., 1] << np.uint32(10) | q[..., 2] << np.uint32(20) | np.uint32(3 << 30)


def pack_unorm10(texels) -> np.ndarray:
    """[..., 3] stored values in [0, 1] -> R10G10B10A2_UNORM words (alpha 3), rounded to nearest."""
    q = np.rint(np.clip(np.asarray(texels, np.float64), 0.0, 1.0) * 1023.0).astype(np.uint32)
    return q[..., 0] | q[..., 1] << np.uint32(10) | q[..., 2] << np.uint32(20) | np.uint32(3 << 30)


def random_rotation(rng) -> np.ndarray:
    """A uniformly distributed rotation, float32 [3, 3], from rng (a numpy Generator): the unit quaternion of four normal draws.
    Its rows are what DDGIUpdateConsts.rayRotation takes: a ray's direction becomes (row0 . d, row1 . d, row2 . d)."""
    q = rng.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float32)


UPDATE_DEFAULTS = dict(seed=0, hysteresis=0.5, distance_exponent=50.0, irradiance_threshold=0.2, brightness_threshold=0.1,     # GIRenderer.cpp:111-118
                       max_ray_distance=1e10,                                                                                # :79 passes the scene's bounding radius
                       relocate=False, classify=False,                # :80-83 switches both on; here they are options
                       min_frontface_distance=0.3,                    # :98, :106: 0.1 for a scene radius below 3, else 0.3
                       fixed_ray_backface_threshold=0.25,             # :121
                       variability=False,                             # :84 switches it on; here it is an option
                       variability_threshold=0.001)                   # :211 m_VariabilityStdDevThreshold


def check_update_settings(settings) -> dict:
    """The probe update's settings with the defaults filled in (UPDATE_DEFAULTS); an unknown key or a value out of range raises."""
    u = dict(UPDATE_DEFAULTS)
    unknown = set(settings) - set(u)
    if unknown:
        raise ValueError(f"ddgi_update: unknown settings {sorted(unknown)}; known: {sorted(u)}")
    u.update(settings)
    u["seed"] = int(u["seed"])
    if u["seed"] < 0:
        raise ValueError("ddgi_update: seed must not be negative")
    u["relocate"], u["classify"], u["variability"] = bool(u["relocate"]), bool(u["classify"]), bool(u["variability"])
    for name in ("hysteresis", "distance_exponent", "irradiance_threshold", "brightness_threshold", "max_ray_distance", "min_frontface_distance",
                 "fixed_ray_backface_threshold", "variability_threshold"):
        u[name] = float(u[name])
        if not (math.isfinite(u[name]) and u[name] >= 0.0):
            raise ValueError(f"ddgi_update: {name} = {u[name]} is not finite and >= 0")
    for name in ("hysteresis", "fixed_ray_backface_threshold"):
        if u[name] > 1.0:
            raise ValueError(f"ddgi_update: {name} = {u[name]} is not in [0, 1]")
    return u


class VariabilityTracker:
    """RTDDGIVolume::Update and SetVariabilityForCurrentFrame (GIRenderer.cpp:158-190) in numpy float32: csrc/host/DDGIVariability.h
    restated, bit for bit.  A ring of the last 16 volume-average variabilities; update() advances the cursor (converged or not),
    takes mean and variance / 16 over the ring in index order, stddev = sqrt(variance / 16) and converged = enabled and
    (samples++ > 16) and stddev < threshold: the 18th update at the earliest.  set() stores 0 for a value that is not normal
    (0, a denormal, inf, NaN).  Nothing wakes a converged tracker but reset(), which re-initialises everything but the switch and the
    threshold."""
    SAMPLES = I.kDDGIMinimumVariabilitySamples

    def __init__(self, threshold: float = 0.001, enabled: bool = True):
        self.threshold, self.enabled = np.float32(threshold), bool(enabled)
        self.reset()

    def reset(self):
        self.ring = np.zeros(self.SAMPLES, np.float32)
        self.cursor, self.samples = 0, 0
        self.average, self.stddev, self.converged = np.float32(0.0), np.float32(1e10), False

    def update(self) -> bool:
        f = np.float32
        self.cursor = (self.cursor + 1) % self.SAMPLES
        total = f(0.0)
        for v in self.ring:
            total = f(total + v)
        mean = f(total / f(self.SAMPLES))
        variance = f(0.0)
        for v in self.ring:
            diff = f(v - mean)
            variance = f(variance + f(diff * diff))
        self.stddev = f(np.sqrt(f(variance / f(self.SAMPLES))))
        self.converged = False
        if self.enabled:
            n = self.samples
            self.samples += 1
            self.converged = bool(n > self.SAMPLES and self.stddev < self.threshold)
        return self.converged

    def set(self, v):
        v = np.float32(v)
        tiny = np.finfo(np.float32).tiny
        self.average = v
        self.ring[self.cursor] = v if (np.isfinite(v) and abs(v) >= tiny) else np.float32(0.0)

    @classmethod
    def run(cls, averages, threshold: float = 0.001):
        """(converged bool [n], stddev float32 [n]) after each update() over a sequence, as trhost_ddgi_variability_run runs it:
        per element one update() and, unless it found the ring converged, one set()."""
        t = cls(threshold)
        conv, dev = [], []
        for a in np.asarray(averages, np.float32):
            conv.append(t.update())
            dev.append(t.stddev)
            if not t.converged:
                t.set(a)
        return np.asarray(conv, bool), np.asarray(dev, np.float32)


def unit_sphere():
    """The unit sphere the probe visualisation draws (CommonResources.cpp:40-102, tessellation 6, winding reversed): (vertices
    UncompressedRawVertexFormat [91], indices uint32 [468]).  Every angle is a multiple of pi / 6, so the sines are exactly 0, 1/2,
    RN(sqrt(3) / 2) and 1 with the quadrant's sign: no libm, and the poles and the seam column are exactly degenerate (120 of the 156
    triangles have area).  Byte for byte csrc/host/CommonResources.cpp's UnitSphere and tests/ddgi_probe_draw_ref.c's table."""
    f = np.float32
    r = f(float.fromhex("0x1.bb67aep-1"))                                  # RN(sqrt(3) / 2)
    s = np.array([0.0, 0.5, r, 1.0, r, 0.5, 0.0, -0.5, -r, -1.0, -r, -0.5], f)
    v = np.zeros(I.kUnitSphereVertices, I.UncompressedRawVertexFormat)
    for i in range(7):
        dy, dxz = s[(i + 9) % 12], s[i]
        for j in range(13):
            n = np.array([s[j % 12] * dxz, dy, s[(j + 3) % 12] * dxz], f)
            v[i * 13 + j] = (n * f(0.5), n, (f(1.0) - f(j) / f(12.0), f(1.0) - f(i) / f(6.0)))
    ix = []
    for i in range(6):
        for j in range(13):
            n = (j + 1) % 13
            ix += [i * 13 + n, (i + 1) * 13 + j, i * 13 + j, (i + 1) * 13 + n, (i + 1) * 13 + j, i * 13 + n]
    return v, np.asarray(ix, np.uint32)


class Volume:
    def __init__(self, origin, spacing, counts, normal_bias: float, view_bias: float, gamma: float = DEFAULT_GAMMA, relocation: bool = True,
                 classification: bool = True, variability: bool = False):
        self.origin = tuple(float(np.float32(x)) for x in origin)
        self.spacing = tuple(float(np.float32(x)) for x in spacing)
        self.counts = tuple(int(x) for x in counts)
        if len(self.origin) != 3 or len(self.spacing) != 3 or len(self.counts) != 3:
            raise ValueError("Volume: origin, spacing and counts have three components")
        if not all(1 <= c <= I.kDDGIMaxProbeCount for c in self.counts):
            raise ValueError(f"Volume: probe counts {self.counts} not in 1..{I.kDDGIMaxProbeCount}")
        if not all(math.isfinite(s) and s > 0.0 for s in self.spacing):
            raise ValueError(f"Volume: probe spacing {self.spacing} is not positive and finite")
        self.normal_bias, self.view_bias, self.gamma = float(normal_bias), float(view_bias), float(gamma)
        self.relocation, self.classification = bool(relocation), bool(classification)
        self.variability = bool(variability)         # flags bit 2: FrameDriver(ddgi_update=dict(variability=True)) sets it, with the buffer the bit needs
        cx, cy, cz = self.counts
        self.irradiance = np.zeros((cy, cz * IRRADIANCE_TEXELS, cx * IRRADIANCE_TEXELS), np.uint32)
        self.distance = np.zeros((cy, cz * DISTANCE_TEXELS, cx * DISTANCE_TEXELS, 2), np.float16)
        self.data = np.zeros((cy, cz, cx, 4), np.float16)

    @classmethod
    def for_scene(cls, aabb_center, aabb_extents, radius: float, spacing=DEFAULT_SPACING, **kw) -> "Volume":
        """GIRenderer.cpp:50-108: spacing at most a fifth of the padded (x 1.1) half extents and at least extents / 64, counts
        ceil(2 * extents / spacing), the origin the box's centre, the sample's biases by the scene's bounding radius."""
        f = np.float32
        ext = np.asarray(aabb_extents, f)
        sp = np.minimum(np.asarray(spacing, f), (ext * f(1.1)) * f(0.2))
        sp = np.maximum(sp, ext / f(64.0))
        counts = tuple(int(math.ceil(float(ext[a] * f(2.0) / sp[a]))) for a in range(3))
        view_bias, normal_bias = (0.1, 0.02) if float(radius) < 3.0 else (0.3, 0.1)
        return cls(aabb_center, sp, counts, normal_bias, view_bias, **kw)

    @classmethod
    def uniform(cls, origin, spacing, counts, normal_bias: float = 0.1, view_bias: float = 0.3, gamma: float = DEFAULT_GAMMA, irradiance=(1.0, 1.0, 1.0),
                max_distance: float = 32000.0) -> "Volume":
        """A volume whose every probe stores the same irradiance and sees nothing nearer than max_distance: a constant ambient
        term (faded out over one spacing beyond the outermost probes) for a caller without a probe generator."""
        v = cls(origin, spacing, counts, normal_bias, view_bias, gamma, relocation=False, classification=False)
        v.irradiance[...] = encode_irradiance(np.asarray(irradiance, np.float64), gamma)
        d = np.float16(max_distance * 0.5)
        v.distance[..., 0] = d
        v.distance[..., 1] = np.float16(min(float(d) * float(d) * 2.0, 65504.0))
        return v

    def reset(self) -> "Volume":
        """Irradiance and distance cleared to zero words, as GIRenderer.cpp:457-458 clears them before the first update (the probe
        data stays).  Returns self."""
        self.irradiance[...] = 0
        self.distance[...] = 0
        return self

    def copy(self) -> "Volume":
        v = Volume(self.origin, self.spacing, self.counts, self.normal_bias, self.view_bias, self.gamma, self.relocation, self.classification, self.variability)
        v.irradiance, v.distance, v.data = self.irradiance.copy(), self.distance.copy(), self.data.copy()
        return v

    def fill_borders(self) -> "Volume":
        fill_borders(self.irradiance, I.kDDGIIrradianceInteriorTexels)
        fill_borders(self.distance, I.kDDGIDistanceInteriorTexels)
        return self

    def desc(self) -> np.ndarray:
        """The 64-byte DDGIVolumeDesc (1 element)."""
        d = np.zeros(1, I.DDGIVolumeDesc)
        d["origin"], d["probeSpacing"], d["probeCounts"] = self.origin, self.spacing, self.counts
        d["probeNormalBias"], d["probeViewBias"], d["probeIrradianceEncodingGamma"] = self.normal_bias, self.view_bias, self.gamma
        d["numIrradianceInteriorTexels"], d["numDistanceInteriorTexels"] = I.kDDGIIrradianceInteriorTexels, I.kDDGIDistanceInteriorTexels
        d["flags"] = ((I.kDDGIFlag_Relocation if self.relocation else 0) | (I.kDDGIFlag_Classification if self.classification else 0) |
                      (I.kDDGIFlag_Variability if self.variability else 0))
        return d

    def probe_positions_and_states(self):
        """(positions float32 [n, 3], states float32 [n]) in probe-index order (index = y * counts.x * counts.z + x + counts.x * z),
        the layout Renderer.load_gi_probes / "giprobevisualization_CS_VisualizeGIProbesCulling" take; relocation applied when on.
        Evaluated as the query evaluates probePos, in float32."""
        f = np.float32
        cx, cy, cz = self.counts
        sp, org = np.asarray(self.spacing, f), np.asarray(self.origin, f)
        ext = (sp * np.asarray([cx - 1, cy - 1, cz - 1], f)) * f(0.5)
        y, z, x = np.meshgrid(np.arange(cy), np.arange(cz), np.arange(cx), indexing="ij")
        c = np.stack([x, y, z], -1).astype(f)
        pos = (sp * c - ext) + org
        if self.relocation:
            pos = pos + self.data[..., :3].astype(f) * sp
        return np.ascontiguousarray(pos.reshape(-1, 3), f), np.ascontiguousarray(self.data[..., 3].astype(f).reshape(-1))

    # ---- device side ---------------------------------------------------------------------------------------------------
    def upload(self, dev, uav: bool = False, data_uav: bool = False):
        """Creates and fills the descriptor buffer and the three array textures: (desc, data, irradiance, distance), what the
        lighting pass binds at t5..t8.  uav: the irradiance and distance textures get the UAV bit, which the two probe blends
        need to write them; data_uav: the data texture gets it, which probe relocation and classification need.  The caller
        releases them."""
        cx, cy, cz = self.counts
        desc = dev.buffer_from(self.desc().view(np.uint8), "DDGI Volume Desc", uav=False)
        data = dev.create_texture_array(cx, cz, cy, rhi.FORMAT_RGBA16_FLOAT, "DDGI Probe Data", uav=data_uav)
        irr = dev.create_texture_array(cx * IRRADIANCE_TEXELS, cz * IRRADIANCE_TEXELS, cy, rhi.FORMAT_R10G10B10A2_UNORM, "DDGI Probe Irradiance", uav=uav)
        dist = dev.create_texture_array(cx * DISTANCE_TEXELS, cz * DISTANCE_TEXELS, cy, rhi.FORMAT_RG16_FLOAT, "DDGI Probe Distance", uav=uav)
        for s in range(cy):
            data.upload_slice(s, self.data[s])
            irr.upload_slice(s, self.irradiance[s])
            dist.upload_slice(s, self.distance[s])
        return desc, data, irr, dist


class DDGIPass:
    """ddgi: None (the default) changes nothing: no ambient term, and debug_mode 10 (Ambient) is refused.  A ddgi.Volume (needs
    lighting=True): the DDGI ambient term from a SUPPLIED probe volume (deferredlighting.hlsl:49-76; the caller
    fills the volume, e.g. ddgi.Volume.uniform, or ddgi_update= below lets it fill itself).  The driver uploads the descriptor and
    the three array textures at construction (self.ddgi_desc, self.ddgi_data, self.ddgi_irradiance, self.ddgi_distance),
    binds them as the lighting pass's t5..t8 with the linear wrap sampler, sets m_bRTDDGIEnabled = 1 and appends the
    descriptor's host copy to the constant block; debug_mode 10 then shows the irradiance.
    ddgi_update: None (the default) changes nothing: the volume stays as supplied.  A dict of settings (needs lighting=True, ddgi=
    and GpuScene.set_raytracing()): GIRenderer::RenderDDGI, the volume fills itself.  Every record() records, behind the TLAS
    refit (which then runs with or without shadows=) and in front of the lighting pass, "giprobetrace_CS_ProbeTrace" and the two
    "ProbeBlendingCS_DDGIProbeBlendingCS" passes with a new ray rotation: ddgi.random_rotation(default_rng([seed, n])) for the
    n-th record() (self.ddgi_updates counts them); the block they ran with is self.ddgi_update_consts.  Settings: seed (0),
    hysteresis (0.5), distance_exponent (50), irradiance_threshold (0.2), brightness_threshold (0.1), max_ray_distance (1e10;
    the reference passes the scene's bounding radius).  The probe textures are then created with the UAV bit, the volume's host
    arrays are the INITIAL state (ddgi.Volume.reset() clears them as the reference does), and download_ddgi() reads the
    current one back.  relocate (False) and classify (False) add GIRenderer.cpp:513-527's probe placement behind the blends:
    "giprobetrace_CS_ProbeTraceFixedRays" (32 unrotated rays from EVERY probe into self.ddgi_fixed_rays; recorded when either is
    on), then "ProbeRelocationCS_DDGIProbeRelocationCS" (rewrites data.xyz: probes leave the geometry) and
    "ProbeClassificationCS_DDGIProbeClassificationCS" (rewrites data.w: probes that see mostly back faces, or nothing within a
    cell, are switched off and wake up when that changes), with min_frontface_distance (0.3; the reference takes 0.1 for a
    scene radius below 3) and fixed_ray_backface_threshold (0.25).  Each needs its flag on the volume (ddgi.Volume(relocation=,
    classification=), on by default) and gives the data texture the UAV bit; the lighting pass of the same frame sees the new
    data; download_ddgi_fixed_rays() reads the distances back.  With both off the supplied data texture is honoured as it is
    and the update records what it recorded before (csrc/k_giprobeplacement.hip).  variability (False) with
    variability_threshold (0.001) adds the reference's convergence early-out (GIRenderer.cpp:158-190, :466-470, :529-576): the
    driver sets flags bit 2 on a COPY of the volume (self.ddgi; host and device copy of the descriptor alike; the caller's Volume is
    not touched, and one that already carries the bit is refused without the option), the radiance
    blend also writes a coefficient of variation per interior texel (u4 = self.ddgi_variability_buffer), "ReductionCS_
    DDGIReductionCS REDUCTION=1" and "ReductionCS_DDGIExtraReductionCS" average it over the active probes, and element 0 goes
    into slot n % 2 of a two-slot read-back.  Update call n first runs ddgi.VariabilityTracker.update() and, converged, records
    NOTHING of the update (no refit unless shadows= needs it, no trace, blend, placement, reduction or copy; self.
    ddgi_updates_skipped counts them, self.ddgi_updates does not); else it stores what call n - 2 copied (0 before that:
    read without waiting for the device) into the ring.  It needs record() per frame, as the rotation does.  self.
    ddgi_variability shows average, stddev, converged and samples; download_ddgi_variability() reads the buffer;
    reset_ddgi_variability() re-arms a converged volume (nothing else does: waking on a light or transform change is not built)."""
    ddgi = ddgi_update = ddgi_update_consts = ddgi_desc = ddgi_data = ddgi_irradiance = ddgi_distance = ddgi_rays = ddgi_fixed_rays = None
    ddgi_variability_buffer = ddgi_variability_readback = ddgi_variability_average = _ddgi_tracker = None
    ddgi_updates = ddgi_updates_skipped = _ddgi_update_calls = 0

    def _check_ddgi(self, ddgi, ddgi_update, lighting, debug_mode):
        if lighting and int(debug_mode) == I.kDeferredLightingDebugMode_Ambient and ddgi is None:
            raise ValueError("debug_mode 10 (Ambient) needs the DDGI volume: pass ddgi=ddgi.Volume(...)")
        if ddgi is not None and not lighting:
            raise ValueError("ddgi=... needs lighting=True: the lighting pass is what reads the probe volume")
        if ddgi is not None and not isinstance(ddgi, Volume):
            raise ValueError("ddgi: needs a ddgi.Volume")
        self.ddgi = ddgi
        if ddgi_update is None:
            return
        if not lighting or ddgi is None:
            raise ValueError("ddgi_update=... needs lighting=True and ddgi=ddgi.Volume(...): the volume the update fills and the pass that reads it")
        if self.scene.rt is None:
            raise ValueError("ddgi_update=... needs GpuScene.set_raytracing(): the acceleration structure the probe rays walk")
        self.ddgi_update = check_update_settings(ddgi_update)
        if self.ddgi_update["variability"]:
            if int(np.prod(ddgi.counts)) * 36 > 1 << 24:
                raise ValueError("ddgi_update: variability=True with more than 2^24 interior irradiance texels; the reduction counts them in a float")
            ddgi = self.ddgi = ddgi.copy()       # the caller's Volume stays as it is: the bit is the driver's, on its own copy
            ddgi.variability = True              # the descriptor's bit 2, before the volume is uploaded
        elif ddgi.variability:
            raise ValueError("ddgi_update: the ddgi.Volume has variability=True (flags bit 2) and ddgi_update has variability=False: the radiance blend would "
                             "need the variability buffer at u4; clear the flag or pass variability=True")
        for option, flag, word in (("relocate", ddgi.relocation, "relocation"), ("classify", ddgi.classification, "classification")):
            if self.ddgi_update[option] and not flag:
                raise ValueError(f"ddgi_update: {option}=True needs ddgi.Volume({word}=True): with the flag off nothing reads what the pass writes")

    def _create_ddgi(self):
        if self.ddgi is None:
            return
        dev, u, n = self.dev, self.ddgi_update, int(np.prod(self.ddgi.counts))
        placement = u is not None and (u["relocate"] or u["classify"])
        # GIRenderer::Setup's textures (GIRenderer.cpp:129-133), filled by the caller
        self.ddgi_desc, self.ddgi_data, self.ddgi_irradiance, self.ddgi_distance = (self._own(r) for r in self.ddgi.upload(dev, uav=u is not None, data_uav=placement))
        if u is None:
            return
        if u["variability"]:
            cx, cy, cz = self.ddgi.counts
            self.ddgi_variability_buffer = self._own(dev.create_buffer(n * 36 * 4, "DDGI Probe Variability", stride=4))
            self.ddgi_variability_buffer.upload(np.zeros(n * 36, np.float32))
            groups = -(-6 * cx // 16) * -(-6 * cz // 16) * -(-cy // 4)       # the first pass's outputs; every later pass has fewer
            self.ddgi_variability_average = [self._own(dev.create_buffer(groups * 8, f"DDGI Probe Variability Average {i}", stride=8)) for i in range(2)]
            self.ddgi_variability_readback = self._own(dev.create_readback(4, 2))
            self._ddgi_tracker = VariabilityTracker(u["variability_threshold"])
        self.ddgi_rays = self._own(dev.create_buffer(n * I.kDDGIRaysPerProbe * 16, "DDGI Ray Data", stride=16))     # GIRenderer::Setup's ray data, float4 records
        self.ddgi_rays.upload(np.zeros(self.ddgi_rays.size // 4, np.float32))     # an inactive probe's records keep what they hold
        if placement:                                # the distances of the 32 fixed rays of every probe
            self.ddgi_fixed_rays = self._own(dev.create_buffer(n * I.kDDGIFixedRays * 4, "DDGI Fixed Ray Distances", stride=4))
            self.ddgi_fixed_rays.upload(np.zeros(self.ddgi_fixed_rays.size // 4, np.float32))

    # ---- GIRenderer::RenderDDGI (GIRenderer.cpp): the probe trace and the two blends ---------------------------------------------
    def _ddgi_begin_update(self):
        """RenderDDGI's opening (GIRenderer.cpp:464-470), once per record(): True when this call records nothing of the update."""
        if self._ddgi_tracker is None:
            return False
        self._ddgi_call = self._ddgi_update_calls        # this call's number since the last reset: its read-back slot is this % 2
        self._ddgi_update_calls += 1
        skip = self._ddgi_tracker.update()
        self.ddgi_updates_skipped += int(skip)
        return skip

    def _ddgi_variability(self, cl, cb):
        """GIRenderer.cpp:529-576: the sample of two calls ago into the ring, this call's reductions, the copy of their result."""
        cx, cy, cz = self.ddgi.counts
        slot = self._ddgi_call % 2
        got, _ = self.ddgi_variability_readback.read(slot, np.float32, 1)   # waits for that slot's copy only; 0 for a slot never written
        self._ddgi_tracker.set(got[0])
        size, n = (6 * cx, 6 * cz, cy), 0
        while n == 0 or max(size) > 1:
            out = tuple(-(-s // g) for s, g in zip(size, I.kDDGIReductionGroup))
            push = np.zeros(1, I.DDGIRootConstants)
            push["reductionInputSizeX"], push["reductionInputSizeY"], push["reductionInputSizeZ"] = size
            src, dst = self.ddgi_variability_average[(n + 1) % 2], self.ddgi_variability_average[n % 2]   # ping-pong: a pass never reads what it writes
            if n == 0:
                cl.dispatch("ReductionCS_DDGIReductionCS REDUCTION=1", [CB(0, cb), PUSH(1), TEX_SRV(3, self.ddgi_data), SRV(4, self.ddgi_variability_buffer), UAV(5, dst)], out, push=push)
            else:
                cl.dispatch("ReductionCS_DDGIExtraReductionCS", [PUSH(1), SRV(4, src), UAV(5, dst)], out, push=push)
            size, n = out, n + 1
        cl.copy_to_readback(self.ddgi_variability_readback, slot, self.ddgi_variability_average[(n + 1) % 2], 0, 4)

    @property
    def ddgi_variability(self):
        """dict(average, stddev, converged, samples) of the convergence rule, or None with variability off."""
        t = self._ddgi_tracker
        return None if t is None else dict(average=t.average, stddev=t.stddev, converged=t.converged, samples=t.samples)

    @property
    def ddgi_variability_ring(self):
        """A copy of the rule's ring of the last 16 stored averages (float32 [16], in index order), or None with variability off."""
        return None if self._ddgi_tracker is None else self._ddgi_tracker.ring.copy()

    def download_ddgi_variability(self) -> np.ndarray:
        """The variability buffer, float32 [counts.y, 6 counts.z, 6 counts.x]."""
        def read():
            cx, cy, cz = self.ddgi.counts
            return self.ddgi_variability_buffer.download(np.float32).reshape(cy, 6 * cz, 6 * cx)
        return self._download("download_ddgi_variability", self.ddgi_variability_buffer, VARIABILITY_OFF, read)

    def reset_ddgi_variability(self):
        """Re-arms the update: the whole tracker starts again, the pending read-back slots are dropped and the variability buffer is zeroed."""
        if self._ddgi_tracker is None:
            raise ValueError("reset_ddgi_variability: " + VARIABILITY_OFF)
        self.dev.wait_idle()
        self._ddgi_tracker.reset()
        self._ddgi_update_calls = self.ddgi_updates_skipped = 0
        self.ddgi_variability_buffer.upload(np.zeros(self.ddgi_variability_buffer.size // 4, np.float32))
        self.ddgi_variability_readback.reset()       # kept: the list recorded last still names it

    def _ddgi_update(self, cl):
        sc, vol, u = self.scene, self.ddgi, self.ddgi_update
        rt = sc.rt
        k = np.zeros(1, I.DDGIUpdateConsts)
        k["m_DirectionalLightVector"], k["m_DirectionalLightStrength"] = self.dir_light
        k["rayRotation"][0, :, :3] = random_rotation(np.random.default_rng([u["seed"], self.ddgi_updates]))
        k["probeMaxRayDistance"], k["probeHysteresis"], k["probeDistanceExponent"] = u["max_ray_distance"], u["hysteresis"], u["distance_exponent"]
        k["probeIrradianceThreshold"], k["probeBrightnessThreshold"] = u["irradiance_threshold"], u["brightness_threshold"]
        if u["relocate"] or u["classify"]:
            k["probeMinFrontfaceDistance"], k["probeFixedRayBackfaceThreshold"] = u["min_frontface_distance"], u["fixed_ray_backface_threshold"]
        self.ddgi_update_consts = k
        self.ddgi_updates += 1
        cb = cl.constant_buffer(np.frombuffer(k.tobytes() + vol.desc().tobytes(), np.uint8), "DDGIUpdateConsts")
        cx, cy, cz = vol.counts
        cl.dispatch("giprobetrace_CS_ProbeTrace",
                    [CB(0, cb), SRV(0, self.ddgi_desc), TEX_SRV(1, self.ddgi_data), TEX_SRV(2, self.ddgi_irradiance), TEX_SRV(3, self.ddgi_distance), SRV(4, rt["tlas_nodes"]),
                     SRV(5, sc.instances), SRV(6, sc.vertices), SRV(7, sc.materials), SRV(8, sc.indices), SRV(9, sc.meshData), SRV(10, rt["tlas_instances"]),
                     SRV(11, rt["headers"]), SRV(12, rt["blas_nodes"]), SRV(13, rt["tri_order"]), UAV(0, self.ddgi_rays), SAMPLER(0), SAMPLER(1), SAMPLER(2)],
                    (I.kDDGIRaysPerProbe // 64, cx * cz, cy))
        cl.dispatch("ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1",
                    [CB(0, cb), SRV(1, self.ddgi_rays), TEX_SRV(3, self.ddgi_data), TEX_UAV(1, self.ddgi_irradiance, 0)] +
                    ([UAV(4, self.ddgi_variability_buffer)] if u["variability"] else []), (cx, cz, cy))
        cl.dispatch("ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0",
                    [CB(0, cb), SRV(1, self.ddgi_rays), TEX_SRV(3, self.ddgi_data), TEX_UAV(2, self.ddgi_distance, 0)], (cx, cz, cy))
        if u["relocate"] or u["classify"]:
            self._ddgi_placement(cl, cb)
        if u["variability"]:
            self._ddgi_variability(cl, cb)

    def _ddgi_placement(self, cl, cb):
        sc, u = self.scene, self.ddgi_update
        rt = sc.rt
        cx, cy, cz = self.ddgi.counts
        n = cx * cy * cz                             # GIRenderer.cpp:513-527: relocation and classification behind the blends
        cl.dispatch("giprobetrace_CS_ProbeTraceFixedRays",
                    [CB(0, cb), SRV(0, self.ddgi_desc), TEX_SRV(1, self.ddgi_data), SRV(4, rt["tlas_nodes"]), SRV(5, sc.instances), SRV(6, sc.vertices), SRV(8, sc.indices),
                     SRV(9, sc.meshData), SRV(10, rt["tlas_instances"]), SRV(11, rt["headers"]), SRV(12, rt["blas_nodes"]), SRV(13, rt["tri_order"]),
                     UAV(0, self.ddgi_fixed_rays)], ((n * I.kDDGIFixedRays + 63) // 64, 1, 1))
        for on, name in ((u["relocate"], "ProbeRelocationCS_DDGIProbeRelocationCS"), (u["classify"], "ProbeClassificationCS_DDGIProbeClassificationCS")):
            if on:
                cl.dispatch(name, [CB(0, cb), UAV(0, self.ddgi_fixed_rays), TEX_UAV(3, self.ddgi_data, 0)], ((n + 31) // 32, 1, 1))

    def _read_volume(self):
        vol = self.ddgi.copy()
        for s in range(vol.counts[1]):
            vol.irradiance[s] = self.ddgi_irradiance.download_slice(s)
            vol.distance[s] = self.ddgi_distance.download_slice(s).reshape(vol.distance[s].shape)
            vol.data[s] = self.ddgi_data.download_slice(s).reshape(vol.data[s].shape)
        return vol

    def download_ddgi(self):
        """A copy of the driver's ddgi.Volume with the probe textures as they are on the device now."""
        return self._download("download_ddgi", self.ddgi, "there is no volume (ddgi=None)", self._read_volume)

    def download_ddgi_rays(self) -> np.ndarray:
        """The ray records of the last update, float32 [numProbes, 256, 4]."""
        return self._download("download_ddgi_rays", self.ddgi_rays, "the probe update is off (ddgi_update=None)",
                              lambda: self.ddgi_rays.download(np.float32).reshape(-1, I.kDDGIRaysPerProbe, 4))

    def download_ddgi_fixed_rays(self) -> np.ndarray:
        """The fixed-ray distances of the last update, float32 [numProbes, 32]: t for a front face, -0.2 t for a back face, 1e27 for a miss."""
        return self._download("download_ddgi_fixed_rays", self.ddgi_fixed_rays, "probe placement is off (ddgi_update without relocate=True or classify=True)",
                              lambda: self.ddgi_fixed_rays.download(np.float32).reshape(-1, I.kDDGIFixedRays))


class ProbeDrawPass:
    """probes: None (the default) changes nothing.  A dict (needs ddgi= and post=True) draws the volume's probes into the back buffer
    behind the post pass, GIDebugRenderer's three dispatches (csrc/k_giprobedraw.hip, csrc/k_giprobe.hip): "giprobevisualization_
    CS_LoadGIProbes" writes every probe's position and state from the LIVE volume into self.probe_positions and
    self.probe_states, "giprobevisualization_CS_VisualizeGIProbesCulling" culls them against the frame's HZB into
    self.probe_culled_positions, self.probe_draw_args and self.probe_instance_to_probe, and "giprobevisualization_PS_
    VisualizeGIProbes" draws the survivors as spheres shaded with their own irradiance, depth-tested against self.depth, which it
    also writes.  Settings: radius (0.1, GIRenderer.cpp's m_ProbeRadius) and hide_inactive (False).  The block the draw ran with
    is self.probe_draw_consts; download_probes() and download_probe_winners() read the results back."""
    probes = probe_positions = probe_states = probe_culled_positions = probe_draw_args = probe_instance_to_probe = None
    probe_sphere_vertices = probe_sphere_indices = probe_winners = probe_draw_consts = probe_cull_consts = None

    def _check_probes(self, probes, post):
        if probes is None:
            return
        if self.ddgi is None or not post:
            raise ValueError("probes=... needs " + ("ddgi=ddgi.Volume(...): the volume whose probes are drawn" if self.ddgi is None else "post=True: the spheres are drawn into the back buffer"))
        unknown = set(probes) - {"radius", "hide_inactive"}
        if unknown:
            raise ValueError(f"probes: unknown settings {sorted(unknown)}; known: ['hide_inactive', 'radius']")
        self.probes = dict(radius=float(probes.get("radius", 0.1)), hide_inactive=bool(probes.get("hide_inactive", False)))
        if not (np.isfinite(self.probes["radius"]) and self.probes["radius"] > 0.0):
            raise ValueError(f"probes: radius = {self.probes['radius']} is not positive and finite")

    def _create_probes(self):                        # GIDebugRenderer::Setup (GIRenderer.cpp:612-657) + CommonResources' UnitSphere
        if self.probes is None:
            return
        dev, n_probes = self.dev, int(np.prod(self.ddgi.counts))
        self.probe_positions = self._own(dev.create_buffer(12 * n_probes, "GI Probe Positions", stride=12))
        self.probe_states = self._own(dev.create_buffer(4 * n_probes, "GI Probe States"))
        self.probe_culled_positions = self._own(dev.create_buffer(12 * n_probes, "Probe Positions", stride=12))
        self.probe_draw_args = self._own(dev.create_buffer(20, "Probe Draw Indirect Args", stride=20, indirect=True))
        self.probe_instance_to_probe = self._own(dev.create_buffer(4 * n_probes, "Instance ID to Probe Index"))
        sphere_v, sphere_i = unit_sphere()
        self.probe_sphere_vertices = self._own(dev.buffer_from(sphere_v, "Unit Sphere Vertex Buffer", uav=False))
        self.probe_sphere_indices = self._own(dev.buffer_from(sphere_i, "Unit Sphere Index Buffer", uav=False))
        self.probe_winners = self._own(dev.create_texture(self.view.renderW, self.view.renderH, 1, rhi.FORMAT_RG32_UINT, "Probe Draw Winners"))

    # ---- GIDebugRenderer::RenderDDGIDebug (GIRenderer.cpp:672-808) ------------------------------
    def _probe_visualization(self, cl):
        v, vol = self.view, self.ddgi
        n = int(np.prod(vol.counts))
        desc = vol.desc()
        cl.dispatch("giprobevisualization_CS_LoadGIProbes",
                    [CB(0, cl.constant_buffer(np.frombuffer(desc.tobytes(), np.uint8), "DDGIVolumeDesc")), SRV(0, self.ddgi_desc), TEX_SRV(1, self.ddgi_data),
                     UAV(0, self.probe_positions), UAV(1, self.probe_states)], ((n + 31) // 32, 1, 1))
        args = np.zeros(1, I.DrawIndexedIndirectArguments)                               # :683-689: the sphere's indices, no instance yet
        args["m_IndexCount"] = I.kUnitSphereIndices
        cl.write_buffer(self.probe_draw_args, args)
        ck = np.zeros(1, I.GIProbeVisualizationUpdateConsts)                             # :687-708
        ck["m_NumProbes"] = n
        ck["m_CameraOrigin"] = self.camera_origin
        ck["m_Frustum"] = self._culling_frustum()
        ck["m_WorldToView"] = v.worldToView
        ck["m_HZBDimensions"] = (self.hzb_w, self.hzb_h)
        ck["m_P00"], ck["m_P11"] = v.viewToClip[0, 0], v.viewToClip[1, 1]
        ck["m_NearPlane"] = v.nearPlane
        ck["m_ProbeRadius"] = self.probes["radius"]
        ck["m_bHideInactiveProbes"] = int(self.probes["hide_inactive"])
        cl.dispatch("giprobevisualization_CS_VisualizeGIProbesCulling",
                    [CB(0, cl.constant_buffer(ck, "GIProbeVisualizationUpdateConsts")), TEX_SRV(0, self.hzb), SRV(10, self.probe_positions), SRV(11, self.probe_states),
                     UAV(0, self.probe_culled_positions), UAV(1, self.probe_draw_args), UAV(2, self.probe_instance_to_probe), SAMPLER(0)], ((n + 31) // 32, 1, 1))
        dk = np.zeros(1, I.GIProbeVisualizationConsts)                                   # :745-752
        dk["m_WorldToClip"] = I.world_to_clip(v.worldToView, v.viewToClip)
        dk["m_CameraDirection"] = -np.asarray(v.worldToView, np.float32)[:3, 2]          # the view looks down -Z; the draw does not read it
        dk["m_ProbeRadius"] = self.probes["radius"]
        dk["m_NearPlane"] = v.nearPlane
        block = np.frombuffer(dk.tobytes() + desc.tobytes(), np.uint8)
        cl.dispatch("giprobevisualization_PS_VisualizeGIProbes",
                    [CB(0, cl.constant_buffer(block, "GIProbeVisualizationConsts")), SRV(0, self.probe_culled_positions), TEX_SRV(1, self.ddgi_data),
                     TEX_SRV(2, self.ddgi_irradiance), TEX_SRV(3, self.ddgi_distance), SRV(4, self.ddgi_desc), SRV(5, self.probe_instance_to_probe),
                     SRV(6, self.probe_draw_args), SRV(7, self.probe_sphere_vertices), SRV(8, self.probe_sphere_indices), TEX_UAV(0, self.depth, 0),
                     TEX_UAV(1, self.back_buffer, 0), TEX_UAV(2, self.probe_winners, 0), SAMPLER(0)], (1, 1, 1))
        self.probe_cull_consts, self.probe_draw_consts = ck, dk

    def _read_probes(self):
        n = int(np.prod(self.ddgi.counts))
        count = min(int(self.probe_draw_args.download(np.uint32, 5)[1]), n)
        return count, self.probe_culled_positions.download(np.float32, 3 * n).reshape(n, 3)[:count], self.probe_instance_to_probe.download(np.uint32, n)[:count]

    def download_probes(self):
        """(count, culled positions float32 [count, 3], instance -> probe index uint32 [count]) of the last frame run."""
        return self._download("download_probes", self.probes, PROBES_OFF, self._read_probes)

    def download_probe_winners(self) -> np.ndarray:
        """The draw's winner words of the last frame run, uint64 [H, W]: (depth bits << 32) | instance << 8 | triangle, 0 = no sphere."""
        return self._download("download_probe_winners", self.probes, PROBES_OFF, lambda: self.probe_winners.download_mip(0))
