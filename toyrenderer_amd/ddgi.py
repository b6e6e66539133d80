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
        from . import rhi
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
