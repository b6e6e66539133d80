"""The Hosek-Wilkie sky parameters on the host: HosekWilkieHelper::CalculateSkyParameters of the reference's SkyRenderer.cpp:41-129,
and the SkyPassParameters block of "sky_PS_HosekWilkieSky" (csrc/k_sky.hip).

The same 30 floats, bit for bit, as csrc/host/SkyRenderer.cpp: the same operations in the same types as the reference writes
them, with its roundings to float (sun_theta, std::max<float>, 1.f / 3.0f, turbidityK, the (float) of each Evaluate).  pow, acos
and cos are math.pow / math.acos / math.cos, the C library's double functions the C++ side calls, never numpy's vector loops.

The dataset (the model's published RGB coefficient tables: three tables of 1080 doubles, three radiance tables of 120 doubles)
is an input, not part of this package: HosekDataset builds from two arrays, loads from an .npz, or reads the
`double name[] = { ... };` arrays out of a header an integrator already has.

Row 9 (the reference divides Z by the luminance of its normalisation helper at the sun): DirectXMath's polynomial Exp2 / Pow are
not restated; the helper is evaluated in double from the 30 rounded floats and row 9 is rounded once."""
from __future__ import annotations

import math
import re

import numpy as np

from . import interop as I
from .rhi import CB, TEX_SRV, TEX_UAV

F = np.float32
DEFAULT_TURBIDITY = 2.0
DEFAULT_GROUND_ALBEDO = (0.1, 0.1, 0.1)
_PI = 3.14159265358979323846


class HosekDataset:
    """rgb: (3, 1080) doubles = per channel 2 albedos x 10 turbidities x 6 control points x 9 parameters; rad: (3, 120)."""

    def __init__(self, rgb, rad):
        self.rgb = np.ascontiguousarray(rgb, np.float64)
        self.rad = np.ascontiguousarray(rad, np.float64)
        if self.rgb.shape != (3, 1080) or self.rad.shape != (3, 120):
            raise ValueError(f"HosekDataset: needs arrays of shape (3, 1080) and (3, 120), got {self.rgb.shape} and {self.rad.shape}")
        if not (np.all(np.isfinite(self.rgb)) and np.all(np.isfinite(self.rad))):
            raise ValueError("HosekDataset: a table entry is not finite")

    @classmethod
    def load(cls, path) -> "HosekDataset":
        with np.load(path) as z:
            return cls(z["rgb"], z["rad"])

    def save(self, path):
        np.savez_compressed(path, rgb=self.rgb, rad=self.rad)

    @classmethod
    def from_header(cls, path, rgb_names=("datasetRGB1", "datasetRGB2", "datasetRGB3"),
                    rad_names=("datasetRGBRad1", "datasetRGBRad2", "datasetRGBRad3")) -> "HosekDataset":
        """Reads `double name[] = { ... };` arrays (comments ignored) out of a C header."""
        with open(path, "r", encoding="utf-8", errors="replace") as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        arrays = {m.group(1): m.group(2) for m in re.finditer(r"double\s+(\w+)\s*\[\s*\]\s*=\s*\{([^{}]*)\}\s*;", text)}

        def table(name):
            if name not in arrays:
                raise ValueError(f"HosekDataset.from_header: no array `double {name}[]` in {path}")
            return np.array([float(t) for t in arrays[name].replace(",", " ").split()], np.float64)
        return cls(np.stack([table(n) for n in rgb_names]), np.stack([table(n) for n in rad_names]))


def _spline(d: np.ndarray, base: int, stride: int, value: float) -> float:
    p = math.pow
    return (1 * p(1.0 - value, 5) * d[base] +
            5 * p(1.0 - value, 4) * p(value, 1) * d[base + stride] +
            10 * p(1.0 - value, 3) * p(value, 2) * d[base + 2 * stride] +
            10 * p(1.0 - value, 2) * p(value, 3) * d[base + 3 * stride] +
            5 * p(1.0 - value, 1) * p(value, 4) * d[base + 4 * stride] +
            1 * p(value, 5) * d[base + 5 * stride])


def _evaluate(table: np.ndarray, offset: int, stride: int, turbidity: F, albedo: F, sun_theta: F) -> float:
    d = [float(x) for x in table]
    elevation = F(1.0 - float(sun_theta) / (_PI * 0.5))                                  # std::max<float>(0.f, double)
    elevation_k = math.pow(float(max(F(0.0), elevation)), float(F(1.0) / F(3.0)))
    t0 = min(max(int(turbidity), 1), 10)                                                 # static_cast<int>: truncation
    t1 = min(t0 + 1, 10)
    tk = min(max(F(turbidity - F(t0)), F(0.0)), F(1.0))
    a0, a1 = offset, offset + stride * 6 * 10
    a0t0 = _spline(d, a0 + stride * 6 * (t0 - 1), stride, elevation_k)
    a1t0 = _spline(d, a1 + stride * 6 * (t0 - 1), stride, elevation_k)
    a0t1 = _spline(d, a0 + stride * 6 * (t1 - 1), stride, elevation_k)
    a1t1 = _spline(d, a1 + stride * 6 * (t1 - 1), stride, elevation_k)
    one_a, one_t, al, tkd = float(F(1.0) - albedo), float(F(1.0) - tk), float(albedo), float(tk)
    return a0t0 * one_a * one_t + a1t0 * al * one_t + a0t1 * one_a * tkd + a1t1 * al * tkd


def helper(params: np.ndarray, c: int, cos_theta, gamma, cos_gamma) -> float:
    """The reference's normalisation helper (SkyRenderer.cpp:73-95) of channel c, in double from float32 rows: not the shader's
    function (no `1 +` in the first factor, F * gamma^2, a base-two exponential)."""
    A, B, C_, D, E, F_, G, H, I_ = (float(params[r, c]) for r in range(9))
    cos_theta, gamma, cos_gamma = F(cos_theta), F(gamma), F(cos_gamma)
    chi = float(F(1.0) + cos_gamma * cos_gamma) / math.pow(H * H + 1.0 - H * float(F(2.0) * cos_gamma), 1.5)
    temp1 = A * math.pow(2.0, B * float(F(1.0) / (cos_theta + F(0.01))))
    temp2 = (C_ + D * math.pow(2.0, E * float(gamma)) + F_ * float(gamma * gamma) + chi * G +
             I_ * float(F(math.sqrt(float(max(cos_theta, F(0.0)))))))
    return temp1 * temp2


def sky_parameters(dataset: HosekDataset, turbidity, ground_albedo, sun_direction) -> np.ndarray:
    """CalculateSkyParameters: float32 (10, 3), rows A B C D E F G H I Z, columns R G B."""
    turbidity = F(turbidity)
    albedo = np.asarray(ground_albedo, F).reshape(3)
    sun = np.asarray(sun_direction, F).reshape(3)
    sun_theta = F(math.acos(float(min(max(sun[1], F(0.0)), F(1.0)))))
    out = np.zeros((10, 3), F)
    for i in range(3):
        for r in range(7):
            out[r, i] = F(_evaluate(dataset.rgb[i], r, 9, turbidity, albedo[i], sun_theta))
        out[7, i] = F(_evaluate(dataset.rgb[i], 8, 9, turbidity, albedo[i], sun_theta))      # data values are swapped
        out[8, i] = F(_evaluate(dataset.rgb[i], 7, 9, turbidity, albedo[i], sun_theta))
        out[9, i] = F(_evaluate(dataset.rad[i], 0, 1, turbidity, albedo[i], sun_theta))
    cos_theta = F(math.cos(float(sun_theta)))
    S = [helper(out, i, cos_theta, 0.0, 1.0) * float(out[9, i]) for i in range(3)]
    lum = S[0] * float(F(0.2126)) + S[1] * float(F(0.7152)) + S[2] * float(F(0.0722))
    with np.errstate(all="ignore"):
        for i in range(3):
            out[9, i] = F(np.float64(out[9, i]) / np.float64(lum))
    return out


def check_settings(turbidity, ground_albedo):
    """The ranges of the reference's sliders (SkyRenderer.cpp:146-147); what trhost_set_sky refuses is refused here."""
    t = float(turbidity)
    if not (math.isfinite(t) and 1.0 <= t <= 10.0):
        raise ValueError(f"sky: turbidity {turbidity} is not a finite number in [1, 10]")
    a = np.asarray(ground_albedo, np.float64).reshape(-1)
    if a.shape != (3,) or not np.all((a >= 0.0) & (a <= 1.0)):
        raise ValueError(f"sky: ground albedo {ground_albedo} is not three numbers in [0, 1]")


def pass_parameters(clip_to_world, sun_direction, camera_position, params) -> np.ndarray:
    """The 256-byte SkyPassParameters block (SkyRenderer.cpp:178-187); .w of every row and the pads are 0."""
    k = np.zeros(1, I.SkyPassParameters)
    k["m_ClipToWorld"] = np.asarray(clip_to_world, F).reshape(4, 4)
    k["m_SunLightDir"] = np.asarray(sun_direction, F).reshape(3)
    k["m_CameraPosition"] = np.asarray(camera_position, F).reshape(3)
    k["m_HosekParams"]["m_Params"][0, :, :3] = np.asarray(params, F).reshape(10, 3)
    return k


class SkyPass:
    """sky: None (the default) changes nothing.  (dataset,) or (dataset, turbidity, ground_albedo) with a sky.HosekDataset
    (needs lighting=True; the reference's defaults are turbidity 2.0 and ground albedo (0.1, 0.1, 0.1)): SkyRenderer
    (SkyRenderer.cpp).  One "sky_PS_HosekWilkieSky" dispatch directly behind the lighting dispatch, in front of bloom and the
    histogram clear, whatever debug_mode is, fills every texel of LightingOutput whose depth is <= 0.  The sun direction is
    dir_light[0] as given, the camera position camera_origin, the matrix the lighting pass's m_ClipToWorld.
    self.sky_consts holds the 256-byte SkyPassParameters of the last record()."""
    sky = sky_consts = None

    def _check_sky(self, sky, lighting):
        if sky is None:
            return
        if not lighting:
            raise ValueError("sky=... needs lighting=True: the pass fills the texels of LightingOutput the lighting pass leaves")
        sky = tuple(sky)
        if not (1 <= len(sky) <= 3) or not isinstance(sky[0], HosekDataset):
            raise ValueError("sky: needs (dataset, turbidity, ground_albedo) with a sky.HosekDataset first")
        turbidity = sky[1] if len(sky) > 1 else DEFAULT_TURBIDITY
        albedo = sky[2] if len(sky) > 2 else DEFAULT_GROUND_ALBEDO
        check_settings(turbidity, albedo)
        self.sky = (sky[0], np.float32(turbidity), tuple(np.float32(x) for x in albedo))

    # ---- SkyRenderer::Render (SkyRenderer.cpp:163-208) -------------------------------------------------------------------
    def _sky(self, cl):
        v = self.view
        dataset, turbidity, albedo = self.sky
        sun = np.asarray(self.dir_light[0], np.float32)
        params = sky_parameters(dataset, turbidity, albedo, sun)
        self.sky_consts = pass_parameters(self.lighting_consts["m_ClipToWorld"][0], sun, self.camera_origin, params)
        cb = cl.constant_buffer(self.sky_consts, "SkyPassParameters")
        cl.dispatch("sky_PS_HosekWilkieSky", [CB(0, cb), TEX_SRV(0, self.depth), TEX_UAV(0, self.lighting_output, 0)], I.groups8(v.renderW, v.renderH))
