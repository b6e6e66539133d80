"""The sky pass's reference (tests/sky_ref.c) and the host side of the Hosek-Wilkie parameters (toyrenderer_amd/sky.py), on the CPU:
the 30 floats of Python against the C restatement bit for bit, the dataset reader, the normalisation of row 9, the software arc
cosine against float64 within the bound derived in the source, the radiometric accuracy of the binary32 pass against the same
formula in float64 within the bound derived in sky_ref.c, and the value spread the GPU tests rely on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sky_ref as SR  # noqa: E402
from suite_support import sk  # noqa: E402, F401
from toyrenderer_amd import interop as I  # noqa: E402
from toyrenderer_amd import sky  # noqa: E402

F = np.float32
W, H = 67, 35


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the dataset ---------------------------------------------------------------------------------------------------------------
def test_fixture_has_the_stated_shapes():
    ds = SR.dataset()
    assert ds.rgb.shape == (3, 1080) and ds.rad.shape == (3, 120) and ds.rgb.dtype == np.float64 and ds.rad.dtype == np.float64
    assert ds.rgb.nbytes + ds.rad.nbytes == 28800
    assert np.all(np.isfinite(ds.rgb)) and np.all(np.isfinite(ds.rad))


def test_from_header_round_trips_a_synthetic_header(tmp_path):
    rng = np.random.default_rng(3)
    rgb, rad = rng.normal(0, 3, (3, 1080)), rng.normal(0, 3, (3, 120))
    rgb[0, :4] = [0.0, -1.099459e+000, 1e-300, -2.5e+17]
    lines = ["// a synthetic header", "#pragma once", "/* block", " comment 1.0, 2.0 */"]
    for c in range(3):
        for name, t in ((f"datasetRGB{c + 1}", rgb[c]), (f"datasetRGBRad{c + 1}", rad[c])):
            lines.append(f"double {name}[] = ")
            lines.append("{")
            for i, v in enumerate(t):
                if i % 9 == 0:
                    lines.append(f"\t// albedo {i // 540}, turbidity {i // 54 % 10 + 1}")
                lines.append("\t" + repr(float(v)) + ",")
            lines.append("};")
            lines.append("")
    lines += ["double* datasetsRGB[] =", "{", "\tdatasetRGB1,", "\tdatasetRGB2,", "\tdatasetRGB3", "};"]
    path = tmp_path / "Synthetic.h"
    path.write_text("\n".join(lines))
    ds = sky.HosekDataset.from_header(str(path))
    assert ds.rgb.tobytes() == rgb.tobytes() and ds.rad.tobytes() == rad.tobytes()
    ds.save(str(tmp_path / "again.npz"))
    again = sky.HosekDataset.load(str(tmp_path / "again.npz"))
    assert again.rgb.tobytes() == rgb.tobytes() and again.rad.tobytes() == rad.tobytes()
    with pytest.raises(ValueError, match="no array"):
        sky.HosekDataset.from_header(str(path), rgb_names=("datasetRGB1", "datasetRGB2", "missing"))
    with pytest.raises(ValueError, match="shape"):
        sky.HosekDataset(rgb[:, :100], rad)
    with pytest.raises(ValueError, match="finite"):
        sky.HosekDataset(np.where(np.arange(1080) == 5, np.nan, rgb), rad)


# ---- CalculateSkyParameters ----------------------------------------------------------------------------------------------------
TURBIDITIES = (1.0, 1.5, 9.99, 10.0, 0.5)


@pytest.mark.parametrize("config", range(len(SR.CONFIGS)))
def test_python_parameters_equal_the_c_restatement(sk, config):
    ds = SR.dataset()
    turbidity, albedo, sun = SR.CONFIGS[config]
    for t in (turbidity,) + TURBIDITIES:
        got, want = sky.sky_parameters(ds, t, albedo, sun), SR.parameters(sk, ds, t, albedo, sun)
        assert got.dtype == F and got.shape == (10, 3)
        assert _bits(got).tolist() == _bits(want).tolist(), (config, t)
        assert np.all(np.isfinite(got))
    # a turbidity below 1 is clamped: the table index and the blend weight are those of 1
    assert _bits(sky.sky_parameters(ds, 0.5, albedo, sun)).tolist() == _bits(sky.sky_parameters(ds, 1.0, albedo, sun)).tolist()


def test_rows_7_and_8_take_dataset_columns_8_and_7():
    """At turbidity 1, albedo 0 and the sun at the zenith the spline weight is on the last control point alone (elevation 1)."""
    ds = SR.dataset()
    p = sky.sky_parameters(ds, 1.0, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    for c in range(3):
        last = ds.rgb[c][5 * 9:6 * 9]                                         # albedo 0, turbidity 1, control point 5
        assert p[7, c] == F(last[8]) and p[8, c] == F(last[7]) and p[0, c] == F(last[0]) and p[6, c] == F(last[6])


@pytest.mark.parametrize("config", range(len(SR.CONFIGS)))
def test_row_9_normalises_the_helper_at_the_sun(sk, config):
    """With row 9 as produced, the luminance of Z * helper at the sun is 1 to the accuracy of one float rounding (of Z, per channel)."""
    ds = SR.dataset()
    turbidity, albedo, sun = SR.CONFIGS[config]
    p = sky.sky_parameters(ds, turbidity, albedo, sun)
    cos_theta = F(math.cos(float(F(math.acos(float(min(max(sun[1], F(0)), F(1))))))))
    w = [float(F(0.2126)), float(F(0.7152)), float(F(0.0722))]
    terms = [w[c] * float(p[9, c]) * sky.helper(p, c, cos_theta, 0.0, 1.0) for c in range(3)]
    assert abs(sum(terms) - 1.0) <= 2.0 ** -24 * sum(abs(t) for t in terms) + 1e-15, (config, sum(terms))
    for c in range(3):                                                        # the C helper is the same function
        assert sky.helper(p, c, cos_theta, 0.0, 1.0) == sk.sk_helper(np.ascontiguousarray(p).ctypes.data, c, float(cos_theta), 0.0, 1.0)


def test_pass_parameters_layout_and_settings():
    p = np.arange(30, dtype=F).reshape(10, 3) + F(1)
    k = sky.pass_parameters(np.arange(16, dtype=F).reshape(4, 4), (1, 2, 3), (4, 5, 6), p)
    raw = k.view(F).reshape(64)
    assert k.itemsize == 256 and raw[:16].tolist() == list(range(16)) and raw[16:24].tolist() == [1, 2, 3, 0, 4, 5, 6, 0]
    assert raw[24:].reshape(10, 4)[:, :3].tolist() == p.tolist() and not raw[24:].reshape(10, 4)[:, 3].any()
    for bad in (0.99, 10.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="turbidity"):
            sky.check_settings(bad, (0.1, 0.1, 0.1))
    for bad in ((0.1, 0.1, 1.01), (-0.01, 0, 0), (0.1, 0.1), (0.1, float("nan"), 0.1)):
        with pytest.raises(ValueError, match="albedo"):
            sky.check_settings(2.0, bad)
    sky.check_settings(1.0, (0.0, 1.0, 0.5)); sky.check_settings(10.0, (1, 1, 1))


# ---- the software arc cosine ---------------------------------------------------------------------------------------------------
def _dense_arguments():
    """Every exponent boundary (and its neighbours) of both signs, +-1, +-0, the denormals' ends, and a stride through the rest."""
    bits = [0x00000000, 0x00000001, 0x00000002, 0x007FFFFF, 0x00800000, 0x3F7FFFFF, 0x3F800000, 0x3F000000, 0x3EFFFFFF, 0x3F000001]
    for e in range(1, 128):
        bits += [(e << 23) - 1, e << 23, (e << 23) + 1]
    pos = np.unique(np.concatenate([np.array(bits, np.uint64), np.arange(0, 0x3F800000, 4099, dtype=np.uint64),
                                    np.arange(0x3E800000, 0x3F800001, 257, dtype=np.uint64)]))
    pos = pos[pos <= 0x3F800000].astype(np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000)]).view(F)


def test_soft_acos_is_within_its_derived_bound(sk):
    x = _dense_arguments()
    bound = SR.acos_bound(sk)
    assert bound == 5.5 * 2.0 ** -24
    got = SR.acos(sk, x).astype(np.float64)
    err = np.abs(got - np.arccos(x.astype(np.float64)))
    worst = int(np.argmax(err))
    print(f"soft acos: {x.size} arguments, max |error| {err[worst]:.4g} = {err[worst] * 2 ** 24:.3f} * 2^-24 at {float(x[worst]).hex()} (bound {bound:.4g})")
    assert err.max() <= bound
    pos, neg = x > 0.5, x < -0.5                                              # the per-branch figures of the derivation
    assert err[pos].max() <= 1.93 * 2.0 ** -24 and err[~pos & ~neg].max() <= 3.36 * 2.0 ** -24 and err[neg].max() <= 5.4 * 2.0 ** -24
    assert sk.sk_acos(1.0) == 0.0 and _bits(sk.sk_acos(-1.0)) == 0x40490FDB and _bits(sk.sk_acos(0.0)) == _bits(sk.sk_acos(-0.0)) == 0x3FC90FDB
    # the C driver's routine (every binary32 of a range) agrees on a window around the worst arguments of the full run
    for lo in (0x3EFF0000, 0xBF000000):
        window = np.arange(lo, lo + 0x20000, dtype=np.uint32).view(F)
        e = np.abs(SR.acos(sk, window).astype(np.float64) - np.arccos(window.astype(np.float64))).max()
        c = sk.sk_acos_max_error(lo, lo + 0x1FFFF, None)                      # libm's acos and numpy's differ in the last place of a double
        assert abs(c - e) <= 1e-15 and c <= bound


def test_soft_acos_outside_its_domain_is_nan(sk):
    bad = np.array([1.0000001, -1.0000001, 2.0, -2.0, 1e30, -1e30, np.inf, -np.inf, np.nan, -np.nan], F)
    assert np.all(np.isnan(SR.acos(sk, bad)))
    assert np.all(np.isnan(SR.acos(sk, np.array([0x7F800001, 0xFFC00000, 0x3F800001, 0xBF800001], np.uint32).view(F))))


# ---- the pass ------------------------------------------------------------------------------------------------------------------
def test_written_iff_depth_is_at_most_zero(sk):
    k = SR.block(SR.CONFIGS[0], W, H, 0.5)
    sky_all = SR.sky_pass(sk, k, np.zeros((H, W), F))
    assert not np.any(sky_all == SR.SENTINEL)
    for name, depth in SR.depth_images(W, H).items():
        out = SR.sky_pass(sk, k, depth)
        with np.errstate(invalid="ignore"):
            written = depth <= 0.0
        assert np.array_equal(out == SR.SENTINEL, ~written), name
        assert np.array_equal(out[written], sky_all[written]), name
    mix = SR.depth_images(W, H)["mix"]
    assert {0x00000000, 0x80000000, 0x00000001, 0x7FC00000, 0x7F800000} <= set(mix.view(np.uint32).ravel().tolist())


@pytest.mark.parametrize("config", range(len(SR.CONFIGS)))
def test_radiometric_accuracy_against_float64(sk, config):
    """From the binary32 V the pass computes, the shader's formula in float64 against the binary32 RGB of sky_ref.c, within the
    bound derived there, which scales with the sum of the magnitudes of the terms.  Measured (all configurations, both pitches and
    the camera looking down): the largest error is 0.364 of the bound (configuration 1) and 3.43e-6 of the scale S (configuration 2); the
    bound is widest near the sun, where dot3's rounding moves acos most."""
    worst_ratio = worst_scaled = 0.0
    bound = SR.acos_bound(sk)
    for pitch, down in ((0.0, False), (0.5, False), (0.0, True)):
        k = SR.block(SR.CONFIGS[config], W, H, pitch, down=down)
        _, rgb, V = SR.sky_pass(sk, k, np.zeros((H, W), F), want_rgb=True, want_view=True)
        want, tol, scale = SR.radiance64(k, V.reshape(-1, 3), bound)
        got = rgb.reshape(-1, 3).astype(np.float64)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)), (config, pitch)
        err = np.abs(got - want)
        worst_ratio, worst_scaled = max(worst_ratio, float((err / tol).max())), max(worst_scaled, float((err / scale).max()))
        assert np.all(err <= tol), (config, pitch, float((err / tol).max()))
    print(f"config {config}: max error / bound {worst_ratio:.3f}, max error / S {worst_scaled:.3g}")


def test_value_spread_of_the_configurations(sk):
    """What the GPU tests rely on, in float64 for the 67 x 35 image with yfov 1.0 at pitch 0 and 0.5: the first five configurations
    stay inside the format (no negative channel, none at 65024); the two with the sun at or below the horizon have Z of order 1e4
    and at most 10 % of their channel values at either clamp."""
    bound = SR.acos_bound(sk)
    for i, config in enumerate(SR.CONFIGS):
        for pitch in SR.PITCHES:
            k = SR.block(config, W, H, pitch)
            V = SR.sky_pass(sk, k, np.zeros((H, W), F), want_view=True)[1]
            rgb, _, _ = SR.radiance64(k, V.reshape(-1, 3), bound)
            neg, sat = float((rgb < 0).mean()), float((rgb >= 65024.0).mean())
            if i < 5:
                assert neg == 0.0 and sat == 0.0, (i, pitch, neg, sat)
            else:
                z = np.abs(k["m_HosekParams"]["m_Params"][0, 9, :3])
                assert np.all(z > 5e3) and np.all(z < 5e4), z
                assert neg <= 0.10 and sat <= 0.10, (i, pitch, neg, sat)       # measured worst: 4.9 % negative, 9.1 % saturated


def test_special_directions_of_the_reference(sk):
    """V equal to the float sun direction: dot3 of the unit vector with itself decides between NaN and a finite value; both are
    pinned here by the arithmetic.  V.y = 0, gamma > 90 degrees, a small positive cos gamma."""
    k = SR.block(SR.CONFIGS[0], W, H)
    found_nan = found_finite = False
    rng = np.random.default_rng(11)
    for _ in range(4000):
        s = SR.unit(rng.normal(size=3) + np.array([0.0, 1.0, 0.0]))
        k["m_SunLightDir"] = s
        d = I.fmaf(s[2], s[2], I.fmaf(s[1], s[1], F(s[0] * s[0])))
        rgb = SR.radiance(sk, k, s)
        if d > F(1.0):
            assert np.all(np.isnan(rgb)), (s, d)
            found_nan = True
        else:
            assert np.all(np.isfinite(rgb)) and np.all(rgb >= 0.5 * 0.999), (s, d, rgb)     # the disc term alone is 0.5 cg^256, cg within 2^-23 of 1
            found_finite = True
    assert found_nan and found_finite
    k = SR.block(SR.CONFIGS[0], W, H)
    sun = k["m_SunLightDir"][0]
    below = SR.radiance(sk, k, SR.unit((0.3, -0.4, -1.0)))                    # V.y < 0 clamps to the horizon's value
    level = SR.radiance(sk, k, np.array([SR.unit((0.3, -0.4, -1.0))[0], 0.0, SR.unit((0.3, -0.4, -1.0))[2]], F))
    assert np.all(np.isfinite(below)) and np.all(np.isfinite(level))
    away = -sun                                                               # gamma = 180 degrees: no disc term, acos(-1) = RN(pi)
    assert np.all(np.isfinite(SR.radiance(sk, k, away)))
    tiny = SR.unit(np.cross(sun.astype(np.float64), (0.0, 0.0, 1.0)))         # perpendicular to the sun: cos gamma about 1e-8, its 256th power is 0
    cg = float(I.fmaf(tiny[2], sun[2], I.fmaf(tiny[1], sun[1], F(tiny[0] * sun[0]))))
    assert abs(cg) < 1e-6
    assert np.all(np.isfinite(SR.radiance(sk, k, tiny)))


def test_the_shader_is_registered_and_the_facade_exports_the_sky_calls():
    from toyrenderer_amd import host, rhi
    assert "sky_PS_HosekWilkieSky" in set(rhi.shader_names())
    lib = host.load()
    for name in ("trhost_load_sky_dataset", "trhost_set_sky", "trhost_get_sky_consts"):
        assert name in host.HOST_SYMBOLS and hasattr(lib, name)
    assert I.SkyPassParameters.itemsize == 256 and I.SkyPassParameters.fields["m_SunLightDir"][1] == 64
    assert I.SkyPassParameters.fields["m_CameraPosition"][1] == 80 and I.SkyPassParameters.fields["m_HosekParams"][1] == 96
