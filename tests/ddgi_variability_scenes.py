"""The inputs of the probe variability tests (tests/test_ddgi_variability_ref.py on the CPU, tests/test_gpu_ddgi_variability.py on the
GPU): the blend cases, whose every branch of the variability value the CPU test counts, and the reduction cases at the shapes where
the passes can go wrong.  No device, no reference library."""
import numpy as np

import ddgi_blend_scenes as BS
import ddgi_update_ref as DU
import ddgi_update_scenes as US
from toyrenderer_amd import interop as I

F = np.float32
RAYS = I.kDDGIRaysPerProbe

# ---- the blend: a 3 x 2 x 3 seeded volume ---------------------------------------------------------------------------------------------
BLEND_COUNTS = (3, 2, 3)
BLEND_INACTIVE = (4, 11)                          # switched off under the classification flag: left alone
BLEND_25_BACK, BLEND_DARK, BLEND_CLEARED = 6, 8, 2   # 25 back faces: left alone; radiance 0; one cleared texel in an ordinary probe
SENTINEL = F(-3.25)                               # pre-fill of the variability buffer: a left-alone probe's 36 values keep it


def blend_volume(name="default", seed=7):
    """"floor": floor_volume().  Else seeded codes and distances (DU.seeded_volume); probe BLEND_CLEARED's texel (2, 3) cleared to the zero word; the dark probe's
    tile holds small codes (0, 1 and 2 per channel, three texels cleared), so that the darker-step floor moves it and its eased
    luminance sits at or below one 10-bit code."""
    if name == "floor":
        return floor_volume()
    vol = DU.seeded_volume(BS._volume(BLEND_COUNTS), seed, inactive=BLEND_INACTIVE)
    BS.irradiance_tile(vol, BLEND_CLEARED)[3, 2] = 0
    rng = np.random.default_rng([seed, 99])
    dark = BS.irradiance_tile(vol, BLEND_DARK)
    dark[...] = BS.pack(rng.integers(0, 3, (6, 6, 3)))
    dark[0, :3] = 0
    return vol.fill_borders()


def blend_rays(name="default", seed=8):
    if name == "floor":
        return floor_rays()
    n = int(np.prod(BLEND_COUNTS))
    r = BS.base_rays(n, seed, back=0.05)
    r[BLEND_25_BACK, :, 3] = np.abs(r[BLEND_25_BACK, :, 3])
    r[BLEND_25_BACK, 10:35, 3] *= F(-0.2)
    r[BLEND_25_BACK, 10:35, :3] = 0.0
    r[BLEND_DARK, :, :3] = 0.0
    r[BLEND_DARK, :, 3] = np.abs(r[BLEND_DARK, :, 3])
    return r


# "floor": one probe whose every texel stores the codes (0, 1, 2), under rays of the constant radiance (R, 0, 0) and hysteresis 0.3
# with thresholds nothing reaches.  R (found by bisecting to the crossing and walking the floats around it) puts the eased value's
# luminance on 2^-10 EXACTLY in 14 of the 36 texels, with lumS2 > 0: the value is 0 by <=, and 1.3735857 where a < stands.
FLOOR_CODES, FLOOR_RADIANCE_BITS = (0, 1, 2), 0x2cc06687
LEFT_ALONE = {"default": 3, "settled": 3, "floor": 0}      # probes of the case that keep the sentinel


def floor_volume():
    vol = BS._volume((1, 1, 1))
    BS.irradiance_tile(vol, 0)[...] = BS.pack(np.broadcast_to(np.array(FLOOR_CODES), (6, 6, 3)))
    return vol.fill_borders()


def floor_rays():
    r = np.array([FLOOR_RADIANCE_BITS], np.uint32).view(F)[0]
    return BS.constant_rays(1, (r, 0.0, 0.0), 9)


# name -> settings of DU.consts.  "settled": hysteresis 0 and a brightness threshold nothing reaches: out = prev + (res - prev),
# which rounds to either side of res, so (res - prev) * (res - out) is a rounding error of either sign: negative lumS2.
BLEND_CONSTS = {"default": dict(), "settled": dict(hysteresis=0.0, irradiance_threshold=10.0, brightness_threshold=10.0),
                "floor": dict(hysteresis=0.3, irradiance_threshold=10.0, brightness_threshold=10.0)}


def blend_consts(name):
    return DU.consts(rotation=US.rotation(5), **BLEND_CONSTS[name])


# ---- the reductions ---------------------------------------------------------------------------------------------------------------------
# name -> (counts, which probes are inactive: a list, or "all")
REDUCTION_CASES = {
    "1x1x1": ((1, 1, 1), []),                     # 6 x 6 x 1: one partial group, no extra pass
    "3x2x3": ((3, 2, 3), [4, 11]),                # 18 x 18 x 2: partial in all three axes
    "3x5x1": ((3, 5, 1), [7]),                    # more than 4 planes: two groups in z
    "43x1x1": ((43, 1, 1), [0, 21, 42]),          # 258 wide: 17 groups, two extra passes
    "all inactive": ((3, 2, 3), "all"),           # average 0, weight 0
    "stale": ((3, 2, 3), [4, 11]),                # a NaN and an inf in the inactive probes' texels
    "tree": ((2, 3, 1), []),                      # 2^24, 1 and -2^24 where only the stated order gives 1 / 216
}


def reduction_case(name, seed=12):
    """(volume, variability float32 [cy, 6 cz, 6 cx])."""
    counts, inactive = REDUCTION_CASES[name]
    n = int(np.prod(counts))
    vol = DU.seeded_volume(BS._volume(counts), seed, inactive=range(n) if inactive == "all" else inactive)
    cx, cy, cz = counts
    rng = np.random.default_rng([seed, n])
    var = rng.uniform(0.0, 0.5, (cy, 6 * cz, 6 * cx)).astype(F)
    if name == "stale":
        var[0, 6:12, 6:12] = np.nan               # probe 4 = (1, 0, 1)
        var[1, 0:6, 12:18] = np.inf               # probe 11 = (2, 1, 0)
    if name == "tree":
        # thread t = tx + 4 ty + 32 tz of the one group: t = 0 covers x 0..3, y 0..1 of plane 0; t = 1 x 4..7; t = 64 plane 2.
        # Strides 64, 32, ..., 1: p[0] = 2^24 + -2^24 = 0 first, + 1 last: the sum is 1.  Strides ascending, or the threads in
        # sequence: 2^24 + 1 rounds back to 2^24 first and the sum is 0.
        var[...] = 0.0
        var[0, 0, 0], var[0, 0, 4], var[2, 0, 0] = F(2.0 ** 24), F(1.0), F(-(2.0 ** 24))
    return vol, var
