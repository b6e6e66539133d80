#!/usr/bin/env python3
"""Cost of the shadow denoiser: FrameDriver(lighting=True, shadows=dict(soft=True, ...), shadow_denoise={}) on the generated city of
tools/shadowmask_cost.py at 3840x2160, the frame counter (the noise phase and the tap rotation) advancing, every frame recorded anew.
Reported from the back-end profile, per frame, each timed `rounds` times (default 3) in this one process with the two drivers
alternated: the any-hit trace of a shadow_denoise=None driver ("shadowmask_CS_ShadowMask#main") beside the penumbra trace
("#penumbra": the closest-commit walk does not end early on occluded rays) and their ratio; the pack pass and the denoiser's four
dispatches, each next to the time its own bytes (what one texel reads and writes once, the tile bytes left out) would take to stream;
and the share of texels in filtered tiles, which is what the three filtering passes' time goes with.
usage: python tools/sigma_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GB/s]"""
import numpy as np

import cost_common as cc

TRACE = "shadowmask_CS_ShadowMask"
# op -> bytes per texel of its own: reads + writes
PASSES = {"shadowmask_CS_PackNormalAndRoughness#main": 16 + 4, "SIGMA_Shadow_ClassifyTiles.cs#main": 2 + 2 + 4, "SIGMA_Shadow_Blur.cs#main": 4 + 2 + 4 + 4 + 4,
          "SIGMA_Shadow_PostBlur.cs#main": 4 + 2 + 4 + 4 + 4, "SIGMA_Shadow_TemporalStabilization.cs#main": 4 + 2 + 4 + 2 + 2 + 1}


def main():
    n, render, opt, _ = cc.parse_args()
    rounds = int(opt("rounds", 3))
    membw = float(opt("membw", 0)) or None
    c = cc.city(n, render, raytracing=True)
    dev, gs = c.dev, c.gs
    from toyrenderer_amd.frame import FrameDriver
    noise = np.random.default_rng(1).integers(0, 256, (128, 128, 4), dtype=np.uint64).astype(np.uint8)
    common = dict(record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=((0.2, 0.35, -0.9), 2.5), shadows=dict(noise=noise, soft=True, ray_start_offset=0.1))
    raw, den = FrameDriver(dev, gs, c.view, **common), FrameDriver(dev, gs, c.view, shadow_denoise={}, **common)

    def frame(drv):
        def run():
            drv.frame_counter += 1
            drv.record(); drv.run()
        return run
    for drv in (raw, den):
        for _ in range(5):
            frame(drv)()
    dev.wait_idle()
    frames = cc.FRAMES
    rows = {k: [] for k in (TRACE + "#main", TRACE + "#penumbra", *PASSES)}
    for _ in range(rounds):
        for drv in (raw, den):
            prof = cc.profile(dev, frame(drv))
            for k in rows:
                if k in prof:
                    rows[k].append(prof[k][1] / frames * 1e3)
    texels = render[0] * render[1]
    tiles, depth, pen = den.download_shadow_tiles(), den.depth.download_mip(0), den.download_shadow_penumbra()
    t = tiles.astype(np.uint32)
    p = np.pad(t, 1, mode="edge")
    th, tw = t.shape
    near = np.zeros_like(t)
    for dy in range(3):
        for dx in range(3):
            near |= p[dy:dy + th, dx:dx + tw]
    traced = int(np.count_nonzero(depth != 0))
    print(f"{len(c.inst)} instances, render {render[0]}x{render[1]}: {traced} traced texels of {texels}, {np.count_nonzero(pen[depth != 0] < 0x7BFF) / max(traced, 1):.3f} occluded; "
          f"{np.count_nonzero(near == 3)} of {t.size} tiles filtered ({np.count_nonzero(t == 3)} hold both kinds themselves)")
    for k in (TRACE + "#main", TRACE + "#penumbra"):
        print(f"  {k:46s}: {cc.spread(rows[k])}")
    print(f"  penumbra trace / any-hit trace, medians: {np.median(rows[TRACE + '#penumbra']) / np.median(rows[TRACE + '#main']):.3f}")
    for k, nbytes in PASSES.items():
        print(f"  {k:46s}: {cc.spread(rows[k])}; its {nbytes * texels / 1e6:.0f} MB" + cc.stream_bound(nbytes * texels, membw))
    print(f"  the five dispatches behind the trace, sum of medians: {sum(np.median(rows[k]) for k in PASSES):.1f} us")
    raw.release(); den.release(); gs.release()
    dev.destroy()


if __name__ == "__main__":
    main()
