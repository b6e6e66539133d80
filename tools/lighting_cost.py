#!/usr/bin/env python3
"""Cost of the deferred lighting pass: FrameDriver(lighting=True) on the generated city of tools/gbuffer_cost.py at 3840x2160,
steady state, "deferredlighting_PS_Main#main" per frame from the back-end profile, next to the time the pass's bytes alone
would take at the box's stream rate (tools/membw, given with --membw=GB/s) and next to other builds of the back end given as
--variant=NAME=PATH (a libtrhip.so built with -DTR_LIGHTING_TILE_W=16: the 16 x 4 wave mapping; one built with
-DTR_LIGHTING_EXPERIMENT_STORE_ONLY: the pass's loads and store without its arithmetic).  Each run is its own process and the
builds alternate `rounds` times (default 3) in one call, so that the differences are taken on one box in one state.
usage: python tools/lighting_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...] [--debug-mode=M]
       python tools/lighting_cost.py --child [--dump=FILE.npy] ...   one run in this process (TRHIP_LIB picks the build); --dump saves LightingOutput"""
import re

import numpy as np

import cost_common as cc

LIGHTING_US = r"deferredlighting_PS_Main\w*#main\s+([0-9.]+) us"


def run(n: int, render, debug_mode: int, dump=None):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render)
    dev, gs = c.dev, c.gs
    shadow = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R8_UNORM, "ShadowMask")
    shadow.upload_mip(0, c.rng.integers(0, 256, (render[1], render[0]), dtype=np.uint64).astype(np.uint8))
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, debug_mode=debug_mode,
                      dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0), shadow_mask=shadow)
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    lit = int(np.count_nonzero(drv.depth.download_mip(0) > 0))
    words = drv.lighting_output.download_mip(0)
    if dump:
        np.save(dump, words)
    print(f"{len(c.inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {lit} lit pixels of {render[0] * render[1]}, "
          f"output checksum {int(words.astype(np.uint64).sum()):#x}")
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("deferredlighting_PS_Main") or name.startswith("basepass_PS_Main"):
            print(f"  {name:45s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    drv.release(); shadow.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    debug_mode = int(opt("debug-mode", 0))
    if "--child" in opts:
        run(n, render, debug_mode, opt("dump"))
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = cc.variants(opts)
        outs = cc.alternate(__file__, builds, rounds, [f"--debug-mode={debug_mode}", n, *render])
        for name, _ in builds:
            print(f"{name:10s}: {cc.spread(cc.figures(outs[name], LIGHTING_US))}")
        lit = int(re.search(r"(\d+) lit pixels", outs[builds[-1][0]][-1]).group(1))
        nbytes = 4 * render[0] * render[1] + lit * (16 + 1 + 4)          # depth for every pixel; GBufferA, the shadow byte and the store for a lit one
        line = f"bytes moved: {nbytes / 1e6:.1f} MB ({lit} lit pixels x 21 B + {render[0] * render[1]} x 4 B of depth)"
        print(line + cc.stream_bound(nbytes, membw, ": ", "; stream rate not given (--membw), bound not computed"))
