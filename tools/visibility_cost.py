#!/usr/bin/env python3
"""Cost of the visibility buffer: the two-phase frame with self-rendered depth (FrameDriver(raster_depth=True), raster
"basepass_MS_Main_depth") against the same frame with FrameDriver(visibility=True) (raster "basepass_MS_Main_visibility"
plus the "basepass_PS_Main_motion" resolve), on a generated city at 3840x2160, steady state, per op from the back-end
profile.  Each mode runs in its own process.
usage: python tools/visibility_cost.py [num_spheres] [width height]"""
import os
import subprocess
import sys

import cost_common as cc


def run(mode: str, n: int, render):
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render, shading=False)
    dev, gs = c.dev, c.gs
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, raster_depth=True, visibility=(mode == "visibility"))
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    print(f"[{mode}] {len(c.inst)} instances, render {render[0]}x{render[1]}, {frames} frames")
    total = 0.0
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("basepass_MS_Main") or name.startswith("basepass_PS_Main"):
            us = ms / frames * 1e3
            total += us
            print(f"  {name:45s} {us:9.1f} us per frame ({cnt // frames} launches)")
    print(f"  {'raster + resolve':45s} {total:9.1f} us per frame")
    drv.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, _ = cc.parse_args()
    if opt("mode"):
        run(opt("mode"), n, render)
    else:
        for m in ("depth", "visibility"):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), f"--mode={m}", str(n), str(render[0]), str(render[1])])
