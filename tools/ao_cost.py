#!/usr/bin/env python3
"""Cost of the ambient occlusion passes: FrameDriver(lighting=True, ao=...) on the generated city of tools/sky_cost.py at 3840x2160,
steady state.  Reported from the back-end profile, per frame: "ambientocclusion_CS_XeGTAO_PrefilterDepths#main",
"...MainPass DEBUG_OUTPUT_MODE=0#main" and "...Denoise#main" (all its dispatches together and per dispatch) for each quality level
with 3 denoise passes and for 1 to 3 denoise passes at Ultra, next to the time each kernel's bytes alone would take at the box's
stream rate (tools/membw, given with --membw=GB/s): prefilter 4 B read + 2 * (1 + 1/4 + 1/16 + 1/64 + 1/256) B written per pixel;
main 2 B (the centre) + 16 B (GBufferA) read and 2 B written per pixel, its 2-byte sample fetches counted apart (4 * slices * steps per
pixel, mostly cache hits: an upper figure); denoise 2 * 9 B gathered (an upper figure, neighbours share them) and 1 B written.
--insts=N (the main pass's SQ_INSTS_VALU of one Ultra frame, from a counter run of `--child` of its own) prints instructions per
pixel.  The same for other builds of the back end given as --variant=NAME=PATH (a libtrhip.so whose csrc/k_ambientocclusion.hip was
built with -DTR_AO_EXPERIMENT_HW_TRIG: v_sin_f32, v_cos_f32, v_log_f32 and v_exp_f32 in place of the software functions, the negative
control that must fail tests/test_gpu_ao.py).  Each run is its own process and the builds alternate `rounds` times (default 3).
usage: python tools/ao_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--insts=N] [--variant=NAME=PATH ...]
       python tools/ao_cost.py --child [--only=QUALITY,PASSES] ...   one run in this process (TRHIP_LIB picks the build)"""
import re

import numpy as np

import cost_common as cc

PREFILTER = "ambientocclusion_CS_XeGTAO_PrefilterDepths#main"
MAIN = "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0#main"
DENOISE = "ambientocclusion_CS_XeGTAO_Denoise#main"
CONFIGS = [(0, 3), (1, 3), (2, 3), (3, 3), (3, 1), (3, 2)]          # (quality, denoise passes)
SAMPLES = {0: 1 * 2, 1: 2 * 2, 2: 3 * 3, 3: 9 * 2}                  # slices * steps


def run(n, render, only=None):
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render)
    dev, gs = c.dev, c.gs
    frames = cc.FRAMES
    print(f"{len(c.inst)} instances, render {render[0]}x{render[1]}, {frames} frames per configuration")
    for quality, passes in ([only] if only else CONFIGS):
        drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, debug_mode=9, ao=dict(quality=quality, denoise_passes=passes))
        drv.record()
        prof = cc.steady_profile(dev, drv.run)
        ssao = drv.download_ssao()
        us = {k: prof[k][1] / frames * 1e3 for k in (PREFILTER, MAIN, DENOISE)}
        print(f"  quality {quality} passes {passes}: prefilter {us[PREFILTER]:8.1f} us, main {us[MAIN]:8.1f} us, denoise {us[DENOISE]:8.1f} us "
              f"({us[DENOISE] / max(1, passes):.1f} per dispatch); SSAO checksum {int(ssao.astype(np.uint64).sum()):#x}")
        drv.release()
    gs.release()
    dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    if "--child" in opts:
        run(n, render, tuple(int(x) for x in opt("only").split(",")) if opt("only") else None)
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = cc.variants(opts)
        outs = cc.alternate(__file__, builds, rounds, [n, *render])
        times = {name: {c: {k: [] for k in ("prefilter", "main", "denoise")} for c in CONFIGS} for name, _ in builds}
        for name, _ in builds:
            for m in re.finditer(r"quality (\d) passes (\d): prefilter\s+([0-9.]+) us, main\s+([0-9.]+) us, denoise\s+([0-9.]+) us", "".join(outs[name])):
                c = (int(m.group(1)), int(m.group(2)))
                for k, x in zip(("prefilter", "main", "denoise"), m.groups()[2:]):
                    times[name][c][k].append(float(x))
        px = render[0] * render[1]
        for c in CONFIGS:
            nbytes = {"prefilter": px * (4 + 2 * (1 + 1 / 4 + 1 / 16 + 1 / 64 + 1 / 256)), "main": px * (2 + 16 + 2), "denoise": max(1, c[1]) * px * (18 + 1)}
            print(f"quality {c[0]}, {c[1]} denoise passes (main pass sample fetches: {4 * SAMPLES[c[0]] * px / 1e6:.0f} MB more if none hit a cache):")
            for k in ("prefilter", "main", "denoise"):
                print(f"  {k}: {nbytes[k] / 1e6:.1f} MB" + cc.stream_bound(nbytes[k], membw))
                for name, _ in builds:
                    print(f"    {name:10s}: {cc.spread(times[name][c][k])}")
        if opt("insts"):
            print(f"main pass at Ultra: {float(opt('insts')) * 64 / px:.0f} VALU instructions per pixel (SQ_INSTS_VALU counts waves: x 64 lanes / {px} pixels)")
