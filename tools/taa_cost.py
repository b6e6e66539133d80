#!/usr/bin/env python3
"""Cost of the temporal resolve: FrameDriver(post=True, taa={...}) on the generated city of tools/postprocess_cost.py at 3840x2160,
steady state with the jitter advancing every frame.  Reported from the back-end profile: "taa_CS_TemporalResolve#main" and the post
pass per frame of the whole frame; then the resolve alone (its own command list on the textures the frames left behind, launched
20 times), next to the time its own bytes (4 colour + 4 depth + 4 motion + 8 history read, 8 history + 4 colour written per
texel) would take at the box's stream rate (tools/membw, given with --membw=GB/s); and the same for other builds of the back end
given as --variant=NAME=PATH (a libtrhip.so whose csrc/k_taa.hip was built with -DTR_TAA_LDS=1: the window staged through LDS;
-DTR_TAA_EXPERIMENT_STORE_ONLY: the pass's loads and stores without its window or arithmetic, the floor).  Each run is its own
process and the builds alternate `rounds` times (default 3) in one call, so that the differences are taken on one box in one
state.  The product's and the LDS build's outputs are summed into checksums that must agree.
usage: python tools/taa_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...]
       python tools/taa_cost.py --child ...   one run in this process (TRHIP_LIB picks the build)"""
import re

import numpy as np

import cost_common as cc

TAA = "taa_CS_TemporalResolve#main"
POST = "postprocess_PS_PostProcess#main"
BYTES_PER_TEXEL = 4 + 4 + 4 + 8 + 8 + 4


def run(n: int, render):
    from toyrenderer_amd.frame import FrameDriver
    from toyrenderer_amd.rhi import PUSH, SAMPLER, TEX_SRV, TEX_UAV
    c = cc.city(n, render)
    dev, gs = c.dev, c.gs
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, post=True, dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0),
                      taa=dict(min_blend=0.1, max_sample_count=64, jitter=True))
    frames = cc.FRAMES

    def frame():                                     # every frame is recorded anew: its jitter and its history textures differ
        drv.record(); drv.run()
        drv.frame_counter += 1
    prof = cc.steady_profile(dev, frame, settle=drv.reset_exposure)
    aa, hist = drv.download_anti_aliased_output(), drv.download_taa_history().view(np.uint16)
    print(f"{len(c.inst)} instances, render {render[0]}x{render[1]}, {frames} frames, anti-aliased output checksum {int(aa.astype(np.uint64).sum()):#x}, "
          f"history checksum {int(hist.astype(np.uint64).sum()):#x}")
    print(f"  {'resolve in frame':20s} {prof[TAA][1] / frames * 1e3:9.1f} us per frame")
    print(f"  {'post':20s} {prof[POST][1] / frames * 1e3:9.1f} us per frame")
    cl = dev.create_command_list()                   # the resolve alone, on the textures the frames left behind
    read, write = drv.taa_history[drv.taa_written], drv.taa_history[1 - drv.taa_written]
    cl.open()
    cl.dispatch("taa_CS_TemporalResolve", [PUSH(0), TEX_SRV(0, drv.lighting_output), TEX_SRV(1, drv.depth), TEX_SRV(2, drv.motion), TEX_SRV(3, read), TEX_UAV(0, write, 0),
                                           TEX_UAV(1, drv.anti_aliased_output, 0), SAMPLER(0)], ((render[0] + 7) // 8, (render[1] + 7) // 8, 1), push=drv.taa_consts)
    cl.close()
    cnt, ms = cc.steady_profile(dev, lambda: dev.execute(cl), warmup=3)[TAA]
    print(f"  {'resolve alone':20s} {ms / cnt * 1e3:9.1f} us per launch")
    cl.release(); drv.release(); gs.release()
    dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    if "--child" in opts:
        run(n, render)
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = cc.variants(opts)
        outs = cc.alternate(__file__, builds, rounds, [n, *render])
        nbytes = BYTES_PER_TEXEL * render[0] * render[1]
        for k in ("resolve in frame", "resolve alone", "post"):
            print(k + (f": {nbytes / 1e6:.2f} MB" + cc.stream_bound(nbytes, membw) if k != "post" else ""))
            for name, _ in builds:
                t = cc.figures(outs[name], r"^\s+" + re.escape(k) + r"\s+([0-9.]+) us", re.M)
                print(f"  {name:10s}: {cc.spread(t)}")
        for name, _ in builds:
            print(f"  {name:10s}: " + re.search(r"anti-aliased output checksum \S+ history checksum \S+", outs[name][0]).group(0))
