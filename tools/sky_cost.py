#!/usr/bin/env python3
"""Cost of the sky pass: FrameDriver(lighting=True, sky=...) on the generated city of tools/postprocess_cost.py at 3840x2160, steady
state.  Reported from the back-end profile: "sky_PS_HosekWilkieSky#main" per frame over the city (its sky and drawn pixel counts
printed), then the pass alone over an all-sky frame (depth all 0, its own command list, launched 20 times), next to the time its
bytes alone would take at the box's stream rate (tools/membw, given with --membw=GB/s): 4 B per drawn pixel (the depth word) plus
8 B per sky pixel (the depth word and the stored word).  The same for other builds of the back end given as --variant=NAME=PATH (a
libtrhip.so whose csrc/k_sky.hip was built with -DTR_SKY_EXPERIMENT_STORE_ONLY: loads and the store without the arithmetic;
-DTR_SKY_EXPERIMENT_HW_EXP: v_exp_f32 and approximate division, the negative control that must fail tests/test_gpu_sky.py).  Each
run is its own process and the builds alternate `rounds` times (default 3) in one call, so that the differences are taken on one
box in one state.  --dump saves LightingOutput, for counting the words a control changes (--compare=A.npz,B.npz prints the count).
The dataset is read from tests/golden/hosek_rgb.npz.
usage: python tools/sky_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...]
       python tools/sky_cost.py --child [--dump=FILE.npz] ...   one run in this process (TRHIP_LIB picks the build)
       python tools/sky_cost.py --compare=A.npz,B.npz"""
import os
import re

import numpy as np

import cost_common as cc

SKY = "sky_PS_HosekWilkieSky#main"
LABELS = ("city", "all sky")


def run(n: int, render, dump=None):
    from toyrenderer_amd import rhi, sky
    from toyrenderer_amd.frame import FrameDriver
    from toyrenderer_amd.rhi import CB, TEX_SRV, TEX_UAV
    c = cc.city(n, render)
    dev, gs = c.dev, c.gs
    sun = np.array([0.3, 0.8, -0.52], np.float64)
    sun = tuple(float(x) for x in (sun / np.linalg.norm(sun)).astype(np.float32))
    dataset = sky.HosekDataset.load(os.path.join(cc.ROOT, "tests", "golden", "hosek_rgb.npz"))
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=(sun, 3.0), camera_origin=(0.0, 0.0, 0.0), sky=(dataset,))
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    depth, out = drv.depth.download_mip(0), drv.lighting_output.download_mip(0)
    nsky = int(np.count_nonzero(depth <= 0))
    print(f"{len(c.inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {nsky} sky pixels, {depth.size - nsky} drawn pixels, "
          f"LightingOutput checksum {int(out.astype(np.uint64).sum()):#x}")
    print(f"  {'city':20s} {prof[SKY][1] / frames * 1e3:9.1f} us per frame")
    if dump:
        np.savez(dump, lighting_output=out)
    cl = dev.create_command_list()                  # the pass alone over an all-sky frame
    zero = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R32_FLOAT, "all sky")
    zero.upload_mip(0, np.zeros((render[1], render[0]), np.float32))
    cl.open()
    cb = cl.constant_buffer(drv.sky_consts, "SkyPassParameters")
    cl.dispatch("sky_PS_HosekWilkieSky", [CB(0, cb), TEX_SRV(0, zero), TEX_UAV(0, drv.lighting_output, 0)], ((render[0] + 7) // 8, (render[1] + 7) // 8, 1))
    cl.close()
    cnt, ms = cc.steady_profile(dev, lambda: dev.execute(cl), warmup=3)[SKY]
    print(f"  {'all sky':20s} {ms / cnt * 1e3:9.1f} us per launch")
    cl.release(); zero.release(); drv.release(); gs.release()
    dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    if opt("compare"):
        a, b = (np.load(p) for p in opt("compare").split(","))
        print(f"LightingOutput words that differ: {int(np.count_nonzero(a['lighting_output'] != b['lighting_output']))} of {a['lighting_output'].size}")
    elif "--child" in opts:
        run(n, render, opt("dump"))
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = cc.variants(opts)
        outs = cc.alternate(__file__, builds, rounds, [n, *render])
        nsky, ndrawn = (int(x) for x in re.search(r"(\d+) sky pixels, (\d+) drawn pixels", outs[builds[-1][0]][-1]).groups())
        nbytes = {"city": 4 * ndrawn + 8 * nsky, "all sky": 8 * render[0] * render[1]}
        for k in LABELS:
            print(f"{k}: {nbytes[k] / 1e6:.2f} MB" + cc.stream_bound(nbytes[k], membw))
            for name, _ in builds:
                t = cc.figures(outs[name], r"^\s+" + re.escape(k) + r"\s+([0-9.]+) us", re.M)
                print(f"  {name:10s}: {cc.spread(t)}")
