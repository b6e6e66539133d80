#!/usr/bin/env python3
"""Cost of the bloom chain: FrameDriver(post=True, bloom_mips=6) on the generated city of tools/postprocess_cost.py at 3840x2160,
steady state.  Reported per frame from the back-end profile: the chain ("bloom_PS_Downsample#main" + "bloom_PS_Upsample#main", all
2 * (mips - 1) launches) and the post pass that reads it; then every pass alone (its own command list, launched 20 times), next to
the time its bytes alone (the source mip read once, the destination mip written once) would take at the box's stream rate
(tools/membw, given with --membw=GB/s); and the same for other builds of the back end given as --variant=NAME=PATH (a libtrhip.so
whose csrc/k_bloom.hip was built with -DTR_BLOOM_LDS_DOWNSAMPLE=1: the downsample staged through LDS;
-DTR_BLOOM_EXPERIMENT_STORE_ONLY: loads and store without the arithmetic; -DTR_BLOOM_EXPERIMENT_FIXED_POINT and -ffp-contract=fast:
the negative controls).  Each run is its own process and the builds alternate `rounds` times (default 3) in one call, so that the
differences are taken on one box in one state.  --dump saves bloom mip 0 and the back buffer, for counting the words a control
changes (--compare=A.npz,B.npz prints the counts).
usage: python tools/bloom_cost.py [num_spheres] [width height] [--mips=N] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...]
       python tools/bloom_cost.py --child [--dump=FILE.npz] ...   one run in this process (TRHIP_LIB picks the build)
       python tools/bloom_cost.py --compare=A.npz,B.npz"""
import re

import numpy as np

import cost_common as cc

CHAIN = ("bloom_PS_Downsample#main", "bloom_PS_Upsample#main")
POST = "postprocess_PS_PostProcess#main"


def passes(render, mips):
    """(label, shader, source mip, destination mip) in the renderer's order."""
    n = mips - 1
    out = [(f"down {i}->{i + 1}", "bloom_PS_Downsample", i, i + 1) for i in range(n)]
    return out + [(f"up {n - i}->{n - i - 1}", "bloom_PS_Upsample", n - i, n - i - 1) for i in range(n)]


def run(n: int, render, mips: int, dump=None):
    from toyrenderer_amd.frame import FrameDriver
    from toyrenderer_amd.rhi import PUSH, SAMPLER, TEX_SRV, TEX_UAV
    c = cc.city(n, render)
    dev, gs = c.dev, c.gs
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, post=True, dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0),
                      bloom_mips=mips)
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run, settle=drv.reset_exposure)
    back, bloom0 = drv.back_buffer.download_mip(0), drv.download_bloom(0)
    print(f"{len(c.inst)} instances, render {render[0]}x{render[1]}, {mips} mips, {frames} frames, bloom mip 0 checksum {int(bloom0.astype(np.uint64).sum()):#x}, "
          f"back buffer checksum {int(back.astype(np.uint64).sum()):#x}")
    chain = sum(prof[name][1] for name in CHAIN) / frames * 1e3
    print(f"  {'chain':20s} {chain:9.1f} us per frame ({sum(prof[name][0] for name in CHAIN) // frames} launches)")
    print(f"  {'post':20s} {prof[POST][1] / frames * 1e3:9.1f} us per frame")
    if dump:
        np.savez(dump, back=back, bloom0=bloom0)
    cl = dev.create_command_list()
    for label, shader, sm, dm in passes(render, mips):   # every pass alone, on the textures the frames left behind
        at = [p[0] for p in passes(render, mips)].index(label)
        k = drv.bloom_consts[at:at + 1]
        src = TEX_SRV(0, drv.lighting_output) if (shader.endswith("Downsample") and sm == 0) else TEX_SRV(0, drv.bloom_texture, sm)
        w, h = render[0] >> dm, render[1] >> dm
        cl.open()
        cl.dispatch(shader, [PUSH(0), src, TEX_UAV(0, drv.bloom_texture, dm), SAMPLER(0)], ((w + 7) // 8, (h + 7) // 8, 1), push=k)
        cl.close()
        cnt, ms = cc.steady_profile(dev, lambda: dev.execute(cl), warmup=3)[shader + "#main"]
        print(f"  {label:20s} {ms / cnt * 1e3:9.1f} us per launch")
    cl.release(); drv.release(); gs.release()
    dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    mips = int(opt("mips", 6))
    if opt("compare"):
        a, b = (np.load(p) for p in opt("compare").split(","))
        for key, what in (("bloom0", "bloom mip 0"), ("back", "back buffer")):
            print(f"{what} words that differ: {int(np.count_nonzero(a[key] != b[key]))} of {a[key].size}")
    elif "--child" in opts:
        run(n, render, mips, opt("dump"))
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = cc.variants(opts)
        labels = ["chain", "post"] + [p[0] for p in passes(render, mips)]
        outs = cc.alternate(__file__, builds, rounds, [n, *render, f"--mips={mips}"])
        texels = lambda m: (render[0] >> m) * (render[1] >> m)                                                          # noqa: E731
        nbytes = {p[0]: 4 * (texels(p[2]) + texels(p[3])) for p in passes(render, mips)}
        nbytes["chain"] = sum(nbytes.values())
        for k in labels:
            print(k + (f": {nbytes[k] / 1e6:.2f} MB" + cc.stream_bound(nbytes[k], membw) if k in nbytes else ""))
            for name, _ in builds:
                t = cc.figures(outs[name], r"^\s+" + re.escape(k) + r"\s+([0-9.]+) us", re.M)
                print(f"  {name:10s}: {cc.spread(t)}")
