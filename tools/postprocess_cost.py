#!/usr/bin/env python3
"""Cost of auto exposure and tone mapping: FrameDriver(post=True) on the generated city of tools/lighting_cost.py at 3840x2160,
steady state, the three kernels per frame from the back-end profile ("adaptluminance_CS_GenerateLuminanceHistogram#main",
"adaptluminance_CS_AdaptExposure#main", "postprocess_PS_PostProcess#main"), next to the time each pass's bytes alone would take at
the box's stream rate (tools/membw, given with --membw=GB/s) and next to other builds of the back end given as --variant=NAME=PATH
(a libtrhip.so built with -DTR_HISTOGRAM_EXPERIMENT_REFERENCE_SHAPE: one 16 x 16 group per tile and 256 global adds each;
-DTR_HISTOGRAM_PER_WAVE=0|1 and -DTR_HISTOGRAM_MERGE_LANES=0|1: a private LDS sub-histogram per wave or one per workgroup, equal bins of
neighbouring lanes merged before the add or not;
-DTR_POST_EXPERIMENT_STORE_ONLY: the post pass's loads and store without its arithmetic; -DTR_POST_EXPERIMENT_HW_LOGEXP and
-DTR_POST_EXPERIMENT_TRUNC_STORE: the negative controls).  With --one-value the histogram pass is also timed on an image of one
value, the worst case for same-address LDS adds.  Each run is its own process and the builds alternate `rounds` times (default 3)
in one call, so that the differences are taken on one box in one state.  --dump saves back buffer and histogram, for counting the
words a control changes.
usage: python tools/postprocess_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...] [--one-value] [--bloom]
       python tools/postprocess_cost.py --child [--dump=FILE.npz] ...   one run in this process (TRHIP_LIB picks the build)"""
import re

import numpy as np

import cost_common as cc

KERNELS = ("adaptluminance_CS_GenerateLuminanceHistogram#main", "adaptluminance_CS_AdaptExposure#main", "postprocess_PS_PostProcess#main")


def run(n: int, render, one_value: bool, bloom_on: bool, dump=None):
    from toyrenderer_amd import interop as I
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver
    from toyrenderer_amd.rhi import PUSH, TEX_SRV, UAV
    c = cc.city(n, render)
    dev, gs = c.dev, c.gs
    bloom = None
    if bloom_on:
        bloom = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R11G11B10_FLOAT, "Bloom")
        bloom.upload_mip(0, (c.rng.integers(0, 16 << 6, (render[1], render[0])) * (1 | 1 << 11)).astype(np.uint32))
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, post=True, dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0),
                      bloom=(bloom, 0.1))
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run, settle=drv.reset_exposure)
    back, hist = drv.back_buffer.download_mip(0), drv.histogram.download(np.uint32, 256)
    print(f"{len(c.inst)} instances, render {render[0]}x{render[1]}, {frames} frames, bloom {'bound' if bloom_on else 'unbound'}, {int(np.count_nonzero(hist))} bins used, "
          f"largest bin {int(hist.max())}, back buffer checksum {int(back.astype(np.uint64).sum()):#x}, luminance {float(drv.luminance.download(np.float32, 1)[0]):.6f}")
    for name in KERNELS:
        cnt, ms = prof[name]
        print(f"  {name:55s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    if dump:
        np.savez(dump, back=back, hist=hist)
    if one_value:                                   # the histogram pass alone on an image of one value: every add of a wave goes to one LDS word
        tex = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R11G11B10_FLOAT, "one value")
        tex.upload_mip(0, np.full((render[1], render[0]), (14 << 6) | (14 << 6) << 11 | (14 << 5) << 22, np.uint32))
        hk = np.zeros(1, I.GenerateLuminanceHistogramParameters)
        lo, hi = I.log_luminance_range(0.004, 12.0)
        hk["m_SrcColorDims"] = render; hk["m_MinLogLuminance"] = lo; hk["m_InverseLogLuminanceRange"] = np.float32(1.0) / np.float32(hi - lo)
        cl = dev.create_command_list()
        cl.open()
        cl.dispatch(KERNELS[0].split("#")[0], [PUSH(0), TEX_SRV(0, tex), UAV(0, drv.histogram)], ((render[0] + 15) // 16, (render[1] + 15) // 16, 1), push=hk)
        cl.close()
        cnt, ms = cc.steady_profile(dev, lambda: dev.execute(cl))[KERNELS[0]]
        print(f"  {'one value: ' + KERNELS[0]:55s} {ms / frames * 1e3:9.1f} us per launch")
        cl.release(); tex.release()
    drv.release(); gs.release()
    if bloom is not None:
        bloom.release()
    dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    one_value, bloom_on = "--one-value" in opts, "--bloom" in opts
    if "--child" in opts:
        run(n, render, one_value, bloom_on, opt("dump"))
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = cc.variants(opts)
        labels = list(KERNELS) + (["one value: " + KERNELS[0]] if one_value else [])
        outs = cc.alternate(__file__, builds, rounds, [n, *render] + [o for o in ("--one-value", "--bloom") if o in opts])
        for k in labels:
            print(k)
            for name, _ in builds:
                t = cc.figures(outs[name], re.escape(k) + r"\s+([0-9.]+) us")
                print(f"  {name:10s}: {cc.spread(t)}")
        px = render[0] * render[1]
        for what, nbytes in (("histogram: 4 B read per pixel", 4 * px), (f"post: {'12' if bloom_on else '8'} B per pixel (colour{', bloom' if bloom_on else ''}, store)", (12 if bloom_on else 8) * px)):
            print(f"bytes moved, {what}: {nbytes / 1e6:.1f} MB" + cc.stream_bound(nbytes, membw, ": ", "; stream rate not given (--membw), bound not computed"))
