#!/usr/bin/env python3
"""Cost of probe variability: FrameDriver(lighting=True, ddgi=..., ddgi_update=dict(variability=...)) on the generated city of
tools/ddgi_update_cost.py, record() and run() per frame (the option needs a recording per frame), from the back-end profile:
the radiance blend without u4 ("off") and with it ("on": threshold 0, which never converges), each reduction pass, the host's wait
in the read-back's read, and the frame's DDGI share (refit, trace, blends, reductions) before and after convergence at the
reference's threshold 0.001, with the update call at which the city converged, if it did within --calls (default 150).
Each run is its own process and the builds (the product, and any other libtrhip.so given as --variant=NAME=PATH; one from before
the feature runs "off" alone) alternate `rounds` times (default 3) in one call.
usage: python tools/ddgi_variability_cost.py [num_spheres] [width height] [--rounds=N] [--calls=N] [--variant=NAME=PATH ...]
       python tools/ddgi_variability_cost.py --child ...   one run in this process (TRHIP_LIB picks the build)"""
import re
import time

import numpy as np

import cost_common as cc

BLEND = "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1#main"
REDUCTION, EXTRA = "ReductionCS_DDGIReductionCS REDUCTION=1#main", "ReductionCS_DDGIExtraReductionCS#main"
SHARE = ("raytracing_CS_RefitTLAS#main", "giprobetrace_CS_ProbeTrace#main", BLEND, "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0#main", REDUCTION, EXTRA)


def run(n: int, render, calls: int):
    from toyrenderer_amd import ddgi, rhi
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render, raytracing=True)
    dev, gs, inst = c.dev, c.gs, c.inst
    pos = inst["m_WorldMatrix"][:, 3, :3].astype(np.float64)
    lo, hi = pos.min(0) - 1.0, pos.max(0) + 1.0
    centre, ext = (lo + hi) * 0.5, (hi - lo) * 0.5
    has = "ReductionCS_DDGIReductionCS REDUCTION=1" in set(rhi.shader_names())
    waits = []

    def driver(**settings):
        vol = ddgi.Volume.for_scene(centre, ext, float(np.linalg.norm(ext)), relocation=False, classification=False).reset()
        return FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=((0.2, 0.35, -0.9), 2.5), camera_origin=(0.0, 0.0, 0.0),
                           ddgi=vol, ddgi_update=dict(seed=1, max_ray_distance=float(np.linalg.norm(ext)), **settings))

    def frame(drv):
        drv.record(); drv.run()

    def timed_read(drv):
        read = drv.ddgi_variability_readback.read

        def wrapped(*a, **kw):
            t0 = time.perf_counter()
            out = read(*a, **kw)
            waits.append((time.perf_counter() - t0) * 1e6)
            return out
        drv.ddgi_variability_readback.read = wrapped

    def report(label, prof, frames):
        share = sum(prof.get(op, (0, 0.0))[1] for op in SHARE) / frames * 1e3
        print(f"  {label:10s} radiance blend {prof.get(BLEND, (0, 0.0))[1] / frames * 1e3:8.1f} us, first reduction {prof.get(REDUCTION, (0, 0.0))[1] / frames * 1e3:6.1f} us, "
              f"extra reduction {prof.get(EXTRA, (0, 0.0))[1] / frames * 1e3:6.1f} us ({prof.get(EXTRA, (0, 0))[0] // frames} launches), DDGI share {share:9.1f} us per frame")

    frames = cc.FRAMES
    drv = driver()
    probes = int(np.prod(drv.ddgi.counts))
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames per figure, {probes} probes, {probes * 36} variability texels")
    report("off", cc.steady_profile(dev, lambda: frame(drv)), frames)
    drv.release()
    if has:
        drv = driver(variability=True, variability_threshold=0.0)
        timed_read(drv)
        report("on", cc.steady_profile(dev, lambda: frame(drv)), frames)
        w = np.asarray(waits[-frames:])
        print(f"  read-back  host wait in read: median {np.median(w):6.1f} us, max {w.max():6.1f} us over {len(w)} reads (two calls behind the copy)")
        drv.release()
        drv = driver(variability=True, variability_threshold=0.001)
        at = None
        for call in range(1, calls + 1):
            frame(drv)
            if drv.ddgi_variability["converged"]:
                at = call
                break
        v = drv.ddgi_variability
        if at is None:
            print(f"  converge   the city did NOT converge at 0.001 within {calls} update calls: stddev {v['stddev']:.3e}, last average {v['average']:.3e}")
        else:
            print(f"  converge   the city converged at 0.001 at update call {at}: stddev {v['stddev']:.3e}, last average {v['average']:.3e}")
            report("converged", cc.steady_profile(dev, lambda: frame(drv)), frames)
        drv.release()
    gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    calls = int(opt("calls", 150))
    if "--child" in opts:
        run(n, render, calls)
    else:
        rounds = int(opt("rounds", 3))
        builds = cc.variants(opts)
        outs = cc.alternate(__file__, builds, rounds, [n, *render, f"--calls={calls}"], timeout=900)
        for name, *_ in builds:
            for label, what in (("off", "radiance blend"), ("on", "radiance blend"), ("on", "first reduction"), ("on", "extra reduction"), ("off", "DDGI share"), ("on", "DDGI share"),
                                ("converged", "DDGI share")):
                got = [m.group(1) for m in (re.search(rf"^\s+{label}\s.*{what}\s+([0-9.]+) us", out, re.M) for out in outs[name]) if m]
                if got:
                    print(f"{name:10s} {label:10s} {what:16s}: {cc.spread([float(g) for g in got])}")
