#!/usr/bin/env python3
"""Cost of the DDGI probe update: FrameDriver(lighting=True, ddgi=..., ddgi_update={...}) on the generated city of
tools/lighting_cost.py, steady state, per update from the back-end profile: "giprobetrace_CS_ProbeTrace#main" and the two
"ProbeBlendingCS_DDGIProbeBlendingCS ...#main" ops, next to "raytracing_CS_RefitTLAS#main" and "deferredlighting_PS_Main#main" of the
same frames.  The volume is ddgi.Volume.for_scene of the city's box, cleared (Volume.reset); the command list is recorded once, so
every timed update runs with one rotation on a volume that has converged under it.  Each run is its own process and the builds
(the product, and any other libtrhip.so that knows the passes, given as --variant=NAME=PATH) alternate `rounds` times (default 3)
in one call.
usage: python tools/ddgi_update_cost.py [num_spheres] [width height] [--rounds=N] [--variant=NAME=PATH ...]
       python tools/ddgi_update_cost.py --child ...   one run in this process (TRHIP_LIB picks the build)"""
import numpy as np

import cost_common as cc

OPS = {"trace": "giprobetrace_CS_ProbeTrace#main", "radiance blend": "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1#main",
       "distance blend": "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0#main", "refit": "raytracing_CS_RefitTLAS#main",
       "lighting": "deferredlighting_PS_Main#main"}


def run(n: int, render):
    from toyrenderer_amd import ddgi
    from toyrenderer_amd import interop as I
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render, raytracing=True)
    dev, gs, inst = c.dev, c.gs, c.inst
    pos = inst["m_WorldMatrix"][:, 3, :3].astype(np.float64)                  # the scene's box, as tools/ddgi_cost.py takes it
    lo, hi = pos.min(0) - 1.0, pos.max(0) + 1.0
    centre, ext = (lo + hi) * 0.5, (hi - lo) * 0.5
    vol = ddgi.Volume.for_scene(centre, ext, float(np.linalg.norm(ext)), relocation=False, classification=False).reset()
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=((0.2, 0.35, -0.9), 2.5), camera_origin=(0.0, 0.0, 0.0),
                      ddgi=vol, ddgi_update=dict(seed=1, max_ray_distance=float(np.linalg.norm(ext))))
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    rays = drv.download_ddgi_rays()
    probes = int(np.prod(vol.counts))
    miss, back = int(np.count_nonzero(rays[..., 3] == np.float32(1e27))), int(np.count_nonzero(rays[..., 3] < 0))
    got = drv.download_ddgi()
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} updates, probes {vol.counts[0]}x{vol.counts[1]}x{vol.counts[2]} = {probes}, "
          f"{probes * I.kDDGIRaysPerProbe} rays: {miss} miss, {back} back faces, {rays[..., 3].size - miss - back} front faces; "
          f"irradiance checksum {int(got.irradiance.astype(np.uint64).sum()):#x}")
    for label, op in OPS.items():
        cnt, ms = prof[op]
        print(f"  {label:15s} {ms / frames * 1e3:10.1f} us per update ({cnt // frames} launches)")
    drv.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    if "--child" in opts:
        run(n, render)
    else:
        rounds = int(opt("rounds", 3))
        builds = cc.variants(opts)
        outs = cc.alternate(__file__, builds, rounds, [n, *render], timeout=600)
        for name, _ in builds:
            for label in OPS:
                pattern = label + r"\s+([0-9.]+) us per update"
                print(f"{name:10s} {label:15s}: {cc.spread(cc.figures(outs[name], pattern))}")
