#!/usr/bin/env python3
"""Cost of the probe visualisation: FrameDriver(lighting=True, post=True, ddgi=..., probes=dict(radius=...)) on the generated city of
tools/lighting_cost.py, steady state, per frame from the back-end profile: "giprobevisualization_CS_LoadGIProbes#main",
"giprobevisualization_CS_VisualizeGIProbesCulling#main" and the draw's two launches "giprobevisualization_PS_VisualizeGIProbes#main"
and "#resolve" (csrc/k_giprobedraw.hip).  Two volumes over the city's box, a supplied one each (seeded irradiance, no probe update: the
three passes read the volume and do not care who filled it): 4 x 4 x 4 probes, the size of the Cornell tests' volume, and 32 x 8 x 32.
The radius is a tenth of the smallest spacing.  Each run is its own process and the two volumes alternate `rounds` times (default 3)
in one call.  This is a debug view: there is no gate, the figures are for the record (profiles/ddgi/README.md).
usage: python tools/ddgi_probe_draw_cost.py [num_spheres] [width height] [--rounds=N]
       python tools/ddgi_probe_draw_cost.py --child --counts=X,Y,Z ...   one run in this process"""
import numpy as np

import cost_common as cc

OPS = {"load probes": "giprobevisualization_CS_LoadGIProbes#main", "cull": "giprobevisualization_CS_VisualizeGIProbesCulling#main",
       "draw, main": "giprobevisualization_PS_VisualizeGIProbes#main", "draw, resolve": "giprobevisualization_PS_VisualizeGIProbes#resolve"}
VOLUMES = ("4,4,4", "32,8,32")


def run(n: int, render, counts):
    from toyrenderer_amd import ddgi
    from toyrenderer_amd import interop as I
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render)
    dev, gs, inst = c.dev, c.gs, c.inst
    pos = inst["m_WorldMatrix"][:, 3, :3].astype(np.float64)                  # the scene's box, as tools/ddgi_update_cost.py takes it
    lo, hi = pos.min(0) - 1.0, pos.max(0) + 1.0
    spacing = (hi - lo) / np.maximum(np.asarray(counts) - 1, 1)
    vol = ddgi.Volume((lo + hi) * 0.5, spacing, counts, normal_bias=0.1, view_bias=0.3)
    rng = np.random.default_rng(11)
    vol.irradiance[...] = ddgi.pack_unorm10(rng.uniform(0.05, 1.0, vol.irradiance.shape + (3,)))
    ddgi.fill_borders(vol.irradiance, I.kDDGIIrradianceInteriorTexels)
    radius = 0.1 * float(spacing.min())
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, post=True, dir_light=((0.2, 0.35, -0.9), 2.5), camera_origin=(0.0, 0.0, 0.0),
                      ddgi=vol, probes=dict(radius=radius))
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    count, _, _ = drv.download_probes()
    won = int(np.count_nonzero(drv.download_probe_winners()))
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, probes {counts[0]}x{counts[1]}x{counts[2]} = {int(np.prod(counts))}, radius {radius:.3f}: "
          f"{count} drawn, {won} texels won; back buffer checksum {int(drv.back_buffer.download_mip(0).astype(np.uint64).sum()):#x}")
    for label, op in OPS.items():
        cnt, ms = prof[op]
        print(f"  {label:15s} {ms / frames * 1e3:10.1f} us per frame ({cnt // frames} launches)")
    drv.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    if "--child" in opts:
        run(n, render, tuple(int(x) for x in opt("counts").split(",")))
    else:
        rounds = int(opt("rounds", 3))
        builds = [(v.replace(",", "x"), None, f"--counts={v}") for v in VOLUMES]
        outs = cc.alternate(__file__, builds, rounds, [n, *render], timeout=600)
        for name, *_ in builds:
            for label in OPS:
                pattern = label + r"\s+([0-9.]+) us per frame"
                print(f"{name:10s} {label:15s}: {cc.spread(cc.figures(outs[name], pattern))}")
