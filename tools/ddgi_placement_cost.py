#!/usr/bin/env python3
"""Cost of probe placement: FrameDriver(lighting=True, ddgi=..., ddgi_update=dict(relocate=True, classify=True, ...)) on the generated
city of tools/lighting_cost.py, steady state, per update from the back-end profile: "giprobetrace_CS_ProbeTraceFixedRays#main",
"ProbeRelocationCS_DDGIProbeRelocationCS#main" and "ProbeClassificationCS_DDGIProbeClassificationCS#main" next to
"giprobetrace_CS_ProbeTrace#main" of the same frames.  The volume is ddgi.Volume.for_scene of the city's box with both flags on,
cleared (Volume.reset); the command list is recorded once, so every update runs with one rotation.  The probes keep moving and
switching from update to update, so the probe trace's time is that of the probes still active: their count after the last update
is printed, and the fixed-ray trace's share is given against the trace's time scaled to all probes too.  Each run is its own
process and the builds (the product, and any other libtrhip.so that knows the passes, given as --variant=NAME=PATH) alternate
`rounds` times (default 3) in one call.
usage: python tools/ddgi_placement_cost.py [num_spheres] [width height] [--rounds=N] [--variant=NAME=PATH ...]
       python tools/ddgi_placement_cost.py --child ...   one run in this process (TRHIP_LIB picks the build)"""
import numpy as np

import cost_common as cc

OPS = {"probe trace": "giprobetrace_CS_ProbeTrace#main", "fixed-ray trace": "giprobetrace_CS_ProbeTraceFixedRays#main",
       "relocation": "ProbeRelocationCS_DDGIProbeRelocationCS#main", "classification": "ProbeClassificationCS_DDGIProbeClassificationCS#main"}


def run(n: int, render):
    from toyrenderer_amd import ddgi
    from toyrenderer_amd import interop as I
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render, raytracing=True)
    dev, gs, inst = c.dev, c.gs, c.inst
    pos = inst["m_WorldMatrix"][:, 3, :3].astype(np.float64)                  # the scene's box, as tools/ddgi_update_cost.py takes it
    lo, hi = pos.min(0) - 1.0, pos.max(0) + 1.0
    centre, ext = (lo + hi) * 0.5, (hi - lo) * 0.5
    radius = float(np.linalg.norm(ext))
    vol = ddgi.Volume.for_scene(centre, ext, radius, relocation=True, classification=True).reset()
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=((0.2, 0.35, -0.9), 2.5), camera_origin=(0.0, 0.0, 0.0),
                      ddgi=vol, ddgi_update=dict(seed=1, max_ray_distance=radius, relocate=True, classify=True, min_frontface_distance=0.1 if radius < 3.0 else 0.3))
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    fixed = drv.download_ddgi_fixed_rays()
    probes = int(np.prod(vol.counts))
    miss, back = int(np.count_nonzero(fixed == np.float32(1e27))), int(np.count_nonzero(fixed < 0))
    got = drv.download_ddgi()
    active = int(np.count_nonzero(got.data[..., 3] != 1.0))
    moved = int(np.count_nonzero(np.any(got.data[..., :3].view(np.uint16) & 0x7FFF, axis=-1)))
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} updates, probes {vol.counts[0]}x{vol.counts[1]}x{vol.counts[2]} = {probes}, "
          f"{probes * I.kDDGIFixedRays} fixed rays: {miss} miss, {back} back faces, {fixed.size - miss - back} front faces; {active} probes active, {moved} moved; "
          f"data checksum {int(got.data.view(np.uint16).astype(np.uint64).sum()):#x}")
    for label, op in OPS.items():
        cnt, ms = prof[op]
        print(f"  {label:15s} {ms / frames * 1e3:10.1f} us per update ({cnt // frames} launches)")
    trace, fixed_ms = prof[OPS["probe trace"]][1], prof[OPS["fixed-ray trace"]][1]
    print(f"  fixed-ray trace / trace = {fixed_ms / trace:.4f}; against the trace scaled from {active} active probes to all {probes}: {fixed_ms / (trace * probes / max(active, 1)):.4f} (1 / 8 = 0.1250)")
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
