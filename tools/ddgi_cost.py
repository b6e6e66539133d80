#!/usr/bin/env python3
"""Cost of the DDGI ambient term in the deferred lighting pass: FrameDriver(lighting=True, ddgi=...) on the generated city of
tools/lighting_cost.py at 3840x2160, steady state, "deferredlighting_PS_Main#main" per frame from the back-end profile, with the
volume of ddgi.Volume.for_scene (random irradiance and distances, borders filled: the cost does not depend on the values, the
Chebyshev and crush branches do), with DDGI on and off, next to other builds of the back end given as --variant=NAME=PATH (a
libtrhip.so of the parent commit: the DDGI-off kernels must not have become slower; one built with
-DTR_LIGHTING_EXPERIMENT_STORE_ONLY: the pass's loads and store without any arithmetic or probe lookup).  Variants run with DDGI
off (they may not know it).  Each run is its own process and the builds alternate `rounds` times (default 3) in one call.
usage: python tools/ddgi_cost.py [num_spheres] [width height] [--rounds=N] [--variant=NAME=PATH ...] [--debug-mode=M]
       python tools/ddgi_cost.py --child --ddgi=0|1 ...   one run in this process (TRHIP_LIB picks the build)"""
import numpy as np

import cost_common as cc

LIGHTING_US = r"deferredlighting_PS_Main\w*#main\s+([0-9.]+) us"


def run(n: int, render, debug_mode: int, use_ddgi: bool):
    from toyrenderer_amd import rhi
    from toyrenderer_amd.frame import FrameDriver
    c = cc.city(n, render)
    dev, gs, inst, rng = c.dev, c.gs, c.inst, c.rng
    shadow = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R8_UNORM, "ShadowMask")
    shadow.upload_mip(0, rng.integers(0, 256, (render[1], render[0]), dtype=np.uint64).astype(np.uint8))
    kw = {}
    note = "DDGI off"
    if use_ddgi:
        from toyrenderer_amd import ddgi
        # the scene's box from its instances' world-space positions (Scene::m_AABB), padded by the largest mesh radius
        pos = inst["m_WorldMatrix"][:, 3, :3].astype(np.float64)
        lo, hi = pos.min(0) - 1.0, pos.max(0) + 1.0
        centre, ext = (lo + hi) * 0.5, (hi - lo) * 0.5
        vol = ddgi.Volume.for_scene(centre, ext, float(np.linalg.norm(ext)))
        vol.irradiance[...] = ddgi.pack_unorm10(rng.uniform(0.15, 1.0, vol.irradiance.shape + (3,)).astype(np.float32))
        mean = (rng.uniform(0.25, 1.3, vol.distance.shape[:-1]) * float(np.mean(vol.spacing))).astype(np.float32)
        vol.distance[..., 0] = (mean * 0.5).astype(np.float16)
        vol.distance[..., 1] = (mean * mean * 0.65).astype(np.float16)
        vol.data[..., :3] = rng.uniform(-0.3, 0.3, vol.data.shape[:-1] + (3,)).astype(np.float16)
        vol.data[..., 3] = (rng.random(vol.data.shape[:-1]) < 0.3).astype(np.float16)
        vol.fill_borders()
        kw["ddgi"] = vol
        mb = (vol.irradiance.nbytes + vol.distance.nbytes + vol.data.nbytes) / 1e6
        note = f"DDGI on, probes {vol.counts[0]}x{vol.counts[1]}x{vol.counts[2]}, spacing {vol.spacing[0]:.3f} {vol.spacing[1]:.3f} {vol.spacing[2]:.3f}, textures {mb:.1f} MB"
    drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, debug_mode=debug_mode,
                      dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0), shadow_mask=shadow, **kw)
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    lit = int(np.count_nonzero(drv.depth.download_mip(0) > 0))
    words = drv.lighting_output.download_mip(0)
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {lit} lit pixels of {render[0] * render[1]}, {note}, "
          f"output checksum {int(words.astype(np.uint64).sum()):#x}")
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("deferredlighting_PS_Main"):
            print(f"  {name:45s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    drv.release(); shadow.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, opts = cc.parse_args()
    debug_mode = int(opt("debug-mode", 0))
    if "--child" in opts:
        run(n, render, debug_mode, opt("ddgi", "0") == "1")
    else:
        rounds = int(opt("rounds", 3))
        builds = [(name, path, f"--ddgi={on}", f"--debug-mode={10 if on and debug_mode else debug_mode}")
                  for (name, path), on in [(("ddgi on", None), 1)] + [(b, 0) for b in cc.variants(opts, "ddgi off")]]
        outs = cc.alternate(__file__, builds, rounds, [n, *render], timeout=300)
        for name, *_ in builds:
            print(f"{name:10s}: {cc.spread(cc.figures(outs[name], LIGHTING_US))}")
