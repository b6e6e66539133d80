#!/usr/bin/env python3
"""Cost of the ray-traced shadow mask: FrameDriver(lighting=True, shadows=...) on the generated city of tools/lighting_cost.py at
3840x2160, steady state.  Reported from the back-end profile, per frame: "raytracing_CS_RefitTLAS#main" (both of its kernels),
"shadowmask_CS_ShadowMask#main" and, from the same run, "deferredlighting_PS_Main#main", for hard and soft shadows; next to them the
host-side build (BLAS of every mesh, TLAS topology) in milliseconds and the structure's size.  Each configuration is timed `rounds`
times (default 3) in this one process; the occluded share of the traced texels says what the rays met.
usage: python tools/shadowmask_cost.py [num_spheres] [width height] [--rounds=N]"""
import numpy as np

import cost_common as cc

REFIT, TRACE, LIGHTING = "raytracing_CS_RefitTLAS#main", "shadowmask_CS_ShadowMask#main", "deferredlighting_PS_Main#main"


def main():
    n, render, opt, _ = cc.parse_args()
    rounds = int(opt("rounds", 3))
    c = cc.city(n, render, raytracing=True)
    dev, gs = c.dev, c.gs
    from toyrenderer_amd.frame import FrameDriver
    rt = gs.rt
    tris = int(sum(int(k) // 3 for k in rt["blas"]["index_counts"]))
    nbytes = sum(b.size for b in rt.values() if hasattr(b, "size") and not isinstance(b, np.ndarray)) + gs.indices.size
    print(f"{len(c.inst)} instances, {len(rt['blas']['headers'])} meshes of {tris} triangles, render {render[0]}x{render[1]}")
    print(f"set_raytracing (read-back, BLAS builds, TLAS topology, uploads): {c.build_ms:.1f} ms on the host; {len(rt['blas']['nodes'])} BLAS nodes, deepest {max(rt['blas']['depths'])}, "
          f"{len(rt['tlas']['nodes'])} TLAS nodes in {rt['tlas']['num_levels']} levels; {nbytes / 1e6:.2f} MB on the device")
    noise = np.random.default_rng(1).integers(0, 256, (128, 128, 4), dtype=np.uint64).astype(np.uint8)
    frames = cc.FRAMES
    for soft in (False, True):
        drv = FrameDriver(dev, gs, c.view, record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=((0.2, 0.35, -0.9), 2.5),
                          shadows=dict(noise=noise, soft=soft, ray_start_offset=0.1))
        drv.record()
        for _ in range(5):
            drv.run()
        dev.wait_idle()
        rows = {k: [] for k in (REFIT, TRACE, LIGHTING)}
        for _ in range(rounds):
            prof = cc.profile(dev, drv.run)
            for k in rows:
                rows[k].append(prof[k][1] / frames * 1e3)
        mask, depth = drv.download_shadow_mask(), drv.depth.download_mip(0)
        traced = int(np.count_nonzero(depth != 0))
        print(f"  soft {soft}: {traced} traced texels of {mask.size}, {np.count_nonzero(mask[depth != 0] == 0) / max(traced, 1):.3f} occluded")
        for k, t in rows.items():
            print(f"    {k:34s}: {cc.spread(t)}")
        drv.release()
    gs.release()
    dev.destroy()


if __name__ == "__main__":
    main()
