#!/usr/bin/env python3
"""Time the two-phase frame with self-rendered depth (FrameDriver(raster_depth=True)) on a generated glTF scene with real
geometry, per kernel (back-end profile).  usage: python tools/raster_time.py [num_spheres] [width height]"""
import numpy as np

import cost_common as cc
from toyrenderer_amd import rhi
from toyrenderer_amd.frame import FrameDriver, GpuScene

n, render, _, _ = cc.parse_args()
s, inst = cc.load_city(n)
inst["m_PrevWorldMatrix"] = s.instances["m_PrevWorldMatrix"]       # this tool leaves the loader's previous matrices and has no camera step
dev = rhi.Device(0)
gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
gs.set_geometry(s.vertices, s.meshletVertexIds, s.meshletTriangles)
view = cc.city_view(s, render, prev_eye=(0.0, 0.0, 0.0))
drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, raster_depth=True)
prof = cc.steady_profile(dev, lambda: (drv.record(), drv.run()), warmup=3, frames=5)
res = drv.results()
print(f"{len(inst)} instances, {len(s.meshlets)} meshlets in meshes, render {render}; visible early {int(res[0]['drawArgs'][0])}, late {int(res[1]['drawArgs'][0]) if res[1] else 0}")
for k_, (cnt, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
    print(f"  {k_:70s} {ms / cnt * 1e3:9.1f} us x{cnt}")
depth = drv.depth.download_mip(0)
print("covered pixels:", int(np.count_nonzero(depth)), "of", depth.size)
