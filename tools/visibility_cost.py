#!/usr/bin/env python3
"""Cost of the visibility buffer: the two-phase frame with self-rendered depth (FrameDriver(raster_depth=True), raster
"basepass_MS_Main_depth") against the same frame with FrameDriver(visibility=True) (raster "basepass_MS_Main_visibility"
plus the "basepass_PS_Main_motion" resolve), on a generated city at 3840x2160, steady state, per op from the back-end
profile.  Each mode runs in its own process.
usage: python tools/visibility_cost.py [num_spheres] [width height]"""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(mode: str, n: int, render):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scene_gen import write_city_gltf
    from toyrenderer_amd import gltf_lite, rhi, synth
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    with tempfile.TemporaryDirectory() as d:
        s = gltf_lite.load(write_city_gltf(Path(d), num_spheres=n, num_cutouts=n // 8))
    inst = s.instances.copy()                       # world matrices on the host: the transform pass is timed elsewhere
    for i in range(len(inst)):
        k = int(s.primToNode[i])
        M = np.eye(4, dtype=np.float64)
        while k != 0xFFFFFFFF:
            t = s.nodes[k]
            L = np.diag(list(t["m_Scale"]) + [1.0]) @ synth.quat_to_matrix(tuple(t["m_Rotation"]))
            L[3, :3] = t["m_Position"]
            M = M @ L
            k = int(t["m_ParentNodeIdx"])
        inst["m_WorldMatrix"][i] = M.astype(np.float32)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    dev = rhi.Device(0)
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(s.vertices, s.meshletVertexIds, s.meshletTriangles)
    cam = s.cameras[0]
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    Vp = synth.world_to_view((-0.05, 0.0, 0.02), cam.orientation)
    view = synth.View(V, Vp, P, float(np.float32(cam.znear)), *render)
    drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, raster_depth=True, visibility=(mode == "visibility"))
    drv.record()
    for _ in range(5):
        drv.run()
    dev.wait_idle()
    dev.profile_reset(); dev.profile_enable(True)
    frames = 20
    for _ in range(frames):
        drv.run()
    dev.wait_idle()
    prof = dev.profile()
    dev.profile_enable(False)
    print(f"[{mode}] {len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames")
    total = 0.0
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("basepass_MS_Main") or name.startswith("basepass_PS_Main"):
            us = ms / frames * 1e3
            total += us
            print(f"  {name:45s} {us:9.1f} us per frame ({cnt // frames} launches)")
    print(f"  {'raster + resolve':45s} {total:9.1f} us per frame")
    drv.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--mode=")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    mode = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--mode=")), None)
    if mode:
        run(mode, n, render)
    else:
        for m in ("depth", "visibility"):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), f"--mode={m}", str(n), str(render[0]), str(render[1])])
