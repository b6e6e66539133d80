#!/usr/bin/env python3
"""Cost of GBufferA: the frame with FrameDriver(visibility=True) (mode A: the "basepass_PS_Main_motion" resolve alone) against
the same frame with FrameDriver(gbuffer=True) (mode B: the fused "basepass_PS_Main_GBuffer" resolve, GBufferA + motion), on a
generated city at 3840x2160, steady state, per op from the back-end profile.  Each mode runs in its own process and the
modes alternate `rounds` times (default 3) in one call, so that B - A is taken on one box in one state; the spread of A
over the rounds is printed next to it.
usage: python tools/gbuffer_cost.py [num_spheres] [width height] [--rounds=N]"""
import os
import re
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
    rng = np.random.default_rng(7)
    inst["m_MaterialDataIdx"] = rng.integers(0, 64, len(inst), dtype=np.uint32)
    v = s.vertices.copy()                           # the generated city has no NORMAL attribute: seeded packed normals
    v["m_PackedNormal"] = rng.integers(0, 1 << 30, len(v), dtype=np.uint64).astype(np.uint32)
    dev = rhi.Device(0)
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(v, s.meshletVertexIds, s.meshletTriangles)
    gs.set_materials(synth.materials(7))
    cam = s.cameras[0]
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    Vp = synth.world_to_view((-0.05, 0.0, 0.02), cam.orientation)
    view = synth.View(V, Vp, P, float(np.float32(cam.znear)), *render)
    drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, visibility=True, gbuffer=(mode == "gbuffer"))
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
    covered = int(np.count_nonzero(drv.visibility.download_mip(0)))
    print(f"[{mode}] {len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {covered} covered pixels")
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("basepass_MS_Main") or name.startswith("basepass_PS_Main"):
            print(f"  {name:45s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    drv.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    mode = next((a.split("=", 1)[1] for a in opts if a.startswith("--mode=")), None)
    rounds = int(next((a.split("=", 1)[1] for a in opts if a.startswith("--rounds=")), 3))
    if mode:
        run(mode, n, render)
    else:
        resolve = {"visibility": [], "gbuffer": []}
        for r in range(rounds):
            for m in ("visibility", "gbuffer"):
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), f"--mode={m}", str(n), str(render[0]), str(render[1])]).decode()
                sys.stdout.write(out); sys.stdout.flush()
                resolve[m].append(float(re.search(r"basepass_PS_Main_\w+#main\s+([0-9.]+) us", out).group(1)))
        a, b = np.array(resolve["visibility"]), np.array(resolve["gbuffer"])
        print(f"A (motion resolve alone)  : {' '.join(f'{x:.1f}' for x in a)} us; median {np.median(a):.1f}, spread {a.max() - a.min():.1f}")
        print(f"B (fused G-buffer resolve): {' '.join(f'{x:.1f}' for x in b)} us; median {np.median(b):.1f}, spread {b.max() - b.min():.1f}")
        print(f"B - A = {np.median(b) - np.median(a):.1f} us for {render[0] * render[1] * 16 / 1e6:.1f} MB of GBufferA stored per frame")
