#!/usr/bin/env python3
"""Cost of the ray-traced shadow mask: FrameDriver(lighting=True, shadows=...) on the generated city of tools/lighting_cost.py at
3840x2160, steady state.  Reported from the back-end profile, per frame: "raytracing_CS_RefitTLAS#main" (both of its kernels),
"shadowmask_CS_ShadowMask#main" and, from the same run, "deferredlighting_PS_Main#main", for hard and soft shadows; next to them the
host-side build (BLAS of every mesh, TLAS topology) in milliseconds and the structure's size.  Each configuration is timed `rounds`
times (default 3) in this one process; the occluded share of the traced texels says what the rays met.
usage: python tools/shadowmask_cost.py [num_spheres] [width height] [--rounds=N]"""
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFIT, TRACE, LIGHTING = "raytracing_CS_RefitTLAS#main", "shadowmask_CS_ShadowMask#main", "deferredlighting_PS_Main#main"


def city(n, render):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scene_gen import write_city_gltf
    from toyrenderer_amd import cached_scene, gltf_lite, rhi, synth
    from toyrenderer_amd.frame import GpuScene
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
    c = cached_scene.from_scene(s)                  # the LOD-0 index buffer and the index counts
    dev = rhi.Device(0)
    gs = GpuScene(dev, inst, c.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(v, s.meshletVertexIds, s.meshletTriangles)
    gs.set_materials(synth.materials(7))
    t0 = time.perf_counter()
    gs.set_raytracing(c.indices, c.meshSpecific)
    build_ms = (time.perf_counter() - t0) * 1e3
    cam = s.cameras[0]
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    Vp = synth.world_to_view((-0.05, 0.0, 0.02), cam.orientation)
    return dev, gs, synth.View(V, Vp, P, float(np.float32(cam.znear)), *render), len(inst), build_ms


def main():
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    rounds = int(next((a.split("=", 1)[1] for a in opts if a.startswith("--rounds=")), 3))
    dev, gs, view, ninst, build_ms = city(n, render)
    from toyrenderer_amd.frame import FrameDriver
    rt = gs.rt
    tris = int(sum(int(c) // 3 for c in rt["blas"]["index_counts"]))
    nbytes = sum(b.size for b in rt.values() if hasattr(b, "size") and not isinstance(b, np.ndarray)) + gs.indices.size
    print(f"{ninst} instances, {len(rt['blas']['headers'])} meshes of {tris} triangles, render {render[0]}x{render[1]}")
    print(f"set_raytracing (read-back, BLAS builds, TLAS topology, uploads): {build_ms:.1f} ms on the host; {len(rt['blas']['nodes'])} BLAS nodes, deepest {max(rt['blas']['depths'])}, "
          f"{len(rt['tlas']['nodes'])} TLAS nodes in {rt['tlas']['num_levels']} levels; {nbytes / 1e6:.2f} MB on the device")
    noise = np.random.default_rng(1).integers(0, 256, (128, 128, 4), dtype=np.uint64).astype(np.uint8)
    frames = 20
    for soft in (False, True):
        drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=((0.2, 0.35, -0.9), 2.5),
                          shadows=dict(noise=noise, soft=soft, ray_start_offset=0.1))
        drv.record()
        for _ in range(5):
            drv.run()
        dev.wait_idle()
        rows = {k: [] for k in (REFIT, TRACE, LIGHTING)}
        for _ in range(rounds):
            dev.profile_reset(); dev.profile_enable(True)
            for _ in range(frames):
                drv.run()
            dev.wait_idle()
            prof = dev.profile()
            dev.profile_enable(False)
            for k in rows:
                rows[k].append(prof[k][1] / frames * 1e3)
        mask, depth = drv.download_shadow_mask(), drv.depth.download_mip(0)
        traced = int(np.count_nonzero(depth != 0))
        print(f"  soft {soft}: {traced} traced texels of {mask.size}, {np.count_nonzero(mask[depth != 0] == 0) / max(traced, 1):.3f} occluded")
        for k, t in rows.items():
            t = np.array(t)
            print(f"    {k:34s}: {' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}")
        drv.release()
    gs.release()
    dev.destroy()


if __name__ == "__main__":
    main()
