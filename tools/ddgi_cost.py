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
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(n: int, render, debug_mode: int, use_ddgi: bool):
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
    drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, lighting=True, debug_mode=debug_mode,
                      dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0), shadow_mask=shadow, **kw)
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
    lit = int(np.count_nonzero(drv.depth.download_mip(0) > 0))
    words = drv.lighting_output.download_mip(0)
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {lit} lit pixels of {render[0] * render[1]}, {note}, "
          f"output checksum {int(words.astype(np.uint64).sum()):#x}")
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("deferredlighting_PS_Main"):
            print(f"  {name:45s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    drv.release(); shadow.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    opt = lambda key, default=None: next((a.split("=", 1)[1] for a in opts if a.startswith(f"--{key}=")), default)   # noqa: E731
    debug_mode = int(opt("debug-mode", 0))
    if "--child" in opts:
        run(n, render, debug_mode, opt("ddgi", "0") == "1")
    else:
        rounds = int(opt("rounds", 3))
        builds = [("ddgi on", None, 1), ("ddgi off", None, 0)] + [tuple(a.split("=", 2)[1:]) + (0,) for a in opts if a.startswith("--variant=")]
        times = {name: [] for name, _, _ in builds}
        for r in range(rounds):
            for name, path, on in builds:
                env = dict(os.environ)
                if path:
                    env["TRHIP_LIB"] = os.path.abspath(path)
                else:
                    env.pop("TRHIP_LIB", None)
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", f"--ddgi={on}", f"--debug-mode={10 if on and debug_mode else debug_mode}",
                                               str(n), str(render[0]), str(render[1])], env=env, timeout=300).decode()
                sys.stdout.write(f"[{name}] " + out); sys.stdout.flush()
                times[name].append(float(re.search(r"deferredlighting_PS_Main\w*#main\s+([0-9.]+) us", out).group(1)))
        for name, _, _ in builds:
            t = np.array(times[name])
            print(f"{name:10s}: {' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}")
