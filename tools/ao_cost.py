#!/usr/bin/env python3
"""Cost of the ambient occlusion passes: FrameDriver(lighting=True, ao=...) on the generated city of tools/sky_cost.py at 3840x2160,
steady state.  Reported from the back-end profile, per frame: "ambientocclusion_CS_XeGTAO_PrefilterDepths#main",
"...MainPass DEBUG_OUTPUT_MODE=0#main" and "...Denoise#main" (all its dispatches together and per dispatch) for each quality level
with 3 denoise passes and for 1 to 3 denoise passes at Ultra, next to the time each kernel's bytes alone would take at the box's
stream rate (tools/membw, given with --membw=GB/s): prefilter 4 B read + 2 * (1 + 1/4 + 1/16 + 1/64 + 1/256) B written per pixel;
main 2 B (the centre) + 16 B (GBufferA) read and 2 B written per pixel, its 2-byte sample fetches counted apart (4 * slices * steps per
pixel, mostly cache hits: an upper figure); denoise 2 * 9 B gathered (an upper figure, neighbours share them) and 1 B written.
--insts=N (the main pass's SQ_INSTS_VALU of one Ultra frame, from a counter run of `--child` of its own) prints instructions per
pixel.  The same for other builds of the back end given as --variant=NAME=PATH (a libtrhip.so whose csrc/k_ambientocclusion.hip was
built with -DTR_AO_EXPERIMENT_HW_TRIG: v_sin_f32, v_cos_f32, v_log_f32 and v_exp_f32 in place of the software functions, the negative
control that must fail tests/test_gpu_ao.py).  Each run is its own process and the builds alternate `rounds` times (default 3).
usage: python tools/ao_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--insts=N] [--variant=NAME=PATH ...]
       python tools/ao_cost.py --child [--only=QUALITY,PASSES] ...   one run in this process (TRHIP_LIB picks the build)"""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFILTER = "ambientocclusion_CS_XeGTAO_PrefilterDepths#main"
MAIN = "ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0#main"
DENOISE = "ambientocclusion_CS_XeGTAO_Denoise#main"
CONFIGS = [(0, 3), (1, 3), (2, 3), (3, 3), (3, 1), (3, 2)]          # (quality, denoise passes)
SAMPLES = {0: 1 * 2, 1: 2 * 2, 2: 3 * 3, 3: 9 * 2}                  # slices * steps


def city(n, render):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scene_gen import write_city_gltf
    from toyrenderer_amd import gltf_lite, rhi, synth
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
    dev = rhi.Device(0)
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(v, s.meshletVertexIds, s.meshletTriangles)
    gs.set_materials(synth.materials(7))
    cam = s.cameras[0]
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    Vp = synth.world_to_view((-0.05, 0.0, 0.02), cam.orientation)
    return dev, gs, synth.View(V, Vp, P, float(np.float32(cam.znear)), *render), len(inst)


def run(n, render, only=None):
    dev, gs, view, ninst = city(n, render)
    from toyrenderer_amd.frame import FrameDriver
    frames = 20
    print(f"{ninst} instances, render {render[0]}x{render[1]}, {frames} frames per configuration")
    for quality, passes in ([only] if only else CONFIGS):
        drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, lighting=True, debug_mode=9, ao=dict(quality=quality, denoise_passes=passes))
        drv.record()
        for _ in range(5):
            drv.run()
        dev.wait_idle()
        dev.profile_reset(); dev.profile_enable(True)
        for _ in range(frames):
            drv.run()
        dev.wait_idle()
        prof = dev.profile()
        dev.profile_enable(False)
        ssao = drv.download_ssao()
        us = {k: prof[k][1] / frames * 1e3 for k in (PREFILTER, MAIN, DENOISE)}
        print(f"  quality {quality} passes {passes}: prefilter {us[PREFILTER]:8.1f} us, main {us[MAIN]:8.1f} us, denoise {us[DENOISE]:8.1f} us "
              f"({us[DENOISE] / max(1, passes):.1f} per dispatch); SSAO checksum {int(ssao.astype(np.uint64).sum()):#x}")
        drv.release()
    gs.release()
    dev.destroy()


if __name__ == "__main__":
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    opt = lambda key, default=None: next((a.split("=", 1)[1] for a in opts if a.startswith(f"--{key}=")), default)   # noqa: E731
    if "--child" in opts:
        run(n, render, tuple(int(x) for x in opt("only").split(",")) if opt("only") else None)
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = [("product", None)] + [tuple(a.split("=", 2)[1:]) for a in opts if a.startswith("--variant=")]
        times = {name: {c: {k: [] for k in ("prefilter", "main", "denoise")} for c in CONFIGS} for name, _ in builds}
        for r in range(rounds):
            for name, path in builds:
                env = dict(os.environ)
                if path:
                    env["TRHIP_LIB"] = os.path.abspath(path)
                else:
                    env.pop("TRHIP_LIB", None)
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", str(n), str(render[0]), str(render[1])], env=env).decode()
                sys.stdout.write(f"[{name}] " + out); sys.stdout.flush()
                for m in re.finditer(r"quality (\d) passes (\d): prefilter\s+([0-9.]+) us, main\s+([0-9.]+) us, denoise\s+([0-9.]+) us", out):
                    c = (int(m.group(1)), int(m.group(2)))
                    for k, x in zip(("prefilter", "main", "denoise"), m.groups()[2:]):
                        times[name][c][k].append(float(x))
        px = render[0] * render[1]
        for c in CONFIGS:
            nbytes = {"prefilter": px * (4 + 2 * (1 + 1 / 4 + 1 / 16 + 1 / 64 + 1 / 256)), "main": px * (2 + 16 + 2), "denoise": max(1, c[1]) * px * (18 + 1)}
            print(f"quality {c[0]}, {c[1]} denoise passes (main pass sample fetches: {4 * SAMPLES[c[0]] * px / 1e6:.0f} MB more if none hit a cache):")
            for k in ("prefilter", "main", "denoise"):
                line = f"  {k}: {nbytes[k] / 1e6:.1f} MB"
                line += f" = {nbytes[k] / membw / 1e3:.1f} us at the box's {membw:.0f} GB/s" if membw else " (stream rate not given with --membw: no bound)"
                print(line)
                for name, _ in builds:
                    t = np.array(times[name][c][k])
                    print(f"    {name:10s}: {' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}")
        if opt("insts"):
            print(f"main pass at Ultra: {float(opt('insts')) * 64 / px:.0f} VALU instructions per pixel (SQ_INSTS_VALU counts waves: x 64 lanes / {px} pixels)")
