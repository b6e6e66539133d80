#!/usr/bin/env python3
"""Cost of the sky pass: FrameDriver(lighting=True, sky=...) on the generated city of tools/postprocess_cost.py at 3840x2160, steady
state.  Reported from the back-end profile: "sky_PS_HosekWilkieSky#main" per frame over the city (its sky and drawn pixel counts
printed), then the pass alone over an all-sky frame (depth all 0, its own command list, launched 20 times), next to the time its
bytes alone would take at the box's stream rate (tools/membw, given with --membw=GB/s): 4 B per drawn pixel (the depth word) plus
8 B per sky pixel (the depth word and the stored word).  The same for other builds of the back end given as --variant=NAME=PATH (a
libtrhip.so whose csrc/k_sky.hip was built with -DTR_SKY_EXPERIMENT_STORE_ONLY: loads and the store without the arithmetic;
-DTR_SKY_EXPERIMENT_HW_EXP: v_exp_f32 and approximate division, the negative control that must fail tests/test_gpu_sky.py).  Each
run is its own process and the builds alternate `rounds` times (default 3) in one call, so that the differences are taken on one
box in one state.  --dump saves LightingOutput, for counting the words a control changes (--compare=A.npz,B.npz prints the count).
The dataset is read from tests/golden/hosek_rgb.npz.
usage: python tools/sky_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...]
       python tools/sky_cost.py --child [--dump=FILE.npz] ...   one run in this process (TRHIP_LIB picks the build)
       python tools/sky_cost.py --compare=A.npz,B.npz"""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKY = "sky_PS_HosekWilkieSky#main"
LABELS = ("city", "all sky")


def run(n: int, render, dump=None):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scene_gen import write_city_gltf
    from toyrenderer_amd import gltf_lite, rhi, sky, synth
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    from toyrenderer_amd.rhi import CB, TEX_SRV, TEX_UAV
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
    sun = np.array([0.3, 0.8, -0.52], np.float64)
    sun = tuple(float(x) for x in (sun / np.linalg.norm(sun)).astype(np.float32))
    dataset = sky.HosekDataset.load(os.path.join(ROOT, "tests", "golden", "hosek_rgb.npz"))
    drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, lighting=True, dir_light=(sun, 3.0), camera_origin=(0.0, 0.0, 0.0), sky=(dataset,))
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
    depth, out = drv.depth.download_mip(0), drv.lighting_output.download_mip(0)
    nsky = int(np.count_nonzero(depth <= 0))
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {nsky} sky pixels, {depth.size - nsky} drawn pixels, "
          f"LightingOutput checksum {int(out.astype(np.uint64).sum()):#x}")
    print(f"  {'city':20s} {prof[SKY][1] / frames * 1e3:9.1f} us per frame")
    if dump:
        np.savez(dump, lighting_output=out)
    cl = dev.create_command_list()                  # the pass alone over an all-sky frame
    zero = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R32_FLOAT, "all sky")
    zero.upload_mip(0, np.zeros((render[1], render[0]), np.float32))
    cl.open()
    cb = cl.constant_buffer(drv.sky_consts, "SkyPassParameters")
    cl.dispatch("sky_PS_HosekWilkieSky", [CB(0, cb), TEX_SRV(0, zero), TEX_UAV(0, drv.lighting_output, 0)], ((render[0] + 7) // 8, (render[1] + 7) // 8, 1))
    cl.close()
    for _ in range(3):
        dev.execute(cl)
    dev.wait_idle()
    dev.profile_reset(); dev.profile_enable(True)
    for _ in range(frames):
        dev.execute(cl)
    dev.wait_idle()
    cnt, ms = dev.profile()[SKY]
    dev.profile_enable(False)
    print(f"  {'all sky':20s} {ms / cnt * 1e3:9.1f} us per launch")
    cl.release(); zero.release(); drv.release(); gs.release()
    dev.destroy()


if __name__ == "__main__":
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    opt = lambda key, default=None: next((a.split("=", 1)[1] for a in opts if a.startswith(f"--{key}=")), default)   # noqa: E731
    if opt("compare"):
        a, b = (np.load(p) for p in opt("compare").split(","))
        print(f"LightingOutput words that differ: {int(np.count_nonzero(a['lighting_output'] != b['lighting_output']))} of {a['lighting_output'].size}")
    elif "--child" in opts:
        run(n, render, opt("dump"))
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = [("product", None)] + [tuple(a.split("=", 2)[1:]) for a in opts if a.startswith("--variant=")]
        times = {name: {k: [] for k in LABELS} for name, _ in builds}
        nsky = ndrawn = 0
        for r in range(rounds):
            for name, path in builds:
                env = dict(os.environ)
                if path:
                    env["TRHIP_LIB"] = os.path.abspath(path)
                else:
                    env.pop("TRHIP_LIB", None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), str(render[0]), str(render[1])]
                out = subprocess.check_output(cmd, env=env).decode()
                sys.stdout.write(f"[{name}] " + out); sys.stdout.flush()
                nsky, ndrawn = (int(x) for x in re.search(r"(\d+) sky pixels, (\d+) drawn pixels", out).groups())
                for k in LABELS:
                    times[name][k].append(float(re.search(r"^\s+" + re.escape(k) + r"\s+([0-9.]+) us", out, re.M).group(1)))
        nbytes = {"city": 4 * ndrawn + 8 * nsky, "all sky": 8 * render[0] * render[1]}
        for k in LABELS:
            line = f"{k}: {nbytes[k] / 1e6:.2f} MB"
            line += f" = {nbytes[k] / membw / 1e3:.1f} us at the box's {membw:.0f} GB/s" if membw else " (stream rate not given with --membw: no bound)"
            print(line)
            for name, _ in builds:
                t = np.array(times[name][k])
                print(f"  {name:10s}: {' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}")
