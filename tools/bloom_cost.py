#!/usr/bin/env python3
"""Cost of the bloom chain: FrameDriver(post=True, bloom_mips=6) on the generated city of tools/postprocess_cost.py at 3840x2160,
steady state.  Reported per frame from the back-end profile: the chain ("bloom_PS_Downsample#main" + "bloom_PS_Upsample#main", all
2 * (mips - 1) launches) and the post pass that reads it; then every pass alone (its own command list, launched 20 times), next to
the time its bytes alone (the source mip read once, the destination mip written once) would take at the box's stream rate
(tools/membw, given with --membw=GB/s); and the same for other builds of the back end given as --variant=NAME=PATH (a libtrhip.so
whose csrc/k_bloom.hip was built with -DTR_BLOOM_LDS_DOWNSAMPLE=1: the downsample staged through LDS;
-DTR_BLOOM_EXPERIMENT_STORE_ONLY: loads and store without the arithmetic; -DTR_BLOOM_EXPERIMENT_FIXED_POINT and -ffp-contract=fast:
the negative controls).  Each run is its own process and the builds alternate `rounds` times (default 3) in one call, so that the
differences are taken on one box in one state.  --dump saves bloom mip 0 and the back buffer, for counting the words a control
changes (--compare=A.npz,B.npz prints the counts).
usage: python tools/bloom_cost.py [num_spheres] [width height] [--mips=N] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...]
       python tools/bloom_cost.py --child [--dump=FILE.npz] ...   one run in this process (TRHIP_LIB picks the build)
       python tools/bloom_cost.py --compare=A.npz,B.npz"""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = ("bloom_PS_Downsample#main", "bloom_PS_Upsample#main")
POST = "postprocess_PS_PostProcess#main"


def passes(render, mips):
    """(label, shader, source mip, destination mip) in the renderer's order."""
    n = mips - 1
    out = [(f"down {i}->{i + 1}", "bloom_PS_Downsample", i, i + 1) for i in range(n)]
    return out + [(f"up {n - i}->{n - i - 1}", "bloom_PS_Upsample", n - i, n - i - 1) for i in range(n)]


def run(n: int, render, mips: int, dump=None):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scene_gen import write_city_gltf
    from toyrenderer_amd import gltf_lite, rhi, synth
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    from toyrenderer_amd.rhi import PUSH, SAMPLER, TEX_SRV, TEX_UAV
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
    drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, post=True, dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0),
                      bloom_mips=mips)
    drv.record()
    for _ in range(5):
        drv.run()
    dev.wait_idle()
    drv.reset_exposure()
    dev.profile_reset(); dev.profile_enable(True)
    frames = 20
    for _ in range(frames):
        drv.run()
    dev.wait_idle()
    prof = dev.profile()
    dev.profile_enable(False)
    back, bloom0 = drv.back_buffer.download_mip(0), drv.download_bloom(0)
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {mips} mips, {frames} frames, bloom mip 0 checksum {int(bloom0.astype(np.uint64).sum()):#x}, "
          f"back buffer checksum {int(back.astype(np.uint64).sum()):#x}")
    chain = sum(prof[name][1] for name in CHAIN) / frames * 1e3
    print(f"  {'chain':20s} {chain:9.1f} us per frame ({sum(prof[name][0] for name in CHAIN) // frames} launches)")
    print(f"  {'post':20s} {prof[POST][1] / frames * 1e3:9.1f} us per frame")
    if dump:
        np.savez(dump, back=back, bloom0=bloom0)
    cl = dev.create_command_list()
    for label, shader, sm, dm in passes(render, mips):   # every pass alone, on the textures the frames left behind
        at = [p[0] for p in passes(render, mips)].index(label)
        k = drv.bloom_consts[at:at + 1]
        src = TEX_SRV(0, drv.lighting_output) if (shader.endswith("Downsample") and sm == 0) else TEX_SRV(0, drv.bloom_texture, sm)
        w, h = render[0] >> dm, render[1] >> dm
        cl.open()
        cl.dispatch(shader, [PUSH(0), src, TEX_UAV(0, drv.bloom_texture, dm), SAMPLER(0)], ((w + 7) // 8, (h + 7) // 8, 1), push=k)
        cl.close()
        for _ in range(3):
            dev.execute(cl)
        dev.wait_idle()
        dev.profile_reset(); dev.profile_enable(True)
        for _ in range(frames):
            dev.execute(cl)
        dev.wait_idle()
        cnt, ms = dev.profile()[shader + "#main"]
        dev.profile_enable(False)
        print(f"  {label:20s} {ms / cnt * 1e3:9.1f} us per launch")
    cl.release(); drv.release(); gs.release()
    dev.destroy()


if __name__ == "__main__":
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    opt = lambda key, default=None: next((a.split("=", 1)[1] for a in opts if a.startswith(f"--{key}=")), default)   # noqa: E731
    mips = int(opt("mips", 6))
    if opt("compare"):
        a, b = (np.load(p) for p in opt("compare").split(","))
        for key, what in (("bloom0", "bloom mip 0"), ("back", "back buffer")):
            print(f"{what} words that differ: {int(np.count_nonzero(a[key] != b[key]))} of {a[key].size}")
    elif "--child" in opts:
        run(n, render, mips, opt("dump"))
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = [("product", None)] + [tuple(a.split("=", 2)[1:]) for a in opts if a.startswith("--variant=")]
        labels = ["chain", "post"] + [p[0] for p in passes(render, mips)]
        times = {name: {k: [] for k in labels} for name, _ in builds}
        for r in range(rounds):
            for name, path in builds:
                env = dict(os.environ)
                if path:
                    env["TRHIP_LIB"] = os.path.abspath(path)
                else:
                    env.pop("TRHIP_LIB", None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), str(render[0]), str(render[1]), f"--mips={mips}"]
                out = subprocess.check_output(cmd, env=env).decode()
                sys.stdout.write(f"[{name}] " + out); sys.stdout.flush()
                for k in labels:
                    times[name][k].append(float(re.search(r"^\s+" + re.escape(k) + r"\s+([0-9.]+) us", out, re.M).group(1)))
        texels = lambda m: (render[0] >> m) * (render[1] >> m)                                                          # noqa: E731
        nbytes = {p[0]: 4 * (texels(p[2]) + texels(p[3])) for p in passes(render, mips)}
        nbytes["chain"] = sum(nbytes.values())
        for k in labels:
            line = k
            if k in nbytes:
                line += f": {nbytes[k] / 1e6:.2f} MB"
                line += f" = {nbytes[k] / membw / 1e3:.1f} us at the box's {membw:.0f} GB/s" if membw else " (stream rate not given with --membw: no bound)"
            print(line)
            for name, _ in builds:
                t = np.array(times[name][k])
                print(f"  {name:10s}: {' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}")
