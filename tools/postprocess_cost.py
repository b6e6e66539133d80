#!/usr/bin/env python3
"""Cost of auto exposure and tone mapping: FrameDriver(post=True) on the generated city of tools/lighting_cost.py at 3840x2160,
steady state, the three kernels per frame from the back-end profile ("adaptluminance_CS_GenerateLuminanceHistogram#main",
"adaptluminance_CS_AdaptExposure#main", "postprocess_PS_PostProcess#main"), next to the time each pass's bytes alone would take at
the box's stream rate (tools/membw, given with --membw=GB/s) and next to other builds of the back end given as --variant=NAME=PATH
(a libtrhip.so built with -DTR_HISTOGRAM_EXPERIMENT_REFERENCE_SHAPE: one 16 x 16 group per tile and 256 global adds each;
-DTR_HISTOGRAM_PER_WAVE=0|1 and -DTR_HISTOGRAM_MERGE_LANES=0|1: a private LDS sub-histogram per wave or one per workgroup, equal bins of
neighbouring lanes merged before the add or not;
-DTR_POST_EXPERIMENT_STORE_ONLY: the post pass's loads and store without its arithmetic; -DTR_POST_EXPERIMENT_HW_LOGEXP and
-DTR_POST_EXPERIMENT_TRUNC_STORE: the negative controls).  With --one-value the histogram pass is also timed on an image of one
value, the worst case for same-address LDS adds.  Each run is its own process and the builds alternate `rounds` times (default 3)
in one call, so that the differences are taken on one box in one state.  --dump saves back buffer and histogram, for counting the
words a control changes.
usage: python tools/postprocess_cost.py [num_spheres] [width height] [--rounds=N] [--membw=GBps] [--variant=NAME=PATH ...] [--one-value] [--bloom]
       python tools/postprocess_cost.py --child [--dump=FILE.npz] ...   one run in this process (TRHIP_LIB picks the build)"""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("adaptluminance_CS_GenerateLuminanceHistogram#main", "adaptluminance_CS_AdaptExposure#main", "postprocess_PS_PostProcess#main")


def run(n: int, render, one_value: bool, bloom_on: bool, dump=None):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scene_gen import write_city_gltf
    from toyrenderer_amd import gltf_lite, rhi, synth
    from toyrenderer_amd import interop as I
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    from toyrenderer_amd.rhi import PUSH, TEX_SRV, UAV
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
    bloom = None
    if bloom_on:
        bloom = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R11G11B10_FLOAT, "Bloom")
        bloom.upload_mip(0, (rng.integers(0, 16 << 6, (render[1], render[0])) * (1 | 1 << 11)).astype(np.uint32))
    drv = FrameDriver(dev, gs, view, record_capacity=1 << 16, culling_flags=7, post=True, dir_light=((0.3, -0.8, 0.52), 3.0), camera_origin=(0.0, 0.0, 0.0),
                      bloom=(bloom, 0.1))
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
    back, hist = drv.back_buffer.download_mip(0), drv.histogram.download(np.uint32, 256)
    print(f"{len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, bloom {'bound' if bloom_on else 'unbound'}, {int(np.count_nonzero(hist))} bins used, "
          f"largest bin {int(hist.max())}, back buffer checksum {int(back.astype(np.uint64).sum()):#x}, luminance {float(drv.luminance.download(np.float32, 1)[0]):.6f}")
    for name in KERNELS:
        cnt, ms = prof[name]
        print(f"  {name:55s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    if dump:
        np.savez(dump, back=back, hist=hist)
    if one_value:                                   # the histogram pass alone on an image of one value: every add of a wave goes to one LDS word
        tex = dev.create_texture(render[0], render[1], 1, rhi.FORMAT_R11G11B10_FLOAT, "one value")
        tex.upload_mip(0, np.full((render[1], render[0]), (14 << 6) | (14 << 6) << 11 | (14 << 5) << 22, np.uint32))
        hk = np.zeros(1, I.GenerateLuminanceHistogramParameters)
        lo, hi = I.log_luminance_range(0.004, 12.0)
        hk["m_SrcColorDims"] = render; hk["m_MinLogLuminance"] = lo; hk["m_InverseLogLuminanceRange"] = np.float32(1.0) / np.float32(hi - lo)
        cl = dev.create_command_list()
        cl.open()
        cl.dispatch(KERNELS[0].split("#")[0], [PUSH(0), TEX_SRV(0, tex), UAV(0, drv.histogram)], ((render[0] + 15) // 16, (render[1] + 15) // 16, 1), push=hk)
        cl.close()
        for _ in range(5):
            dev.execute(cl)
        dev.wait_idle()
        dev.profile_reset(); dev.profile_enable(True)
        for _ in range(frames):
            dev.execute(cl)
        dev.wait_idle()
        cnt, ms = dev.profile()[KERNELS[0]]
        dev.profile_enable(False)
        print(f"  {'one value: ' + KERNELS[0]:55s} {ms / frames * 1e3:9.1f} us per launch")
        cl.release(); tex.release()
    drv.release(); gs.release()
    if bloom is not None:
        bloom.release()
    dev.destroy()


if __name__ == "__main__":
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    opt = lambda key, default=None: next((a.split("=", 1)[1] for a in opts if a.startswith(f"--{key}=")), default)   # noqa: E731
    one_value, bloom_on = "--one-value" in opts, "--bloom" in opts
    if "--child" in opts:
        run(n, render, one_value, bloom_on, opt("dump"))
    else:
        rounds = int(opt("rounds", 3))
        membw = float(opt("membw", 0)) or None
        builds = [("product", None)] + [tuple(a.split("=", 2)[1:]) for a in opts if a.startswith("--variant=")]
        labels = list(KERNELS) + (["one value: " + KERNELS[0]] if one_value else [])
        times = {name: {k: [] for k in labels} for name, _ in builds}
        for r in range(rounds):
            for name, path in builds:
                env = dict(os.environ)
                if path:
                    env["TRHIP_LIB"] = os.path.abspath(path)
                else:
                    env.pop("TRHIP_LIB", None)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), str(render[0]), str(render[1])] + [o for o in ("--one-value", "--bloom") if o in opts]
                out = subprocess.check_output(cmd, env=env).decode()
                sys.stdout.write(f"[{name}] " + out); sys.stdout.flush()
                for k in labels:
                    times[name][k].append(float(re.search(re.escape(k) + r"\s+([0-9.]+) us", out).group(1)))
        for k in labels:
            print(k)
            for name, _ in builds:
                t = np.array(times[name][k])
                print(f"  {name:10s}: {' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}")
        px = render[0] * render[1]
        for what, nbytes in (("histogram: 4 B read per pixel", 4 * px), (f"post: {'12' if bloom_on else '8'} B per pixel (colour{', bloom' if bloom_on else ''}, store)", (12 if bloom_on else 8) * px)):
            line = f"bytes moved, {what}: {nbytes / 1e6:.1f} MB"
            line += f": {nbytes / membw / 1e3:.1f} us at the box's {membw:.0f} GB/s" if membw else "; stream rate not given (--membw), bound not computed"
            print(line)
