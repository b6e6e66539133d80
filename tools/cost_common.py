"""What the cost tools share: the generated city, the steady-state profile, the command line and the parent that alternates
builds of the back end.  A tool keeps what is its own: its FrameDriver arguments, the ops it reports, its extra modes.

The city is one scene for every tool, so that their numbers can be set side by side: tests/scene_gen.write_city_gltf(num_spheres=n,
num_cutouts=n // 8), world matrices walked up the node parents in float64 on the host (the transform pass is timed elsewhere),
material indices and packed normals drawn from seed 7 in that order, and the camera of the file at the origin with a previous
view a step away.  A tool that draws more (a shadow texture, textures, a probe volume) goes on with the returned generator."""
import os
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FRAMES = 20


def load_city(n):
    """The loaded glTF scene and a copy of its instances with world matrices (previous = current)."""
    from scene_gen import write_city_gltf
    from toyrenderer_amd import gltf_lite, synth
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
    return s, inst


def seeded_normals(s, rng):
    """A copy of the vertices with packed normals drawn from rng: the generated city has no NORMAL attribute."""
    v = s.vertices.copy()
    v["m_PackedNormal"] = rng.integers(0, 1 << 30, len(v), dtype=np.uint64).astype(np.uint32)
    return v


def city_view(s, render, prev_eye=(-0.05, 0.0, 0.02)):
    from toyrenderer_amd import synth
    cam = s.cameras[0]
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    Vp = synth.world_to_view(prev_eye, cam.orientation)
    return synth.View(V, Vp, P, float(np.float32(cam.znear)), *render)


def city(n, render, shading=True, raytracing=False):
    """The city on device 0: dev, gs, view, s, inst, rng (seed 7, after the shared draws) and, with raytracing, build_ms.
    shading=False leaves out the seeded material indices, normals and materials (the depth and visibility rasters);
    raytracing=True takes the mesh data and the LOD-0 index buffer of cached_scene and calls GpuScene.set_raytracing."""
    from toyrenderer_amd import cached_scene, rhi, synth
    from toyrenderer_amd.frame import GpuScene
    s, inst = load_city(n)
    rng = np.random.default_rng(7)
    v = s.vertices
    if shading:
        inst["m_MaterialDataIdx"] = rng.integers(0, 64, len(inst), dtype=np.uint32)
        v = seeded_normals(s, rng)
    c = cached_scene.from_scene(s) if raytracing else None
    dev = rhi.Device(0)
    gs = GpuScene(dev, inst, c.meshData if raytracing else s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(v, s.meshletVertexIds, s.meshletTriangles)
    if shading:
        gs.set_materials(synth.materials(7))
    build_ms = None
    if raytracing:
        t0 = time.perf_counter()
        gs.set_raytracing(c.indices, c.meshSpecific)
        build_ms = (time.perf_counter() - t0) * 1e3
    return SimpleNamespace(dev=dev, gs=gs, view=city_view(s, render), s=s, inst=inst, rng=rng, build_ms=build_ms)


def profile(dev, run, frames=FRAMES):
    """The back-end profile of `frames` calls of run(): {op: (count, ms)}."""
    dev.profile_reset(); dev.profile_enable(True)
    for _ in range(frames):
        run()
    dev.wait_idle()
    prof = dev.profile()
    dev.profile_enable(False)
    return prof


def steady_profile(dev, run, warmup=5, frames=FRAMES, settle=None):
    """Warm-up calls of run(), an idle device, settle() if given (say, the exposure reset), then profile()."""
    for _ in range(warmup):
        run()
    dev.wait_idle()
    if settle:
        settle()
    return profile(dev, run, frames)


def parse_args(argv=None):
    """[num_spheres] [width height] and --key=value / --flag options: (n, render, opt, opts); opt(key, default) is the value of --key=."""
    argv = sys.argv[1:] if argv is None else argv
    opts = [a for a in argv if a.startswith("--")]
    args = [a for a in argv if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)

    def opt(key, default=None):
        return next((a.split("=", 1)[1] for a in opts if a.startswith(f"--{key}=")), default)
    return n, render, opt, opts


def variants(opts, product="product"):
    """[(name, path of its libtrhip.so or None for the product's)] from the --variant=NAME=PATH options."""
    return [(product, None)] + [tuple(a.split("=", 2)[1:]) for a in opts if a.startswith("--variant=")]


def alternate(script, builds, rounds, child_args, timeout=None):
    """`rounds` times over builds [(name, path, extra child arguments...)], each run a fresh `script --child` process with
    TRHIP_LIB set to path or removed; its output is echoed behind "[name] ".  Returns {name: [output of each round]}."""
    outs = {b[0]: [] for b in builds}
    for _ in range(rounds):
        for name, path, *extra in builds:
            env = dict(os.environ)
            if path:
                env["TRHIP_LIB"] = os.path.abspath(path)
            else:
                env.pop("TRHIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(script), "--child", *extra, *(str(a) for a in child_args)]
            out = subprocess.check_output(cmd, env=env, timeout=timeout).decode()
            sys.stdout.write(f"[{name}] " + out); sys.stdout.flush()
            outs[name].append(out)
    return outs


def figures(outs, pattern, flags=0):
    """The first group of pattern in each output, as floats: a kernel's microseconds over the rounds."""
    return [float(re.search(pattern, out, flags).group(1)) for out in outs]


def spread(t):
    """"a b c us; median M, spread S" of a list of microsecond figures."""
    t = np.array(t)
    return f"{' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}"


def stream_bound(nbytes, membw, sep=" = ", missing=" (stream rate not given with --membw: no bound)"):
    """The time nbytes take at the stream rate tools/membw measured (GB/s), as the tools print it next to a kernel's time."""
    return f"{sep}{nbytes / membw / 1e3:.1f} us at the box's {membw:.0f} GB/s" if membw else missing
