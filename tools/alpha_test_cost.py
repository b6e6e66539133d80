#!/usr/bin/env python3
"""Cost of the alpha test: the ALPHA_MASK_MODE=1 rasters and the textured trace beside the plain ones, on the generated city at
3840x2160 with a tenth of its instances in the alpha-mask list, each with an albedo texture out of 16 seeded 256 x 256 textures
(random alpha, full mip chains, cutoff 0.5; texture coordinates seeded from the positions, about a texel per pixel in the middle
distance).  Steady state, from the back-end profile, per frame.  The two sides alternate `rounds` times (default 3) in this one
process, on one device:
  rasters  a frame of the alpha-mask list ALONE (no opaque list, no occlusion culling: FrameDriver(visibility=True, culling_flags=5)),
           so that both sides draw exactly the same visible lists: "basepass_MS_Main_visibility#main" / "#tiles" with
           alpha_test=False beside "basepass_MS_Main_visibility ALPHA_MASK_MODE=1#main" / "#tiles" with alpha_test=True;
  trace    the whole city, FrameDriver(gbuffer=True, shadows=..., culling_flags=7): "shadowmask_CS_ShadowMask#main" with
           alpha_test=False beside "#textured" with alpha_test=True, hard and soft.  The rays of the two sides start from the
           depth their own rasters left (solid cards, cut-out cards), as they would in a frame.
usage: python tools/alpha_test_cost.py [num_spheres] [width height] [--rounds=N]"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIS, TRACE = "basepass_MS_Main_visibility", "shadowmask_CS_ShadowMask"
ALPHA = " ALPHA_MASK_MODE=1"


def city(n, render):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scene_gen import write_city_gltf
    from toyrenderer_amd import cached_scene, gltf_lite, rhi, synth
    from toyrenderer_amd import interop as I
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
    ids = np.arange(len(inst), dtype=np.uint32)
    alpha = ids[ids % 10 == 3]                      # a tenth of the instances: alpha-masked and textured (materials 0..15)
    opaque = ids[ids % 10 != 3]
    inst["m_MaterialDataIdx"] = rng.integers(16, 64, len(inst), dtype=np.uint32)
    inst["m_MaterialDataIdx"][alpha] = rng.integers(0, 16, len(alpha), dtype=np.uint32)
    v = s.vertices.copy()                           # the generated city has neither NORMAL nor TEXCOORD_0: seeded
    v["m_PackedNormal"] = rng.integers(0, 1 << 30, len(v), dtype=np.uint64).astype(np.uint32)
    v["m_TexCoord"] = (v["m_Position"][:, [0, 2]] * np.float32(2.0) + v["m_Position"][:, [1, 1]]).astype(np.float16).view(np.uint16)
    textures = [(I.make_mips(rng.integers(0, 256, (256, 256, 4), dtype=np.uint16).astype(np.uint8), srgb=True), rhi.FORMAT_SRGBA8_UNORM) for _ in range(16)]
    mats = synth.materials(7)
    mats["m_ConstAlbedo"][:, 3] = 1.0
    mats["m_AlphaCutoff"] = 0.5
    mats["m_MaterialFlags"][:16] = I.MaterialFlag_UseAlbedoTexture
    mats["m_AlbedoTexture"]["m_DescriptorIndex"][:16] = np.arange(16)
    mats["m_AlbedoTexture"]["m_IsWrapSampler"][:16] = 1
    c = cached_scene.from_scene(s)                  # the LOD-0 index buffer and the index counts
    dev = rhi.Device(0)
    scenes = []
    for op in (opaque, np.zeros(0, np.uint32)):     # the whole city; its alpha-mask list alone
        gs = GpuScene(dev, inst, c.meshData, s.meshlets, op, alpha)
        gs.set_geometry(v, s.meshletVertexIds, s.meshletTriangles)
        gs.set_textures(textures)
        gs.set_materials(mats)
        scenes.append(gs)
    scenes[0].set_raytracing(c.indices, c.meshSpecific)
    cam = s.cameras[0]
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view((0.0, 0.0, 0.0), cam.orientation)
    Vp = synth.world_to_view((-0.05, 0.0, 0.02), cam.orientation)
    return dev, scenes, synth.View(V, Vp, P, float(np.float32(cam.znear)), *render), len(inst), len(alpha)


def timed(dev, drv, names, frames=20):
    dev.profile_reset(); dev.profile_enable(True)
    for _ in range(frames):
        drv.run()
    dev.wait_idle()
    prof = dev.profile()
    dev.profile_enable(False)
    return [prof[k][1] / frames * 1e3 if k in prof else float("nan") for k in names]


def compare(dev, make, sides, rounds, rows):
    """sides: [(label, alpha_test, [profile names])]; rows: the launches' labels."""
    drivers = [make(alpha_test) for _, alpha_test, _ in sides]
    for drv in drivers:
        drv.record()
        for _ in range(5):
            drv.run()
    dev.wait_idle()
    us = [[] for _ in sides]
    for _ in range(rounds):                         # plain, alpha, plain, alpha, ...
        for i, (drv, (_, _, names)) in enumerate(zip(drivers, sides)):
            us[i].append(timed(dev, drv, names))
    for j, row in enumerate(rows):
        for i, (label, _, names) in enumerate(sides):
            t = np.array([r[j] for r in us[i]])
            print(f"    {row:6s} {label:6s} {names[j]:52s}: {' '.join(f'{x:.1f}' for x in t)} us; median {np.median(t):.1f}, spread {t.max() - t.min():.1f}")
    return drivers


def main():
    opts = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 2000
    render = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    rounds = int(next((a.split("=", 1)[1] for a in opts if a.startswith("--rounds=")), 3))
    dev, (whole, alone), view, ninst, nalpha = city(n, render)
    from toyrenderer_amd.frame import FrameDriver
    print(f"{ninst} instances, {nalpha} of them alpha-masked and textured, render {render[0]}x{render[1]}, {rounds} rounds of 20 frames, sides alternated")
    print("  rasters, the alpha-mask list alone:")
    drivers = compare(dev, lambda a: FrameDriver(dev, alone, view, record_capacity=1 << 16, culling_flags=5, visibility=True, alpha_test=a),
                      [("plain", False, [VIS + "#main", VIS + "#tiles"]), ("alpha", True, [VIS + ALPHA + "#main", VIS + ALPHA + "#tiles"])], rounds, ["main", "tiles"])
    covered = [int(np.count_nonzero(d.visibility.download_mip(0))) for d in drivers]
    print(f"    covered pixels: {covered[0]} solid, {covered[1]} with the discard ({covered[1] / max(covered[0], 1):.3f})")
    for d in drivers:
        d.release()
    noise = np.random.default_rng(1).integers(0, 256, (128, 128, 4), dtype=np.uint64).astype(np.uint8)
    for soft in (False, True):
        print(f"  trace, the whole city, soft {soft}:")
        drivers = compare(dev, lambda a: FrameDriver(dev, whole, view, record_capacity=1 << 16, culling_flags=7, gbuffer=True, dir_light=((0.2, 0.35, -0.9), 2.5),
                                                     shadows=dict(noise=noise, soft=soft, ray_start_offset=0.1), alpha_test=a),
                          [("plain", False, [TRACE + "#main"]), ("alpha", True, [TRACE + "#textured"])], rounds, ["trace"])
        for d, label in zip(drivers, ("plain", "alpha")):
            mask, depth = d.download_shadow_mask(), d.depth.download_mip(0)
            traced = int(np.count_nonzero(depth != 0))
            print(f"    {label}: {traced} traced texels, {np.count_nonzero(mask[depth != 0] == 0) / max(traced, 1):.3f} occluded")
            d.release()
    whole.release(); alone.release()
    dev.destroy()


if __name__ == "__main__":
    main()
