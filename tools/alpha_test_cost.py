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
import numpy as np

import cost_common as cc

VIS, TRACE = "basepass_MS_Main_visibility", "shadowmask_CS_ShadowMask"
ALPHA = " ALPHA_MASK_MODE=1"


def city(n, render):
    from toyrenderer_amd import cached_scene, rhi, synth
    from toyrenderer_amd import interop as I
    from toyrenderer_amd.frame import GpuScene
    s, inst = cc.load_city(n)
    rng = np.random.default_rng(7)
    ids = np.arange(len(inst), dtype=np.uint32)
    alpha = ids[ids % 10 == 3]                      # a tenth of the instances: alpha-masked and textured (materials 0..15)
    opaque = ids[ids % 10 != 3]
    inst["m_MaterialDataIdx"] = rng.integers(16, 64, len(inst), dtype=np.uint32)
    inst["m_MaterialDataIdx"][alpha] = rng.integers(0, 16, len(alpha), dtype=np.uint32)
    v = cc.seeded_normals(s, rng)                   # the generated city has no TEXCOORD_0 either: seeded from the positions
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
    return dev, scenes, cc.city_view(s, render), len(inst), len(alpha)


def timed(dev, drv, names, frames=cc.FRAMES):
    prof = cc.profile(dev, drv.run, frames)
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
            print(f"    {row:6s} {label:6s} {names[j]:52s}: {cc.spread([r[j] for r in us[i]])}")
    return drivers


def main():
    n, render, opt, _ = cc.parse_args()
    rounds = int(opt("rounds", 3))
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
