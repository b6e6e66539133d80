#!/usr/bin/env python3
"""Cost of textured materials: the fused "basepass_PS_Main_GBuffer" resolve of a generated city at 3840x2160, steady state, from the
back-end profile, in three modes that alternate `rounds` times (default 3) in one call, each in its own process:
  plain     texture-free materials, no table bound: "basepass_PS_Main_GBuffer#main" (the kernel of tools/gbuffer_cost.py's mode B);
  textured  every material with all four textures out of 16 seeded 256 x 256 textures with full mip chains (base colour and
            emissive sRGB), texture coordinates seeded from the positions (about a texel per pixel in the middle distance, wrap):
            "basepass_PS_Main_GBuffer#textured";
  baseline  `plain` with another build of the back end (--baseline-lib=PATH to its libtrhip.so, e.g. the parent commit's): shows
            whether the texture-free kernel moved.  The margin to judge it by is the baseline's own spread over the rounds.
  baseline-textured  `textured` with that other build: shows whether the RGBA8 path of the textured kernel moved.
--format=rgba8|bc1|bc3|mixed (default rgba8: the textures above).  With a block-compressed format the 16 textures are seeded random
blocks at the same 256 x 256 with full mip chains (bc1: BC1_UNORM_SRGB / BC1_UNORM by slot; bc3: BC3 likewise; mixed: base colour
BC1_UNORM_SRGB, normal BC5, metallic-roughness BC4, emissive BC3_UNORM_SRGB), sampled by a further mode:
  compressed  `textured` on the block-compressed textures, while `textured` (and `baseline-textured`) of the same invocation
            sample their interop.bc_decode twins as RGBA8_UNORM / SRGBA8_UNORM: both runs sample identical values.
usage: python tools/material_texture_cost.py [num_spheres] [width height] [--rounds=N] [--baseline-lib=PATH] [--format=rgba8|bc1|bc3|mixed]"""
import os
import re
import subprocess
import sys

import numpy as np

import cost_common as cc


BC_SLOT_FORMATS = {"bc1": (15, 14, 14, 15), "bc3": (19, 18, 18, 19), "mixed": (15, 21, 20, 19)}      # rhi.FORMAT_BC* by slot: base colour, normal, metallic-roughness, emissive


def bc_textures(fmt_name, compressed):
    """16 (mips, format) of seeded random blocks, 256 x 256 with full chains: the blocks themselves, or their bc_decode twins."""
    from toyrenderer_amd import interop as I
    from toyrenderer_amd import rhi
    rng = np.random.default_rng(11)
    out = []
    for t in range(16):
        fmt = BC_SLOT_FORMATS[fmt_name][t % 4]
        mips = I.BlockMips([rng.integers(0, 256, I.bc_level_bytes(256, 256, fmt, k), dtype=np.uint16).astype(np.uint8) for k in range(9)], 256, 256)
        if compressed:
            out.append((mips, fmt))
        else:
            out.append((I.bc_decode_mips(mips, fmt), rhi.FORMAT_SRGBA8_UNORM if fmt in (15, 17, 19) else rhi.FORMAT_RGBA8_UNORM))
    return out


def run(mode: str, n: int, render, fmt_name="rgba8"):
    from toyrenderer_amd import interop as I
    from toyrenderer_amd import rhi, synth
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    s, inst = cc.load_city(n)
    rng = np.random.default_rng(7)
    inst["m_MaterialDataIdx"] = rng.integers(0, 64, len(inst), dtype=np.uint32)
    v = cc.seeded_normals(s, rng)                   # the generated city has no TEXCOORD_0 either: seeded from the positions
    v["m_TexCoord"] = (v["m_Position"][:, [0, 2]] * np.float32(2.0) + v["m_Position"][:, [1, 1]]).astype(np.float16).view(np.uint16)
    dev = rhi.Device(0)
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(v, s.meshletVertexIds, s.meshletTriangles)
    mats = synth.materials(7)
    if mode in ("textured", "compressed"):
        textures = []
        for t in range(16 if fmt_name == "rgba8" else 0):
            img = rng.integers(0, 256, (256, 256, 4), dtype=np.uint16).astype(np.uint8)
            if t % 4 == 1:
                img[..., :2] = 70 + img[..., :2] % 116                                   # a normal map: x, y inside the unit disc
            textures.append((I.make_mips(img, srgb=t % 4 in (0, 3)), rhi.FORMAT_SRGBA8_UNORM if t % 4 in (0, 3) else rhi.FORMAT_RGBA8_UNORM))
        if fmt_name != "rgba8":
            textures = bc_textures(fmt_name, mode == "compressed")
        gs.set_textures(textures)
        mats["m_MaterialFlags"] = I.kMaterialFlagAnyTexture
        for c, slot in enumerate(("m_AlbedoTexture", "m_NormalTexture", "m_MetallicRoughnessTexture", "m_EmissiveTexture")):
            mats[slot]["m_DescriptorIndex"] = 4 * (np.arange(len(mats)) % 4) + c
            mats[slot]["m_IsWrapSampler"] = 1
    gs.set_materials(mats)
    drv = FrameDriver(dev, gs, cc.city_view(s, render), record_capacity=1 << 16, culling_flags=7, gbuffer=True)
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    covered = int(np.count_nonzero(drv.visibility.download_mip(0)))
    what = mode if fmt_name == "rgba8" or mode == "plain" else f"{mode} {fmt_name}" + ("" if mode == "compressed" else " twins")
    print(f"[{what}] {len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {covered} covered pixels, {rhi.LIB_PATH}")
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("basepass_PS_Main"):
            print(f"  {name:45s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    drv.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, _ = cc.parse_args()
    mode = opt("mode")
    rounds = int(opt("rounds", 3))
    baseline = opt("baseline-lib")
    fmt_name = opt("format", "rgba8")
    if fmt_name not in ("rgba8",) + tuple(BC_SLOT_FORMATS):
        sys.exit(f"--format={fmt_name}: one of rgba8, bc1, bc3, mixed")
    if mode:
        run(mode, n, render, fmt_name)
    else:
        modes = (["baseline", "baseline-textured"] if baseline else []) + ["plain", "textured"] + (["compressed"] if fmt_name != "rgba8" else [])
        us = {m: [] for m in modes}
        for r in range(rounds):
            for m in modes:
                env = dict(os.environ, TRHIP_LIB=os.path.abspath(baseline)) if m.startswith("baseline") else dict(os.environ)
                child = {"baseline": "plain", "baseline-textured": "textured"}.get(m, m)
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), f"--mode={child}", f"--format={fmt_name}", str(n), str(render[0]), str(render[1])],
                                              env=env, timeout=300).decode()
                sys.stdout.write(out); sys.stdout.flush()
                us[m].append(float(re.search(r"basepass_PS_Main_GBuffer#\w+\s+([0-9.]+) us", out).group(1)))
        for m in modes:
            print(f"{m:17s}: {cc.spread(us[m])}")
        print(f"textured - plain = {np.median(us['textured']) - np.median(us['plain']):.1f} us")
        if baseline:
            b = np.array(us["baseline"])
            print(f"plain - baseline = {np.median(us['plain']) - np.median(b):+.1f} us against the baseline's own spread of {b.max() - b.min():.1f} us")
            b = np.array(us["baseline-textured"])
            print(f"textured - baseline-textured = {np.median(us['textured']) - np.median(b):+.1f} us against the baseline's own spread of {b.max() - b.min():.1f} us")
        if fmt_name != "rgba8":
            print(f"compressed ({fmt_name}) - textured (its RGBA8 twins) = {np.median(us['compressed']) - np.median(us['textured']):+.1f} us")
