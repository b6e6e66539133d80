#!/usr/bin/env python3
"""Cost of texture streaming in the G-buffer resolve: the city of tools/material_texture_cost.py at 3840x2160 (every material with all
four textures out of 16 seeded 256 x 256 textures, full mip chains), steady state, from the back-end profile, in modes that alternate
`rounds` times (default 3) in one call, each in its own process:
  baseline-textured  "basepass_PS_Main_GBuffer#textured" with another build of the back end (--baseline-lib=PATH to its libtrhip.so,
                     the parent commit's): #textured of this tree must sit inside that build's own spread;
  textured           #textured with this tree's library;
  streamed           #streamed: the same textures streamable (regions of 64 x 64), fully resident, every min-mip texel 0, the maps
                     named by every material, m_bWriteSamplerFeedback = 0: the clamp and the map lookup alone;
  feedback           #streamed with m_bWriteSamplerFeedback = 1: the recorded frame clears, writes and decodes the feedback of all
                     16 textures every frame (FrameDriver(streaming=dict(textures_per_frame=16))), as TextureFeedbackManager would;
  naive-feedback     `feedback` with a build whose feedback write is one atomic per mark (--naive-lib=PATH: the csrc Makefile with
                     -DTRHIP_FEEDBACK_NAIVE added to CXXFLAGS and another LIBDIR): what the per-lane drop and the wave merge buy.
The frame is recorded once and run again and again, so the residency loop applies nothing: the textures are made fully resident by
hand before the first frame.  The other kernels of the frame do not change between the modes.
usage: python tools/texture_streaming_cost.py [num_spheres] [width height] [--rounds=N] [--baseline-lib=PATH] [--naive-lib=PATH]"""
import os
import re
import subprocess
import sys

import numpy as np

import cost_common as cc

REGION = (64, 64)


def run(mode: str, n: int, render):
    from toyrenderer_amd import interop as I
    from toyrenderer_amd import rhi, synth
    from toyrenderer_amd.frame import FrameDriver, GpuScene
    s, inst = cc.load_city(n)
    rng = np.random.default_rng(7)
    inst["m_MaterialDataIdx"] = rng.integers(0, 64, len(inst), dtype=np.uint32)
    v = cc.seeded_normals(s, rng)
    v["m_TexCoord"] = (v["m_Position"][:, [0, 2]] * np.float32(2.0) + v["m_Position"][:, [1, 1]]).astype(np.float16).view(np.uint16)
    dev = rhi.Device(0)
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(v, s.meshletVertexIds, s.meshletTriangles)
    mats = synth.materials(7)
    textures = []
    for t in range(16):
        img = rng.integers(0, 256, (256, 256, 4), dtype=np.uint16).astype(np.uint8)
        if t % 4 == 1:
            img[..., :2] = 70 + img[..., :2] % 116
        textures.append((I.make_mips(img, srgb=t % 4 in (0, 3)), rhi.FORMAT_SRGBA8_UNORM if t % 4 in (0, 3) else rhi.FORMAT_RGBA8_UNORM))
    streamed = mode != "textured"
    gs.set_textures(textures, streaming=dict(region=REGION) if streamed else None)
    for st in gs.streams:                                                 # fully resident by hand: every level uploaded, every min-mip texel 0
        for k, m in enumerate(st.host):
            st.texture.upload_mip(k, m)
        st.resident[:] = 1
        st.min_mip[...] = 0
        st.min_mip_map.upload_mip(0, st.min_mip)
    mats["m_MaterialFlags"] = I.kMaterialFlagAnyTexture
    for c, slot in enumerate(("m_AlbedoTexture", "m_NormalTexture", "m_MetallicRoughnessTexture", "m_EmissiveTexture")):
        mats[slot]["m_DescriptorIndex"] = 4 * (np.arange(len(mats)) % 4) + c
        mats[slot]["m_IsWrapSampler"] = 1
    gs.set_materials(mats)                                                # fills in the map indices of the streamable textures
    kw = dict(streaming=dict(textures_per_frame=16, evict_after=1 << 20)) if mode == "feedback" else {}
    drv = FrameDriver(dev, gs, cc.city_view(s, render), record_capacity=1 << 16, culling_flags=7, gbuffer=True, **kw)
    drv.record()
    frames = cc.FRAMES
    prof = cc.steady_profile(dev, drv.run)
    covered = int(np.count_nonzero(drv.visibility.download_mip(0)))
    print(f"[{mode}] {len(inst)} instances, render {render[0]}x{render[1]}, {frames} frames, {covered} covered pixels, {rhi.LIB_PATH}")
    for name, (cnt, ms) in sorted(prof.items()):
        if name.startswith("basepass_PS_Main") or name.startswith("decode_sampler_feedback"):
            print(f"  {name:45s} {ms / frames * 1e3:9.1f} us per frame ({cnt // frames} launches)")
    if mode == "feedback":
        asked = [int((drv.download_feedback(i) != 0xFF).sum()) for i in range(16)]
        print(f"  regions asked for, per texture: {asked} of {(256 // REGION[0]) * (256 // REGION[1])}")
    drv.release(); gs.release(); dev.destroy()


if __name__ == "__main__":
    n, render, opt, _ = cc.parse_args()
    mode = opt("mode")
    rounds = int(opt("rounds", 3))
    baseline, naive = opt("baseline-lib"), opt("naive-lib")
    if mode:
        run(mode, n, render)
    else:
        modes = (["baseline-textured"] if baseline else []) + ["textured", "streamed", "feedback"] + (["naive-feedback"] if naive else [])
        child = {"baseline-textured": "textured", "naive-feedback": "feedback"}
        lib = {"baseline-textured": baseline, "naive-feedback": naive}
        us = {m: [] for m in modes}
        for r in range(rounds):
            for m in modes:
                env = dict(os.environ, TRHIP_LIB=os.path.abspath(lib[m])) if m in lib else dict(os.environ)
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), f"--mode={child.get(m, m)}", str(n), str(render[0]), str(render[1])],
                                              env=env, timeout=300).decode()
                sys.stdout.write(out); sys.stdout.flush()
                us[m].append(float(re.search(r"basepass_PS_Main_GBuffer#\w+\s+([0-9.]+) us", out).group(1)))
        for m in modes:
            print(f"{m:17s}: {cc.spread(us[m])}")
        med = {m: float(np.median(us[m])) for m in modes}
        if baseline:
            b = np.array(us["baseline-textured"])
            print(f"textured - baseline-textured = {med['textured'] - np.median(b):+.1f} us against the baseline's own spread of {b.max() - b.min():.1f} us")
        print(f"streamed - textured = {med['streamed'] - med['textured']:+.1f} us; feedback - streamed = {med['feedback'] - med['streamed']:+.1f} us; "
              f"feedback / textured = {med['feedback'] / med['textured']:.2f}")
        if naive:
            print(f"naive-feedback - feedback = {med['naive-feedback'] - med['feedback']:+.1f} us: what the per-lane drop and the wave merge buy")
