"""What the shadow mask's GPU test modules share (tests/test_gpu_shadowmask.py, tests/test_gpu_shadow_walk_scenes.py): refit + trace
through rhi bindings, and the references of tests/shadow_scenes.py WALK_CASES, computed once per process (tests/test_shadowmask_ref.py
asserts their preconditions from the same objects).  Not a test module: every assert here says what it compared."""
import numpy as np

import shadow_scenes as SS
import shadowmask_ref as SR
from toyrenderer_amd import accel
from toyrenderer_amd import interop as I

F = np.float32
TRACE, REFIT = "shadowmask_CS_ShadowMask", "raytracing_CS_RefitTLAS"


class Pass:
    """The textures of one size over one GpuScene: refit + trace through rhi bindings, targets pre-filled."""

    def __init__(self, dev, gs, W, H, noise):
        from toyrenderer_amd import rhi
        self.dev, self.gs, self.W, self.H = dev, gs, W, H
        self.depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
        self.gbuffer = dev.create_texture(W, H, 1, rhi.FORMAT_RGBA32_UINT, "GBufferA")
        self.mask = dev.create_texture(W, H, 1, rhi.FORMAT_R8_UNORM, "Shadow Mask Texture")
        self.lvd = dev.create_texture(W, H, 1, rhi.FORMAT_R16_FLOAT, "Linear View Depth")
        self.noise = dev.create_texture(128, 128, 1, rhi.FORMAT_RGBA8_UNORM, "Blue Noise", uav=False)
        self.noise.upload_mip(0, accel.noise_words(noise))
        self.cl = dev.create_command_list()

    def refit_bindings(self):
        from toyrenderer_amd.rhi import PUSH, SRV, UAV
        gs, rt = self.gs, self.gs.rt
        return [PUSH(0), SRV(0, gs.instances), SRV(1, rt["headers"]), SRV(2, rt["blas_nodes"]), SRV(3, rt["level_offsets"]), SRV(4, rt["level_nodes"]),
                UAV(0, rt["tlas_nodes"]), UAV(1, rt["tlas_instances"])]

    def refit_push(self):
        k = np.zeros(1, I.RefitTLASConstants)
        k["m_NumInstances"], k["m_NumNodes"], k["m_NumLevels"] = self.gs.numInstances, len(self.gs.rt["tlas"]["nodes"]), self.gs.rt["tlas"]["num_levels"]
        return k

    def trace_bindings(self, cb):
        from toyrenderer_amd.rhi import CB, SAMPLER, SRV, TEX_SRV, TEX_UAV
        gs, rt = self.gs, self.gs.rt
        return [CB(0, cb), TEX_SRV(0, self.depth), SRV(1, rt["tlas_nodes"]), TEX_SRV(2, self.gbuffer), SRV(3, gs.instances), SRV(4, gs.vertices), SRV(5, gs.materials),
                SRV(6, gs.indices), SRV(7, gs.meshData), TEX_SRV(8, self.noise), TEX_UAV(0, self.mask, 0), TEX_UAV(1, self.lvd, 0), SRV(9, rt["tlas_instances"]),
                SRV(10, rt["headers"]), SRV(11, rt["blas_nodes"]), SRV(12, rt["tri_order"]), SAMPLER(0), SAMPLER(1)]

    def groups(self):
        return ((self.W + 7) // 8, (self.H + 7) // 8, 1)

    def run(self, k, depth, g, refit=True):
        self.depth.upload_mip(0, np.ascontiguousarray(depth, F))
        self.gbuffer.upload_mip(0, np.ascontiguousarray(g, np.uint32))
        self.mask.upload_mip(0, np.full((self.H, self.W), SR.SENTINEL8, np.uint8))
        self.lvd.upload_mip(0, np.full((self.H, self.W), SR.SENTINEL16, np.uint16))
        self.cl.open()
        if refit:
            self.cl.dispatch(REFIT, self.refit_bindings(), ((self.gs.numInstances + 63) // 64, 1, 1), push=self.refit_push())
        cb = self.cl.constant_buffer(np.ascontiguousarray(k, I.ShadowMaskConsts), "ShadowMaskConsts")
        self.cl.dispatch(TRACE, self.trace_bindings(cb), self.groups())
        self.cl.close()
        self.dev.execute(self.cl); self.dev.wait_idle()
        return self.mask.download_mip(0), self.lvd.download_mip(0)

    def structure(self):
        rt = self.gs.rt
        return rt["tlas_nodes"].download(I.AccelNode, len(rt["tlas"]["nodes"])), rt["tlas_instances"].download(I.TLASInstance, self.gs.numInstances)

    def release(self):
        self.cl.release()
        for t in (self.depth, self.gbuffer, self.mask, self.lvd, self.noise):
            t.release()


# ---- the references of SS.WALK_CASES, computed once ------------------------------------------------------------------------------------
class WalkCase:
    """One entry of SS.WALK_CASES with its reference: the maker's dict as attributes (sc, k, depth, g, noise, moved, singular,
    info), the structure built from the scene's rest transforms (acc), the instances the passes see (inst: the moved ones, or the
    scene's own), and brute force over them (mask, lvd)."""

    def __init__(self, sm, name):
        self.name = name
        for key, value in SS.WALK_CASES[name](sm).items():
            setattr(self, key, value)
        self.acc = SR.Accel(self.sc)
        self.inst = self.sc["instances"] if self.moved is None else self.moved
        self.mask, self.lvd, _ = SR.trace(sm, self.k, self.acc, self.depth, self.g, self.noise, SR.BRUTE, instances=self.inst)
        self.mask.setflags(write=False); self.lvd.setflags(write=False)
        self.W, self.H = (int(x) for x in self.k["m_OutputResolution"][0])
        self.far = self.depth == 0


_WALK_CASES = {}


def walk_case(sm, name) -> WalkCase:
    if name not in _WALK_CASES:
        _WALK_CASES[name] = WalkCase(sm, name)
    return _WALK_CASES[name]


class UnflaggedCase:
    """suite_support.unflagged_leaves under the sun: 7 instances of the DDGI scene "attributes" keep their leaves, boxes and
    object-from-world rows and lose only their flags.  mask / lvd: brute force, which reads the same flags and skips them;
    restored: brute force with those flags put back, which is what a walk that entered such a leaf would give."""

    def __init__(self, sm, soft):
        import copy

        from suite_support import unflagged_leaves
        self.sc, self.acc, self.off = unflagged_leaves(sm)
        listed = copy.copy(self.acc)
        listed.flags = accel.instance_flags(len(self.sc["instances"]), self.sc["opaqueIds"], self.sc["alphaMaskIds"])
        self.W, self.H = 67, 35
        self.noise = SS.noise_image()
        self.k = SS.consts(self.W, self.H, SS.LIGHTS["x"], soft, 3)
        # Seven leaves among 65 decide few texels of a seeded image (13 of 2345 here), and texels are independent of each other: so
        # each texel takes its depth and normal from the first of 12 seeded images in which those leaves decide it, else from the first.
        for seed in range(77, 89):
            depth, g = SS.images(self.W, self.H, seed)
            mask, lvd, _ = SR.trace(sm, self.k, self.acc, depth, g, self.noise, SR.BRUTE)
            restored, _, _ = SR.trace(sm, self.k, listed, depth, g, self.noise, SR.BRUTE)
            if seed == 77:
                self.depth, self.g, self.mask, self.lvd, self.restored = depth, g, mask, lvd, restored
            take = (mask == 255) & (restored == 0) & ~((self.mask == 255) & (self.restored == 0))
            for mine, theirs in ((self.depth, depth), (self.g, g), (self.mask, mask), (self.lvd, lvd), (self.restored, restored)):
                mine[take] = theirs[take]
        self.far = self.depth == 0


_UNFLAGGED = {}


def unflagged_case(sm, soft) -> UnflaggedCase:
    if soft not in _UNFLAGGED:
        _UNFLAGGED[soft] = UnflaggedCase(sm, soft)
    return _UNFLAGGED[soft]
