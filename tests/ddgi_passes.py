"""What the DDGI GPU test modules share (tests/test_gpu_ddgi_update.py, tests/test_gpu_ddgi_placement.py,
tests/test_gpu_ddgi_trace_scenes.py, tests/test_gpu_ddgi_blend_rules.py): the passes of the probe update and of probe placement through rhi
bindings, and the references of tests/ddgi_update_scenes.py TRACE_CASES, computed once
per process.  Not a test module: every assert here says what it compared."""
import numpy as np

import ddgi_placement_ref as DP
import ddgi_update_ref as DU
import ddgi_update_scenes as US
import shadowmask_ref as SR
from toyrenderer_amd import interop as I

F = np.float32
TRACE = "giprobetrace_CS_ProbeTrace"
BLEND_RADIANCE = "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1"
BLEND_DISTANCE = "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0"
FIXED = "giprobetrace_CS_ProbeTraceFixedRays"
RELOCATION = "ProbeRelocationCS_DDGIProbeRelocationCS"
CLASSIFICATION = "ProbeClassificationCS_DDGIProbeClassificationCS"
RAY_SENTINEL = F(7.5)                             # pre-fill of the ray records: an inactive probe's keep it
DISTANCE_SENTINEL = F(-7.5)                       # pre-fill of the fixed-ray distances: the trace writes every word


def _record_refit(cl, gs):
    from toyrenderer_amd.rhi import PUSH, SRV, UAV
    rt = gs.rt
    k = np.zeros(1, I.RefitTLASConstants)
    k["m_NumInstances"], k["m_NumNodes"], k["m_NumLevels"] = gs.numInstances, len(rt["tlas"]["nodes"]), rt["tlas"]["num_levels"]
    cl.dispatch("raytracing_CS_RefitTLAS", [PUSH(0), SRV(0, gs.instances), SRV(1, rt["headers"]), SRV(2, rt["blas_nodes"]), SRV(3, rt["level_offsets"]),
                                            SRV(4, rt["level_nodes"]), UAV(0, rt["tlas_nodes"]), UAV(1, rt["tlas_instances"])],
                ((gs.numInstances + 63) // 64, 1, 1), push=k)


def refitted_structure(gs):
    """(TLAS nodes, TLAS instance records) as the last refit left them on the device."""
    rt = gs.rt
    return rt["tlas_nodes"].download(I.AccelNode, len(rt["tlas"]["nodes"])), rt["tlas_instances"].download(I.TLASInstance, gs.numInstances)


class Update:
    """One volume's device resources and the three passes of the update through rhi bindings."""

    def __init__(self, dev, vol, gs=None, uav=True):
        self.dev, self.vol, self.gs = dev, vol, gs
        self.desc, self.data, self.irr, self.dist = vol.upload(dev, uav=uav)
        self.n = int(np.prod(vol.counts))
        self.rays = dev.create_buffer(self.n * DU.RAYS * 16, "DDGI Ray Data", stride=16)
        self.cl = dev.create_command_list()

    def block(self, k):
        return np.frombuffer(np.ascontiguousarray(k, I.DDGIUpdateConsts).tobytes() + self.vol.desc().tobytes(), np.uint8)

    def trace_bindings(self, cb):
        from toyrenderer_amd.rhi import CB, SAMPLER, SRV, TEX_SRV, UAV
        gs, rt = self.gs, self.gs.rt
        return [CB(0, cb), SRV(0, self.desc), TEX_SRV(1, self.data), TEX_SRV(2, self.irr), TEX_SRV(3, self.dist), SRV(4, rt["tlas_nodes"]), SRV(5, gs.instances),
                SRV(6, gs.vertices), SRV(7, gs.materials), SRV(8, gs.indices), SRV(9, gs.meshData), SRV(10, rt["tlas_instances"]), SRV(11, rt["headers"]),
                SRV(12, rt["blas_nodes"]), SRV(13, rt["tri_order"]), UAV(0, self.rays), SAMPLER(0), SAMPLER(1), SAMPLER(2)]

    def trace_groups(self):
        cx, cy, cz = self.vol.counts
        return (DU.RAYS // 64, cx * cz, cy)

    def blend_bindings(self, cb, radiance):
        from toyrenderer_amd.rhi import CB, SRV, TEX_SRV, TEX_UAV
        return [CB(0, cb), SRV(1, self.rays), TEX_SRV(3, self.data), TEX_UAV(1, self.irr, 0) if radiance else TEX_UAV(2, self.dist, 0)]

    def blend_groups(self):
        cx, cy, cz = self.vol.counts
        return (cx, cz, cy)

    def refit(self):
        _record_refit(self.cl, self.gs)

    def run_trace(self, k):
        self.rays.upload(np.full(self.n * DU.RAYS * 4, RAY_SENTINEL, F))
        self.cl.open()
        self.refit()
        self.cl.dispatch(TRACE, self.trace_bindings(self.cl.constant_buffer(self.block(k), "DDGIUpdateConsts")), self.trace_groups())
        self.cl.close()
        self.dev.execute(self.cl); self.dev.wait_idle()
        return self.rays.download(F).reshape(self.n, DU.RAYS, 4)

    def run_blends(self, k, rays):
        self.rays.upload(np.ascontiguousarray(rays, F).reshape(-1))
        self.cl.open()
        cb = self.cl.constant_buffer(self.block(k), "DDGIUpdateConsts")
        self.cl.dispatch(BLEND_RADIANCE, self.blend_bindings(cb, True), self.blend_groups())
        self.cl.dispatch(BLEND_DISTANCE, self.blend_bindings(cb, False), self.blend_groups())
        self.cl.close()
        self.dev.execute(self.cl); self.dev.wait_idle()
        return self.textures()

    def textures(self):
        cy = self.vol.counts[1]
        irr = np.stack([self.irr.download_slice(s) for s in range(cy)])
        dist = np.stack([self.dist.download_slice(s) for s in range(cy)]).reshape(self.vol.distance.shape)
        return irr, dist

    def release(self):
        self.cl.release()
        for r in (self.desc, self.data, self.irr, self.dist, self.rays):
            r.release()


class Placement:
    """One volume's device resources and the three passes of probe placement through rhi bindings."""

    def __init__(self, dev, vol, gs=None, data_uav=True):
        self.dev, self.vol, self.gs = dev, vol, gs
        self.desc, self.data, self.irr, self.dist = vol.upload(dev, data_uav=data_uav)
        self.n = int(np.prod(vol.counts))
        self.distances = dev.create_buffer(self.n * DP.FIXED * 4, "DDGI Fixed Ray Distances", stride=4)
        self.cl = dev.create_command_list()

    def block(self, k):
        return np.frombuffer(np.ascontiguousarray(k, I.DDGIUpdateConsts).tobytes() + self.vol.desc().tobytes(), np.uint8)

    def fixed_bindings(self, cb):
        from toyrenderer_amd.rhi import CB, SRV, TEX_SRV, UAV
        gs, rt = self.gs, self.gs.rt
        return [CB(0, cb), SRV(0, self.desc), TEX_SRV(1, self.data), SRV(4, rt["tlas_nodes"]), SRV(5, gs.instances), SRV(6, gs.vertices), SRV(8, gs.indices), SRV(9, gs.meshData),
                SRV(10, rt["tlas_instances"]), SRV(11, rt["headers"]), SRV(12, rt["blas_nodes"]), SRV(13, rt["tri_order"]), UAV(0, self.distances)]

    def fixed_groups(self):
        return ((self.n * DP.FIXED + 63) // 64, 1, 1)

    def place_bindings(self, cb):
        from toyrenderer_amd.rhi import CB, TEX_UAV, UAV
        return [CB(0, cb), UAV(0, self.distances), TEX_UAV(3, self.data, 0)]

    def place_groups(self):
        return ((self.n + 31) // 32, 1, 1)

    def refit(self):
        _record_refit(self.cl, self.gs)

    def run_fixed(self, k):
        self.distances.upload(np.full(self.n * DP.FIXED, DISTANCE_SENTINEL, F))
        self.cl.open()
        self.refit()
        self.cl.dispatch(FIXED, self.fixed_bindings(self.cl.constant_buffer(self.block(k), "DDGIUpdateConsts")), self.fixed_groups())
        self.cl.close()
        self.dev.execute(self.cl); self.dev.wait_idle()
        return self.distances.download(F).reshape(self.n, DP.FIXED)

    def run_place(self, k, names, distances=None):
        """Dispatches the passes of `names` in order on what the data texture holds (and `distances`, if given); returns the data."""
        if distances is not None:
            self.distances.upload(np.ascontiguousarray(distances, F).reshape(-1))
        self.cl.open()
        cb = self.cl.constant_buffer(self.block(k), "DDGIUpdateConsts")
        for name in names:
            self.cl.dispatch(name, self.place_bindings(cb), self.place_groups())
        self.cl.close()
        self.dev.execute(self.cl); self.dev.wait_idle()
        return self.download_data()

    def upload_data(self, data):
        for s in range(self.vol.counts[1]):
            self.data.upload_slice(s, np.ascontiguousarray(data[s]))

    def download_data(self):
        return np.stack([self.data.download_slice(s) for s in range(self.vol.counts[1])]).reshape(self.vol.data.shape)

    def release(self):
        self.cl.release()
        for r in (self.desc, self.data, self.irr, self.dist, self.distances):
            r.release()


# ---- the references of US.TRACE_CASES, computed once ----------------------------------------------------------------------------------
class TraceCase:
    """One entry of US.TRACE_CASES with its reference: the scene dict (sc), its structure (acc), the instances the trace sees (inst:
    the moved ones, or the scene's own), the reference scene refitted to them (scene), the constants (k), a fresh volume per call of
    volume(), and the reference trace over a buffer pre-filled with RAY_SENTINEL (rays, kinds; DU.WALK)."""

    def __init__(self, sm, lib, name):
        make, moved, self.volume, self.k = US.TRACE_CASES[name]
        self.name, self.sc = name, make()
        self.acc = SR.Accel(self.sc)
        self.inst = self.sc["instances"] if moved is None else moved(self.sc)
        self.scene = DU.Scene(sm, self.acc, self.inst)
        vol = self.volume()
        self.init = np.full((int(np.prod(vol.counts)), DU.RAYS, 4), RAY_SENTINEL, F)
        self.rays, self.kinds = DU.trace(lib, self.k, vol, self.scene, DU.WALK, self.init)
        self.rays.setflags(write=False); self.kinds.setflags(write=False)

    def hits(self, lib, mode=DU.WALK, scene=None, tmax=None):
        """DU.closest over the probes' own 256 rays each: Hit [numProbes, 256]."""
        vol = self.volume()
        pos, _ = DU.probe_positions(lib, vol)
        d = DU.ray_directions(lib, self.k)
        o = np.repeat(pos, DU.RAYS, axis=0)
        h, _ = DU.closest(lib, self.scene if scene is None else scene, o, np.tile(d, (len(pos), 1)), mode, tmax=float(self.k["probeMaxRayDistance"][0]) if tmax is None else tmax)
        return h.reshape(len(pos), DU.RAYS)


_TRACE_CASES = {}


def trace_case(sm, lib, name) -> TraceCase:
    if name not in _TRACE_CASES:
        _TRACE_CASES[name] = TraceCase(sm, lib, name)
    return _TRACE_CASES[name]


# ---- the generated city as the frame-level trace test sees it -----------------------------------------------------------------------------
def city_trace_scene(tmp_path, oracle):
    """The generated city with seeded normals and materials, as the shadow tests' test_city_frame sets it up: (loaded scene, cached
    scene, vertices, materials, scene dict for SR.Accel, (lo, hi) of its world-space bounds)."""
    from gbuffer_scenes import with_normals_and_materials
    from toyrenderer_amd import cached_scene
    from visibility_scenes import city
    s, sc0 = city(tmp_path, oracle, lods=False)
    v, sc0, mats = with_normals_and_materials(s, sc0)
    c = cached_scene.from_scene(s)
    s.meshData = c.meshData
    sc = dict(vertices=v, indices=c.indices, meshData=c.meshData, index_counts=c.meshSpecific["m_NumIndices"], instances=sc0["instances"], opaqueIds=s.opaqueIds,
              alphaMaskIds=s.alphaMaskIds, materials=mats)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in sc0["instances"]:
        m = int(inst["m_MeshDataIdx"])
        vb, ib, n = int(c.meshData["m_GlobalVertexBufferIdx"][m]), int(c.meshData["m_GlobalIndexBufferIdx"][m]), int(sc["index_counts"][m])
        W = inst["m_WorldMatrix"].astype(np.float64)
        p = v["m_Position"][vb + c.indices[ib:ib + n]].astype(np.float64) @ W[:3, :3] + W[3, :3]
        lo, hi = np.minimum(lo, p.min(0)), np.maximum(hi, p.max(0))
    return s, c, v, mats, sc, (lo, hi)


def city_volume(bounds):
    """3 x 2 x 3 probes, the first and the last in opposite corners of the city's bounds; cleared."""
    return US.trace_volume((3, 2, 3), bounds[0], bounds[1], seeded=False)
