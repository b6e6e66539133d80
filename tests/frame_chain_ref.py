"""The whole frame of FrameDriver._record_frame on the CPU, every option on: one chain of the existing references from the scene, the
camera path and the settings to the back buffer, with what the renderer carries from frame to frame (the TAA history, the sigma
history, the adapted luminance, the DDGI volume and its variability state, the previous world-to-clip, the jitter, the HZB).  It takes
NO intermediate of a GPU run: tests/test_gpu_frame_chain.py compares every download and every constant block of both drivers with
it, so an upstream error that is self-consistent on the device shows.  tests/test_frame_chain_ref.py holds the conditions that make
the comparison mean something (no pass vacuous) and ties the chain to the per-pass chains the suite already trusts.

Every constant block is built here from the UNJITTERED view of the frame, the frame number and the settings, through the public
builders; which matrix a pass reads under TAA is the reference project's decision, cited at each block.

The scene (scene()): tests/alpha_test_scenes.py's shadow_scene() -- an opaque floor under open sky and an alpha-mask cut-out above it
-- with the cut-out's albedo as a BC3 texture, the floor's albedo as BC1_SRGB and its normal map as BC5, and an upright texture-free
box of five faces on the floor, which moves between frames 0 and 1 (instances_at()).  A 4 x 4 x 4 probe volume sits round the box.

Not a test module: every assert here says what it compared."""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import alpha_test_ref as AT  # noqa: E402
import alpha_test_scenes as A  # noqa: E402
import bc_blocks as B  # noqa: E402
import bc_passes as P  # noqa: E402
import bc_ref  # noqa: E402
import bloom_ref as BR  # noqa: E402
import ddgi_placement_ref as DP  # noqa: E402
import ddgi_probe_draw_ref as PD  # noqa: E402
import ddgi_ref as DG  # noqa: E402
import ddgi_update_ref as DU  # noqa: E402
import ddgi_variability_frames as VF  # noqa: E402
import ddgi_variability_ref as DV  # noqa: E402
import frame_stream as FS  # noqa: E402
import gtao_ref as GT  # noqa: E402
import lighting_ref as LR  # noqa: E402
import material_texture_scenes as S  # noqa: E402
import material_textures_ref as MT  # noqa: E402
import postprocess_ref as PR  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
import sigma_ref as SG  # noqa: E402
import sky_ref as SK  # noqa: E402
import taa_ref as TR  # noqa: E402
import taa_scenes as TS  # noqa: E402
import visibility_ref as VR  # noqa: E402
from suite_support import halves_to_words  # noqa: E402
from toyrenderer_amd import accel, ddgi, gltf_lite, gtao, sky  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from toyrenderer_amd import taa as T  # noqa: E402
from toyrenderer_amd.frame import culling_frustum  # noqa: E402
from visibility_scenes import consts as basepass_consts  # noqa: E402

F = np.float32
RENDER = FS.RENDER
FRAMES = 3
FLAGS = 7
RECORD_CAPACITY = 4096
LIGHT = (SS.unit((0.15, 0.9, -0.25)), 2.0)           # towards the sun: the cut-out's shadow falls on the floor in view
SKY = (3.0, (0.2, 0.2, 0.2))                         # the everything configuration's turbidity and ground albedo
BLOOM_MIPS, BLOOM_RADIUS, BLOOM_STRENGTH = 3, 0.005, 0.1
AUTO_EXPOSURE = (0.004, 12.0, 0.04)                  # FrameDriver's defaults
PROBE_RADIUS = 0.1
UPDATE = VF.settings()                               # seed 13, relocation, classification, variability at the reference's threshold
T_CUT, T_FLOOR_ALBEDO, T_FLOOR_NORMAL = 0, 1, 2      # descriptor indices of textures()
M_FLOOR, M_CUT, M_BOX = 0, 1, 2                      # material indices
BOX = (2, 3, 4, 5, 6)                                # the instances of the box's faces
BOX_MOVE = (0.3, 0.0, 0.25)                          # its translation from frame 1 on
OPTIONS = ("taa", "alpha_test", "textures", "ao", "shadows", "ddgi", "sky", "bloom", "probes")


# ---- the scene -----------------------------------------------------------------------------------------------------------------------------
def textures():
    """(mips, format): the cut-out's albedo (its alpha decides the discard) as BC3, the floor's albedo as BC1_SRGB and its normal map
    as BC5, each 8 x 8 with its full chain, of tests/bc_blocks.py's blocks."""
    return [(B.block_mips(70, 8, 8, 4, B.BC3), B.BC3), (B.block_mips(71, 8, 8, 4, B.BC1_SRGB), B.BC1_SRGB), (B.block_mips(72, 8, 8, 4, B.BC5), B.BC5)]


def materials(textured=True):
    none = (S.NONE,) * 4
    m = np.concatenate([
        S.material(flags=(S.ALBEDO | S.NORMAL) if textured else 0, albedo=(0.8, 0.8, 0.7, 1.0), indices=(T_FLOOR_ALBEDO, T_FLOOR_NORMAL, S.NONE, S.NONE) if textured else none),
        S.material(flags=S.ALBEDO if textured else 0, albedo=(0.9, 0.8, 0.7, 1.0), indices=(T_CUT, S.NONE, S.NONE, S.NONE) if textured else none),
        S.material(albedo=(0.7, 0.3, 0.2, 1.0))])
    m["m_AlphaCutoff"] = A.CUTOFF
    return m


def _box(cx, cz, half, y0, y1):
    """Five quads, each wound so that (p10 - p00) x (p01 - p00) points out of the box."""
    x0, x1, z0, z1 = cx - half, cx + half, cz - half, cz + half
    uv = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0))
    faces = [((x0, y0, z1), (x1, y0, z1), (x0, y1, z1), (x1, y1, z1), (0.0, 0.0, 1.0)),       # towards the camera
             ((x1, y0, z0), (x0, y0, z0), (x1, y1, z0), (x0, y1, z0), (0.0, 0.0, -1.0)),
             ((x1, y0, z1), (x1, y0, z0), (x1, y1, z1), (x1, y1, z0), (1.0, 0.0, 0.0)),
             ((x0, y0, z0), (x0, y0, z1), (x0, y1, z0), (x0, y1, z1), (-1.0, 0.0, 0.0)),
             ((x0, y1, z1), (x1, y1, z1), (x0, y1, z0), (x1, y1, z0), (0.0, 1.0, 0.0))]
    return [S.quad(*f[:4], *uv, M_BOX, grid=1, normal=f[4]) for f in faces]


BOX_CENTRE, BOX_HALF, BOX_Y = (-0.9, -4.2), 0.4, (-0.6, 0.25)


def scene(textured=True):
    """The scene dict (tests/alpha_test_scenes.py's form) at rest: instance 0 the floor, 1 the cut-out, 2..6 the box."""
    base = A.shadow_scene()
    floor = S.quad((-3.0, -0.6, -1.0), (3.0, -0.6, -1.0), (-3.0, -0.6, -14.0), (3.0, -0.6, -14.0), (0.0, 0.0), (3.0, 0.0), (0.0, 6.0), (3.0, 6.0),
                   M_FLOOR, grid=2, normal=(0.0, 1.0, 0.0))
    cut = S.quad((-1.6, 0.9, -2.5), (1.6, 0.9, -2.5), (-1.6, 0.9, -9.0), (1.6, 0.9, -9.0), (0.0, 0.0), (3.0, 0.0), (0.0, 3.0), (3.0, 3.0),
                 M_CUT, grid=2, normal=(0.0, 1.0, 0.0))
    placed = [(floor, "opaque"), (cut, "alpha")] + [(q, "opaque") for q in _box(*BOX_CENTRE, BOX_HALF, *BOX_Y)]
    sc = A.build(placed, materials(textured), textures() if textured else [])
    sc["meshlets"]["m_ConeAxisAndCutoff"] = 0xFF808080       # cutoff 1: dot(c, axis) < |c| + r, so the cone test (flags bit 2) culls no face
    n = len(base["vertices"])                        # the floor and the cut-out are shadow_scene()'s, position for position
    assert np.array_equal(sc["vertices"]["m_Position"][:n], base["vertices"]["m_Position"]), "the floor and the cut-out of alpha_test_scenes.shadow_scene()"
    return sc


def instances_at(sc, f):
    """The instance buffer of frame f: at rest in frame 0; from frame 1 on the box stands BOX_MOVE further, m_PrevWorldMatrix the
    rest matrix in frame 1 and the moved one from frame 2 on, as the per-frame instance update leaves it."""
    inst = sc["instances"].copy()
    if f >= 1:
        moved = inst["m_WorldMatrix"][list(BOX)].copy()
        moved[:, 3, :3] += np.asarray(BOX_MOVE, F)
        inst["m_WorldMatrix"][list(BOX)] = moved
        if f >= 2:
            inst["m_PrevWorldMatrix"][list(BOX)] = moved
    return inst


def camera():
    """A camera whose tests/taa_scenes.py path starts a little left of the scene's axis at the floor's near end, turned towards the box."""
    return gltf_lite.Camera("frame chain", (0.15, -0.05, 3.32), (0.0, 0.0, 0.0, 1.0), float(np.radians(45.0)), 0.1, RENDER[0] / RENDER[1])


def view_at(f):
    """(the unjittered View of frame f, its eye)."""
    return TS.view_at(camera(), f, RENDER), tuple(F(x) for x in TS.camera_at(camera(), f)[0])


def volume():
    """4 x 4 x 4 probes round the box at rest, as ddgi_variability_frames.driver_volume() is round the Cornell blocks: the lowest layer
    under the floor, the inner probes inside the box, one probe pre-marked inactive."""
    v = ddgi.Volume((BOX_CENTRE[0], 0.05, BOX_CENTRE[1]), (0.55, 0.5, 0.55), (4, 4, 4), normal_bias=0.02, view_bias=0.1, gamma=5.0, relocation=True,
                    classification=True).reset()
    v.data[1, 1, 2, 3] = 1.0
    return v


def driver_settings(off=()):
    """FrameDriver's keywords for the chain with the options in `off` left out: the everything configuration of tests/frame_stream.py."""
    on = lambda name: name not in off                                                     # noqa: E731
    kw = dict(post=True, record_capacity=RECORD_CAPACITY, culling_flags=FLAGS, dir_light=LIGHT, auto_exposure=AUTO_EXPOSURE, alpha_test=on("alpha_test"))
    if on("ao"):
        kw["ao"] = dict()
    if on("shadows"):
        kw["shadows"], kw["shadow_denoise"] = dict(noise=SS.noise_image()), dict()
    if on("ddgi"):
        kw["ddgi"], kw["ddgi_update"] = volume(), dict(UPDATE)
    if on("sky"):
        kw["sky"] = (SK.dataset(), *SKY)
    if on("bloom"):
        kw["bloom_mips"] = BLOOM_MIPS
    if on("taa"):
        kw["taa"] = dict()
    if on("probes") and on("ddgi"):
        kw["probes"] = dict(hide_inactive=True)
    return kw


# ---- the reference libraries -----------------------------------------------------------------------------------------------------------------
class Libraries:
    """Every reference library the chain calls, compiled into one directory.  sigma_ref.c includes the shadow mask's and the alpha
    test's references and ddgi_placement_ref.c the probe update's, so those two serve as theirs."""

    def __init__(self, tmpdir):
        self.at, self.mt, self.bc, self.gt, self.sg = AT.load(tmpdir), MT.load(tmpdir), bc_ref.load(tmpdir), GT.load(tmpdir), SG.load(tmpdir)
        self.dp, self.dv, self.dg, self.lr, self.sk = DP.load(tmpdir), DV.load(tmpdir), DG.load(tmpdir), LR.load(tmpdir), SK.load(tmpdir)
        self.bl, self.pr, self.ta, self.pd = BR.load(tmpdir), PR.load(tmpdir), TR.load(tmpdir), PD.load(tmpdir)


def probe_cull_consts(view, eye, n_probes, radius, hide_inactive):
    """GIProbeVisualizationUpdateConsts (GIRenderer.cpp:687-708): m_ViewToClip (the jittered one under TAA, :693, :705-706) gives the
    frustum, m_P00 and m_P11; m_WorldToView is the view's (:703)."""
    hw, hh = I.hzb_dims(view.renderW, view.renderH)
    k = np.zeros(1, I.GIProbeVisualizationUpdateConsts)
    k["m_NumProbes"], k["m_CameraOrigin"], k["m_Frustum"], k["m_WorldToView"] = n_probes, eye, culling_frustum(view.viewToClip), view.worldToView
    k["m_HZBDimensions"], k["m_P00"], k["m_P11"], k["m_NearPlane"] = (hw, hh), view.viewToClip[0, 0], view.viewToClip[1, 1], view.nearPlane
    k["m_ProbeRadius"], k["m_bHideInactiveProbes"] = radius, int(hide_inactive)
    return k


def host_eye(view):
    """m_Eye of csrc/host/Scene.cpp's View::Update: the point m_WorldToView maps to the origin, -t R^T summed left to right in binary32."""
    V = np.asarray(view.worldToView, F)
    return tuple(F(-F(F(F(V[3, 0] * V[j, 0]) + F(V[3, 1] * V[j, 1])) + F(V[3, 2] * V[j, 2]))) for j in range(3))


def nodes_at(sc, f):
    """The host mirror's form of instances_at(): one identity node per instance, the box's nodes at BOX_MOVE from frame 1 on."""
    n = len(sc["instances"])
    nodes = np.zeros(n, I.NodeLocalTransform)
    nodes["m_ParentNodeIdx"], nodes["m_Scale"] = 0xFFFFFFFF, 1.0
    nodes["m_Rotation"][:, 3] = 1.0
    if f >= 1:
        nodes["m_Position"][list(BOX)] = BOX_MOVE
    return nodes


def ddgi_consts(update):
    """The DDGIUpdateConsts of recorded update number `update` (GIRenderer.cpp:111-118 and :98; the rotation is the driver's draw)."""
    u = ddgi.check_update_settings(UPDATE)
    k = DU.consts(light=LIGHT, rotation=ddgi.random_rotation(np.random.default_rng([u["seed"], update])), max_ray_distance=u["max_ray_distance"], hysteresis=u["hysteresis"],
                  distance_exponent=u["distance_exponent"], irradiance_threshold=u["irradiance_threshold"], brightness_threshold=u["brightness_threshold"])
    k["probeMinFrontfaceDistance"], k["probeFixedRayBackfaceThreshold"] = u["min_frontface_distance"], u["fixed_ray_backface_threshold"]
    return k


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------------
class Chain:
    """The renderer's state between frames; frame(f) runs frame f (call them in order from 0) and returns a dict of every
    intermediate ("depth", "vis", ...), every constant block ("*_consts") and the counters of the non-vacuity conditions
    ("counters").  off: the options of OPTIONS left out; what they would write is absent from the dict.  For the host mirror:
    consts_of(update), the DDGIUpdateConsts of an update (the mirror draws its rotation from another generator); frame_number(f),
    g_Graphic.m_FrameCounter in frame f (Graphic::Update counts before it records: f + 1); eye_of(view), m_Eye as the mirror
    derives it from the world-to-view matrix it is handed (host_eye)."""

    def __init__(self, L, oracle, sc=None, off=(), consts_of=ddgi_consts, frame_number=lambda f: f, eye_of=None):
        unknown = set(off) - set(OPTIONS)
        assert not unknown, f"unknown options {sorted(unknown)}"
        self.L, self.oracle, self.off = L, oracle, tuple(off)
        self.sc = scene(textured=self.on("textures")) if sc is None else sc
        self.consts_of, self.frame_number, self.eye_of = consts_of, frame_number, eye_of
        W, H = RENDER
        self.hzb = oracle.HzbTexture(*I.hzb_dims(W, H))                                   # cleared to far, as FrameDriver's and GBufferRenderer::Initialize's
        self.twins = P.twins(L.bc, self.sc["textures"])
        self.table = [MT.Texture(*t) for t in self.twins]
        self.acc = SR.Accel(self.sc)                                                      # the topology of the rest transforms, as set_raytracing builds it
        self.last = None                                                                  # (jitter, world-to-clip) of the previous frame
        self.taa_history, self.sigma_history = np.zeros((H, W, 4), np.uint16), np.zeros((H, W), np.uint16)
        self.luminance = F(1.0)
        self.noise = SS.noise_image()
        self.penumbra_init = None                                                         # what the penumbra texture held (default: the sentinel): texels at the far plane keep it
        if self.on("ddgi"):
            self.vol = volume()
            self.vol.variability = True
            self.rays, self.var = np.zeros((64, DU.RAYS, 4), F), np.zeros(DV.variability_shape(self.vol), F)
            self.tracker = ddgi.VariabilityTracker(UPDATE["variability_threshold"])
            self.pending, self.calls, self.updates = [None, None], 0, 0

    def on(self, name):
        return name not in self.off and not (name == "probes" and "ddgi" in self.off)

    def frame(self, f):
        L, sc, W, H = self.L, self.sc, *RENDER
        out, n = dict(frame=f), dict()
        number = self.frame_number(f)                                                     # g_Graphic.m_FrameCounter of this frame
        view, eye = view_at(f)
        if self.eye_of is not None:
            eye = self.eye_of(view)
        inst = instances_at(sc, f)
        scf = dict(sc, instances=inst)
        # ---- View::Update (Scene.cpp:113-133): the jitter, the jittered projection, the previous world-to-clip ------------------------
        if self.on("taa"):
            current = TR.jitter_sequence(number + 1)[number]                              # Scene.cpp:114
            jittered = dataclasses.replace(view, viewToClip=T.jittered_view_to_clip(view.viewToClip, current, W, H))   # Scene.cpp:127-131
        else:
            current, jittered = (F(0.0), F(0.0)), view
        w2c = I.world_to_clip(jittered.worldToView, jittered.viewToClip)                 # Scene.cpp:133
        c2w = I.clip_to_world(jittered.worldToView, jittered.viewToClip)                 # Scene.cpp:134
        if self.on("taa"):
            previous, prev_w2c = self.last if self.last is not None else (current, w2c)   # Scene.cpp:113, :119
        else:
            previous, prev_w2c = current, I.world_to_clip(view.prevWorldToView, view.viewToClip)
        self.last = (current, w2c)
        out.update(jitter=(current, previous), view=jittered, unjittered_view=view, eye=eye, instances=inst, world_to_clip=w2c, prev_world_to_clip=prev_w2c)

        # ---- the cull, the rasters, both HZB builds (BasePassRenderers.cpp:341-347, :446-453, :557: all from the jittered m_ViewToClip) ----
        ref = self.oracle.frame(scf, jittered.as_dict(), self.hzb, np.zeros((H, W), F), cullingFlags=FLAGS, record_capacity=RECORD_CAPACITY,
                                raster=(w2c, sc["vertices"], sc["vertexIds"], sc["triangles"]))
        k = basepass_consts(jittered)
        k["m_PrevWorldToClip"] = prev_w2c                                                 # BasePassRenderers.cpp:447
        geo = VR.Geometry(scf, sc["vertices"], sc["vertexIds"], sc["triangles"])
        alpha = self.on("alpha_test")
        vis, depth, kept = AT.frame_raster(L.at, k, geo, ref, W, H, sc["materials"], self.twins, alpha)
        self.hzb.build_from_depth(depth)                                                  # the frame's last GenerateHZB, from the alpha-tested depth
        recs = [ref.records[s] if ref.passRan[s] else None for s in range(4)]
        lsts = [ref.visibleList[s] if ref.passRan[s] else None for s in range(4)]
        g, m, taps = MT.gbuffer(L.mt, k, geo, recs, lsts, vis, sc["materials"], self.table, 0)
        motion = halves_to_words(VR.to_half_bits(m))
        out.update(cull=ref, vis=vis, depth=depth, hzb=self.hzb.texels.copy(), gbuffer=g, motion=motion, taps=taps, basepass_consts=k)
        _, slot, pos, _ = VR.decode(vis)
        owner = np.full((H, W), -1, np.int64)
        for s in range(4):
            if ref.passRan[s]:
                sel = (vis != 0) & (slot == s)
                owner[sel] = ref.records[s].view(I.MeshletAmplificationData)["m_InstanceConstIdx"][ref.visibleList[s][pos[sel]] >> 5]
        out["owner"] = owner
        n.update(covered=int((depth > 0).sum()), sky=int((depth <= 0).sum()), alpha_kept=int(kept[0] + kept[2]), alpha_discarded=int(kept[1] + kept[3]),
                 alpha_slot_ran=bool(ref.passRan[2] or ref.passRan[3]), taps=[int((taps[..., i] > 0).sum()) for i in range(4)],
                 taps_by_texture={"BC3 albedo": int((taps[owner == 1][:, 0] > 0).sum()), "BC1_SRGB albedo": int((taps[owner == 0][:, 0] > 0).sum()),
                                  "BC5 normal": int((taps[owner == 0][:, 1] > 0).sum())},
                 box_motion=int((motion[np.isin(owner, BOX)] != 0).sum()), box_texels=int(np.isin(owner, BOX).sum()))

        # ---- XeGTAO (AmbientOcclusionRenderer.cpp:136: the jittered m_ViewToClip; :179: m_WorldToView) ----------------------------------
        ssao = None
        if self.on("ao"):
            settings = gtao.check_settings({})
            gk = gtao.update_constants(W, H, settings, jittered.viewToClip, number % 256)
            ao = GT.frame(L.gt, gk, gtao.main_pass_constants(jittered.worldToView, settings["quality"]), depth, g, settings["denoise_passes"])
            ssao = ao["ssao"]
            out.update(gtao_consts=gk, ao_chain=ao["chain"], ao_edges=ao["edges"], ao_working=ao["working"], ssao=ssao)
            n["ssao_below_255"] = int((ssao[depth > 0] < 255).sum())

        # ---- the probe update (GIRenderer.cpp:464-576), in front of lighting as FrameDriver records it --------------------------------------
        if self.on("ddgi"):
            before = self.vol.copy()
            call = self.calls
            self.calls += 1
            skipped = self.tracker.update()
            n["ddgi_skipped"] = bool(skipped)
            if not skipped:
                dk = self.consts_of(self.updates)
                self.updates += 1
                world = DU.Scene(L.sg, self.acc, inst)                                    # the TLAS refitted to this frame's matrices
                self.rays, fixed = DP.update(L.dp, dk, self.vol, world, rays_init=self.rays)
                irr, self.var, _ = DV.blend_radiance(L.dv, dk, before, self.rays, self.var)
                assert np.array_equal(irr, self.vol.irradiance), "the two statements of the radiance blend"
                slot_ = call % 2
                self.tracker.set(F(0.0) if self.pending[slot_] is None else self.pending[slot_])
                average, _, passes = DV.average(L.dv, self.vol, self.var)                 # behind placement: the data the reductions read
                self.pending[slot_] = average
                out.update(ddgi_update_consts=dk, ddgi_rays=self.rays.copy(), ddgi_fixed_rays=fixed, ddgi_variability=self.var.copy(), ddgi_average=average)
                n.update(reduction_passes=passes)
            out["volume"] = self.vol.copy()
            n.update(irradiance_changed=int((self.vol.irradiance != before.irradiance).sum()), probes_moved=int(np.any(self.vol.data[..., :3] != before.data[..., :3], -1).sum()),
                     probes_switched=int((self.vol.data[..., 3] != before.data[..., 3]).sum()))

        # ---- the sun shadows and their denoiser (ShadowMaskRenderer.cpp:267: m_ClipToWorld; :350: m_ViewToClip; :356-359: both jitters) ------
        mask = None
        if self.on("shadows"):
            shadows = accel.check_settings(dict(noise=self.noise))
            sk = accel.shadow_consts(c2w, LIGHT[0], eye, W, H, shadows, number, denoise=True)
            table = self.twins if alpha and len(self.twins) else None                     # the trace binds the table with alpha_test on a textured scene
            pen, lvd, _ = SG.trace_penumbra(L.sg, sk, self.acc, depth, g, self.noise, SG.BRUTE, textures=table, instances=inst, penumbra=self.penumbra_init)
            delta = T.jitter_delta(current, previous)
            gk_ = accel.sigma_consts(c2w, jittered.viewToClip, W, H, accel.check_denoise_settings({}), number, 0, f == 0, delta)
            r = SG.denoise(L.sg, gk_, pen, lvd, depth, g, motion, self.sigma_history)
            self.sigma_history, mask = r["history"], r["mask"]
            out.update(shadow_consts=sk, sigma_consts=gk_, penumbra=pen, linear_view_depth=lvd, shadow_tiles=r["tiles"], shadow_history=r["history"], shadow_mask=mask,
                       normal_roughness=r["normal_roughness"], sigma_path=r["path"])
            solid, _, _ = SG.trace_penumbra(L.sg, sk, self.acc, depth, g, self.noise, SG.BRUTE, textures=None, instances=inst)
            raw = np.where(pen < SG.NO_OCCLUDER, 0, 255)
            floor_ = (owner == 0)
            under = floor_ & (solid < SG.NO_OCCLUDER)                                     # the floor texels in the solid card's shadow
            n.update(floor_lit=int((floor_ & (pen == SG.NO_OCCLUDER)).sum()), floor_shadowed=int((floor_ & (pen < SG.NO_OCCLUDER)).sum()),
                     behind_kept=int((under & (pen < SG.NO_OCCLUDER)).sum()), behind_discarded=int((under & (pen == SG.NO_OCCLUDER)).sum()),
                     denoised_differs=int(((mask != raw) & (depth > 0)).sum()), sigma_history_reads=int(r["reads"]),
                     sigma_history_texels=int(((r["path"] & SG.PATH_HISTORY) != 0).sum()))

        # ---- deferred lighting (DeferredLightingRenderer.cpp:65, :68: m_Eye and the jittered m_ClipToWorld) ----------------------------------
        lk = LR.consts(c2w, eye, LIGHT[0], LIGHT[1], (W, H), 0, ssao_enabled=int(ssao is not None))
        lk["m_bRTDDGIEnabled"] = int(self.on("ddgi"))                                     # DeferredLightingRenderer.cpp:72
        if self.on("ddgi"):
            lit = DG.lighting(L.dg, lk, self.vol, g, depth, ssao=ssao, shadow=mask, motion=motion)
        else:
            lit = LR.lighting(L.lr, lk, g, depth, ssao=ssao, shadow=mask, motion=motion)
        out.update(lighting_consts=lk, lighting_before_sky=lit)

        # ---- the sky onto the texels nothing was drawn to (SkyRenderer.cpp:179, :181) -------------------------------------------------------------
        if self.on("sky"):
            sun = np.asarray(LIGHT[0], F)
            kk = sky.pass_parameters(c2w, sun, eye, sky.sky_parameters(SK.dataset(), F(SKY[0]), tuple(F(x) for x in SKY[1]), sun))
            lit = SK.sky_pass(L.sk, kk, depth, dest=lit)
            out["sky_consts"] = kk
            n["sky_filled"] = int((lit != out["lighting_before_sky"]).sum())
        out["lighting_output"] = lit

        # ---- bloom, the histogram and the exposure: all three read LightingOutput behind the sky (Scene.cpp:502-505) ----------------------------
        bloom = None
        if self.on("bloom"):
            bloom = BR.bloom_chain(L.bl, lit, W, H, BLOOM_MIPS, BLOOM_RADIUS)
            out.update(bloom=bloom, bloom_consts=BR.pass_consts(W, H, BLOOM_MIPS, F(BLOOM_RADIUS)))
            n["bloom_mip0_nonzero"] = int((bloom[0] != 0).sum())
        hk = PR.histogram_params((W, H), AUTO_EXPOSURE[0], AUTO_EXPOSURE[1])
        ak = PR.adapt_params(W * H, AUTO_EXPOSURE[2], 0.18, AUTO_EXPOSURE[0], AUTO_EXPOSURE[1])
        histogram = PR.histogram(L.pr, lit, hk)
        self.luminance, exposure = PR.adapt_exposure(L.pr, ak, histogram, self.luminance)
        out.update(histogram=histogram, luminance=self.luminance, exposure=exposure)
        n["luminance"] = float(self.luminance)

        # ---- the TAA resolve (TAARenderer.cpp:273-275 for the inputs) -------------------------------------------------------------------------------
        colour = lit
        if self.on("taa"):
            tk = TR.consts(W, H, T.jitter_delta(current, previous), T.DEFAULTS["min_blend"], T.DEFAULTS["max_sample_count"], reset=f == 0)
            self.taa_history, colour, path = TR.resolve(L.ta, tk, lit, depth, motion, self.taa_history)
            out.update(taa_consts=tk, taa_history=self.taa_history, anti_aliased_output=colour, taa_path=path)
            n.update(taa_differs=int((colour != lit).sum()), taa_valid=int(((path & TR.VALID) != 0).sum()))

        # ---- the post pass on the anti-aliased output (PostProcessRenderer.cpp:25-27, :52) -------------------------------------------------------
        pk = PR.post_params((W, H), 0.0, 0.18, bloom_strength=BLOOM_STRENGTH if bloom is not None else 0.0)
        back = PR.post(L.pr, pk, colour, bloom=None if bloom is None else bloom[0], luminance_in=self.luminance)
        out.update(post_consts=(hk, ak, pk), back_buffer_before_probes=back)

        # ---- the probe draw (GIRenderer.cpp:672-808): the live volume, the frame's HZB and depth, onto the back buffer --------------------------
        if self.on("probes"):
            positions, states = PD.load_probes(L.pd, self.vol)
            hzb = self.oracle.HzbTexture(*I.hzb_dims(W, H))
            hzb.texels[:] = self.hzb.texels
            ck = probe_cull_consts(jittered, eye, len(positions), PROBE_RADIUS, True)
            culled, args, to_probe = self.oracle.gi_probe_cull(ck, positions, states, hzb, draw_args=np.array([I.kUnitSphereIndices, 0, 0, 0, 0], np.uint32))
            full_pos, full_idx = np.zeros((len(positions), 3), F), np.zeros(len(positions), np.uint32)
            full_pos[:len(to_probe)], full_idx[:len(to_probe)] = culled.reshape(-1, 3), to_probe
            dk_ = PD.consts(w2c, PROBE_RADIUS, jittered.nearPlane, camera_direction=-np.asarray(jittered.worldToView, F)[:3, 2])   # GIRenderer.cpp:750
            winners, back, depth_after, drawn = PD.draw(L.pd, dk_, self.vol, full_pos, full_idx, int(args[1]), depth, back)
            out.update(probe_cull_consts=ck, probe_draw_consts=dk_, probe_positions=positions, probe_states=states, probe_culled_positions=culled.reshape(-1, 3),
                       probe_draw_args=args, probe_instance_to_probe=to_probe, probe_winners=winners, depth_after_probes=depth_after)
            n.update(probes_won=drawn["won"], probes_lost_to_scene=drawn["lost_to_scene"], probes_drawn=int(args[1]))
        out["back_buffer"] = back
        out["counters"] = n
        return out


def run(L, oracle, frames=FRAMES, **kw):
    """The dicts of `frames` consecutive frames."""
    c = Chain(L, oracle, **kw)
    return [c.frame(f) for f in range(frames)]
