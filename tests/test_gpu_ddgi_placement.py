"""Probe placement on the GPU ("giprobetrace_CS_ProbeTraceFixedRays", "ProbeRelocationCS_DDGIProbeRelocationCS",
"ProbeClassificationCS_DDGIProbeClassificationCS"; csrc/k_giprobeplacement.hip), every word against tests/ddgi_placement_ref.c: each
pass dispatched directly on the scenes of tests/ddgi_placement_scenes.py, relocation and classification from a supplied distance
buffer, volumes of 1, 2, 3 and 33 probes, three chained updates through FrameDriver(ddgi_update=dict(relocate=True, classify=True)),
two through the host mirror, what is recorded with both options off, and misuse."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_placement_ref as DP  # noqa: E402
import ddgi_placement_scenes as PS  # noqa: E402
import ddgi_update_ref as DU  # noqa: E402
import ddgi_update_scenes as US  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from ddgi_passes import CLASSIFICATION, FIXED, RELOCATION, Placement  # noqa: E402
from suite_support import bare_gpu_scene, dev, gpu_scene, recorded, ref_library, same, sm  # noqa: E402, F401
from toyrenderer_amd import ddgi, gltf_lite  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
dp = ref_library(DP)
UPDATE = ["giprobetrace_CS_ProbeTrace", "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=1", "ProbeBlendingCS_DDGIProbeBlendingCS RTXGI_DDGI_BLEND_RADIANCE=0"]
CORNELL_MIN_FRONT = 0.1                           # GIRenderer.cpp:98: the fixture's bounding radius is below 3


def _bits(data):
    return np.ascontiguousarray(data).view(np.uint16)


@pytest.fixture(scope="module")
def cornell(dev, oracle, sm):
    """The Cornell fixture as the frames have it, with its acceleration structure: (scene dict, GpuScene, reference scene)."""
    sc = SS.cornell()
    s = sc["loaded"]
    inst = sc["instances"].copy()
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    sc["instances"] = inst
    s.meshData = sc["meshData"]
    gs = gpu_scene(dev, s, inst, s.vertices, sc["materials"])
    gs.set_raytracing(sc["indices"], sc["cached"].meshSpecific)
    yield sc, gs, DU.Scene(sm, SR.Accel(sc))
    gs.release()


@pytest.fixture(scope="module")
def closed_cube(dev, sm):
    sc = US.closed_cube()
    gs = bare_gpu_scene(dev, sc)
    yield sc, gs, DU.Scene(sm, SR.Accel(sc))
    gs.release()


# ---- 1. each pass, dispatched directly ----------------------------------------------------------------------------------------------------
VOLUMES = {"tight": (PS.tight_volume, "cornell", CORNELL_MIN_FRONT), "tight, offsets": (lambda: PS.tight_volume(True), "cornell", CORNELL_MIN_FRONT),
           "3x2x4, seeded": (lambda: PS.cornell_volume("3x2x4", True), "cornell", CORNELL_MIN_FRONT), "closed cube": (PS.cube_volume, "closed cube", CORNELL_MIN_FRONT)}
VOLUMES.update({f"wide {i}": ((lambda i=i: PS.wide_volume(i)), "cornell", 0.3) for i in range(3)})
VOLUMES.update({f"{int(np.prod(c))} probes": ((lambda c=c: PS.ragged_volume(c)), "cornell", CORNELL_MIN_FRONT) for c in PS.RAGGED_COUNTS})


@pytest.mark.parametrize("name", list(VOLUMES))
def test_each_pass_matches_the_reference(dev, dp, cornell, closed_cube, name):
    """The fixed-ray trace, then relocation on its distances, then classification on the relocated data, each a dispatch of its
    own: every word of the distance buffer and of the data texture equals the reference after each.  The volumes are the ones
    tests/test_ddgi_placement_ref.py names the branches of; those of 1, 2, 3 and 33 probes are the wave that holds one probe and the
    ragged last group of both dispatch shapes.  The trace is run from the relocated positions once more: it reads data.xyz."""
    make, which, min_front = VOLUMES[name]
    sc, gs, scene = cornell if which == "cornell" else closed_cube
    vol = make()
    k = DP.consts(min_frontface_distance=min_front, rotation=US.rotation(3))      # a rotation in the block: the fixed rays must not take it
    p = Placement(dev, vol, gs)
    try:
        got = p.run_fixed(k)
        want = DP.trace_fixed(dp, k, vol, scene)
        same(got.view(np.uint32), want.view(np.uint32), f"{name}: fixed-ray distances")
        moved, branches = DP.relocate(dp, k, vol, want)
        same(_bits(p.run_place(k, [RELOCATION])), _bits(moved), f"{name}: data after relocation")
        vol.data = moved
        switched, reasons = DP.classify(dp, k, vol, want)
        same(_bits(p.run_place(k, [CLASSIFICATION])), _bits(switched), f"{name}: data after classification")
        vol.data = switched
        same(p.run_fixed(k).view(np.uint32), DP.trace_fixed(dp, k, vol, scene).view(np.uint32), f"{name}: fixed-ray distances from the relocated probes")
        if name == "tight":
            assert np.count_nonzero(branches == DP.A_TAKEN) == 12 and np.count_nonzero(reasons == DP.OFF_BACKFACES) == 15
    finally:
        p.release()


def test_relocation_and_classification_from_a_supplied_distance_buffer(dev, dp):
    """No trace: seeded distances with a probe at exactly 8 back faces and one at 9 (either side of 0.25 x 32), an all-miss, an
    all-back and an all-far probe, one whose front faces come nearer from ray to ray (no ray is ever the farthest: the `else if`), and
    seeded offsets and states.  Each pass alone from the supplied data, then both in the update's
    order, under the reference's two minimum distances and a second threshold."""
    vol = PS.seeded_volume()
    d = PS.seeded_distances(vol)
    p = Placement(dev, vol)
    try:
        for k in (DP.consts(), DP.consts(min_frontface_distance=0.1), DP.consts(fixed_ray_backface_threshold=0.3)):
            moved, branches = DP.relocate(dp, k, vol, d)
            switched, reasons = DP.classify(dp, k, vol, d)
            p.upload_data(vol.data)
            same(_bits(p.run_place(k, [RELOCATION], d)), _bits(moved), "relocation alone")
            p.upload_data(vol.data)
            same(_bits(p.run_place(k, [CLASSIFICATION], d)), _bits(switched), "classification alone")
            both = vol.copy()
            both.data = moved
            p.upload_data(vol.data)
            same(_bits(p.run_place(k, [RELOCATION, CLASSIFICATION], d)), _bits(DP.classify(dp, k, both, d)[0]), "relocation, then classification")
        assert reasons[PS.SEEDED_9_BACK] != DP.OFF_BACKFACES, "at a threshold of 0.3 nine back faces are not enough"
    finally:
        p.release()


# ---- 2. frames ----------------------------------------------------------------------------------------------------------------------------
WOKEN, SWITCHED_OFF = 22, 21                      # probe (2, 1, 1) in the open middle of the box; probe (1, 1, 1) inside one of its blocks


def _driver_volume():
    """The tight Cornell volume with probe 22, in the open, pre-marked inactive and probe 21, inside a block (30 of its 32 fixed rays
    meet back faces), active like the rest."""
    vol = PS.tight_volume()
    vol.data[1, 1, 2, 3] = 1.0
    return vol


def test_three_chained_updates_through_the_driver(dev, oracle, dp, cornell):
    """Cornell at 64 x 36 through FrameDriver(ddgi=volume, ddgi_update=dict(relocate=True, classify=True, ...)): after each of three
    record() / run() pairs the data, irradiance and distance textures, the 256-ray records and the fixed-ray distances equal the
    reference update of the state before.  Probe 22 starts switched off: the first update traces nothing for it (its records stay
    zero) but its fixed rays wake it, and the second update writes its 256 records.  Probe 21 starts active inside a block and is
    switched off by the first update, for good.  The 12 probes above the ceiling are switched off by the first update too, which
    also moves them down into the box: the second update wakes them (15 probes off, then 3)."""
    from toyrenderer_amd.frame import FrameDriver
    sc, gs, scene = cornell
    cam = sc["camera"]
    view = gltf_lite.view_of(cam, (64, 36))
    vol = _driver_volume()
    settings = dict(seed=13, relocate=True, classify=True, min_frontface_distance=CORNELL_MIN_FRONT)
    drv = FrameDriver(dev, gs, view, ddgi=vol, ddgi_update=settings, record_capacity=4096, culling_flags=7, lighting=True, dir_light=US.LIGHT,
                      camera_origin=tuple(float(x) for x in cam.position))
    try:
        state = vol.copy()
        rays = np.zeros((64, DU.RAYS, 4), F)
        for n in range(3):
            drv.record(); drv.run(); drv.results()
            k = drv.ddgi_update_consts
            assert k["probeMinFrontfaceDistance"][0] == F(0.1) and k["probeFixedRayBackfaceThreshold"][0] == F(0.25) and k["pad"][0] == 0
            rays, fixed = DP.update(dp, k, state, scene, rays_init=rays)          # state: one reference update further
            same(drv.download_ddgi_rays().view(np.uint32), rays.view(np.uint32), f"update {n}: ray records")
            same(drv.download_ddgi_fixed_rays().view(np.uint32), fixed.view(np.uint32), f"update {n}: fixed-ray distances")
            got = drv.download_ddgi()
            same(_bits(got.data), _bits(state.data), f"update {n}: probe data")
            same(got.irradiance, state.irradiance, f"update {n}: irradiance")
            same(_bits(got.distance), _bits(state.distance), f"update {n}: distance")
            w = got.data[..., 3].reshape(-1)
            assert w[WOKEN] == 0.0 and w[SWITCHED_OFF] == 1.0
            written = bool(np.any(drv.download_ddgi_rays()[WOKEN] != 0))
            assert written == (n >= 1), f"update {n}: the woken probe's records"
            assert np.count_nonzero(w == 1.0) == (15 if n == 0 else 3) and np.count_nonzero(np.any(_bits(got.data)[..., :3] != 0, axis=-1)) >= 12
    finally:
        drv.release()


def test_with_both_options_off_the_update_records_what_it_did(dev, oracle, cornell):
    """relocate=False, classify=False (the defaults): the recorded dispatches are the three of the update and its 96-byte block is
    what it was, the two new fields zero.  With both on the three placement passes follow the blends; with one on, the fixed-ray
    trace and that pass.  An option is refused on a volume whose flag is off."""
    from toyrenderer_amd.frame import FrameDriver
    sc, gs, scene = cornell
    view = gltf_lite.view_of(sc["camera"], (64, 36))
    common = dict(record_capacity=4096, culling_flags=7, lighting=True, dir_light=US.LIGHT)
    made = [FrameDriver(dev, gs, view, ddgi=_driver_volume(), **common),
            FrameDriver(dev, gs, view, ddgi=_driver_volume(), ddgi_update=dict(seed=4), **common),
            FrameDriver(dev, gs, view, ddgi=_driver_volume(), ddgi_update=dict(seed=4, relocate=False, classify=False, min_frontface_distance=0.1), **common),
            FrameDriver(dev, gs, view, ddgi=_driver_volume(), ddgi_update=dict(seed=4, relocate=True, classify=True), **common),
            FrameDriver(dev, gs, view, ddgi=_driver_volume(), ddgi_update=dict(seed=4, classify=True), **common),
            FrameDriver(dev, gs, view, ddgi=_driver_volume(), ddgi_update=dict(seed=4, relocate=True), **common)]
    try:
        plain, default, off, on, classify, relocate = ([shader for _, shader in recorded(d) if shader] for d in made)
        at = plain.index("deferredlighting_PS_Main")
        today = plain[:at] + ["raytracing_CS_RefitTLAS"] + UPDATE + plain[at:]
        assert default == today and off == today
        at += 4
        assert on == today[:at] + [FIXED, RELOCATION, CLASSIFICATION] + today[at:]
        assert classify == today[:at] + [FIXED, CLASSIFICATION] + today[at:] and relocate == today[:at] + [FIXED, RELOCATION] + today[at:]
        want = DU.consts(light=US.LIGHT, rotation=ddgi.random_rotation(np.random.default_rng([4, 0])))      # the block as it was: 12 zero bytes at its end
        for d in made[1:3]:
            assert d.ddgi_update_consts.tobytes() == want.tobytes() and d.ddgi_update_consts.tobytes()[84:] == bytes(12)
            assert d.ddgi_fixed_rays is None
            with pytest.raises(ValueError, match="download_ddgi_fixed_rays: probe placement is off"):
                d.download_ddgi_fixed_rays()
        assert made[3].ddgi_update_consts.tobytes()[84:92] == F(0.3).tobytes() + F(0.25).tobytes()
    finally:
        for d in made:
            d.release()
    flat = ddgi.Volume(PS.TIGHT[2], PS.TIGHT[1], PS.TIGHT[0], normal_bias=0.02, view_bias=0.1, relocation=False, classification=True)
    with pytest.raises(ValueError, match="ddgi_update: relocate=True needs ddgi.Volume\\(relocation=True\\)"):
        FrameDriver(dev, gs, view, ddgi=flat, ddgi_update=dict(relocate=True), **common)
    flat.relocation, flat.classification = True, False
    with pytest.raises(ValueError, match="ddgi_update: classify=True needs ddgi.Volume\\(classification=True\\)"):
        FrameDriver(dev, gs, view, ddgi=flat, ddgi_update=dict(classify=True), **common)


def test_two_updates_through_the_host_mirror(oracle, dp, sm):
    """The same through host.Renderer: trhost_set_ddgi_probe_placement is refused without a volume and for a pass whose flag the
    volume has off; with it two frames leave the data, irradiance and distance textures the reference leaves, under the block
    trhost_get_ddgi_update_consts shows; switched off again, the block's two fields are zero and the data stays."""
    from suite_support import host_renderer
    from toyrenderer_amd import host
    sc = SS.cornell()
    s = sc["loaded"]
    inst = sc["instances"].copy()
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    ref = dict(sc); ref["instances"] = inst
    scene = DU.Scene(sm, SR.Accel(ref))
    s.meshData = sc["meshData"]
    render = (64, 36)
    view = gltf_lite.view_of(sc["camera"], render)
    vol = _driver_volume()
    with host_renderer(s, gltf_lite.apply_materials(s), (s.vertices, s.meshletVertexIds, s.meshletTriangles), sc["materials"], render=render, max_groups=4096) as r:
        r.set_deferred_lighting(True)
        r.set_directional_light(*US.LIGHT)
        r.set_culling(7)
        r.set_node_transforms(s.nodes)
        r.set_camera(view)
        with pytest.raises(host.HostError, match="trhost_set_ddgi_probe_placement: no DDGI volume.*ProbeRelocationCS_DDGIProbeRelocationCS"):
            r.set_ddgi_probe_placement(True, True)
        flat = vol.copy()
        flat.relocation = False
        r.upload_ddgi_volume(flat)
        with pytest.raises(host.HostError, match="relocation \\(bit 0\\) off.*ProbeRelocationCS_DDGIProbeRelocationCS"):
            r.set_ddgi_probe_placement(True, False)
        r.upload_ddgi_volume(vol)
        with pytest.raises(host.HostError, match="fixed_ray_backface_threshold in \\[0, 1\\]"):
            r.set_ddgi_probe_placement(True, True, 0.1, 1.5)
        r.load_raytracing(sc["indices"], sc["cached"].meshSpecific)
        r.set_ddgi(True)
        r.set_ddgi_update(True, seed=6)
        r.set_ddgi_probe_placement(True, True, CORNELL_MIN_FRONT, 0.25)
        state = vol.copy()
        rays = np.zeros((64, DU.RAYS, 4), F)
        for n in range(2):
            r.frame(); r.results()
            k = r.ddgi_update_consts()
            assert k["probeMinFrontfaceDistance"][0] == F(0.1) and k["probeFixedRayBackfaceThreshold"][0] == F(0.25) and k["pad"][0] == 0
            rays, _ = DP.update(dp, k, state, scene, rays_init=rays)
            got = r.download_ddgi_volume(vol)
            same(_bits(got.data), _bits(state.data), f"host update {n}: probe data")
            same(got.irradiance, state.irradiance, f"host update {n}: irradiance")
            same(_bits(got.distance), _bits(state.distance), f"host update {n}: distance")
        w = got.data[..., 3].reshape(-1)
        assert w[WOKEN] == 0.0 and w[SWITCHED_OFF] == 1.0
        r.set_ddgi_probe_placement(False, False)
        r.frame(); r.results()
        assert r.ddgi_update_consts().tobytes()[84:] == bytes(12)
        same(_bits(r.download_ddgi_volume(vol).data), _bits(state.data), "host: placement off, the data stays")


# ---- 3. misuse -----------------------------------------------------------------------------------------------------------------------------
def test_misuse_of_the_passes_is_refused(dev, cornell):
    """A short constant block, a distance buffer of the wrong size, data without the UAV bit, a non-array texture or one of the wrong
    format or size, wrong group counts, and relocation or classification on a volume whose flag is off: each is refused with the
    pass's name."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, SRV, TEX_SRV, TEX_UAV, UAV
    sc, gs, scene = cornell
    vol = PS.cornell_volume("3x2x4", True)
    p, ro = Placement(dev, vol, gs), Placement(dev, vol, gs, data_uav=False)
    made = []
    cl = p.cl
    k = DP.consts()
    cl.open()
    try:
        cb = cl.constant_buffer(p.block(k), "DDGIUpdateConsts")
        short = cl.constant_buffer(p.block(k)[:96], "short")
        small = dev.create_buffer(p.n * DP.FIXED * 4 - 4, "small distances", stride=4); made.append(small)
        records = dev.create_buffer(p.n * DU.RAYS * 16, "the 256-ray records", stride=16); made.append(records)
        plain = dev.create_texture(3, 4, 1, rhi.FORMAT_RGBA16_FLOAT, "plain"); made.append(plain)
        other = dev.create_texture_array(4, 4, 2, rhi.FORMAT_RGBA16_FLOAT, "other size", uav=True); made.append(other)
        rg = dev.create_texture_array(3, 4, 2, rhi.FORMAT_RG16_FLOAT, "wrong format", uav=True); made.append(rg)

        def swap(bindings, kind, slot, new):
            return [b for b in bindings if not (b.type == kind and b.slot == slot)] + ([new] if new is not None else [])

        def block_with(**fields):
            d = vol.desc().copy()
            for f, x in fields.items():
                d[f] = x
            return cl.constant_buffer(np.frombuffer(k.tobytes() + d.tobytes(), np.uint8), "bad")

        for name, bindings, groups in ((FIXED, p.fixed_bindings, p.fixed_groups()), (RELOCATION, p.place_bindings, p.place_groups()), (CLASSIFICATION, p.place_bindings, p.place_groups())):
            cases = [("160 bytes", swap(bindings(cb), rhi.BIND_CONSTANT_BUFFER, 0, CB(0, short)), groups),
                     ("160 bytes", swap(bindings(cb), rhi.BIND_CONSTANT_BUFFER, 0, None), groups),
                     ("direct dispatch of", bindings(cb), (groups[0] + 1, 1, 1)),
                     ("direct dispatch of", bindings(cb), (groups[0], 2, 1)),
                     ("not in 1..1024", bindings(block_with(probeCounts=(3, 0, 4))), groups),
                     ("the fixed-ray distances at u0 hold", swap(bindings(cb), rhi.BIND_STRUCTURED_UAV, 0, UAV(0, small)), groups),
                     ("the fixed-ray distances at u0 hold", swap(bindings(cb), rhi.BIND_STRUCTURED_UAV, 0, UAV(0, records)), groups),
                     ("u0 = the fixed-ray distances", swap(bindings(cb), rhi.BIND_STRUCTURED_UAV, 0, None), groups)]
            if name == FIXED:
                cases += [("t0 = the 64-byte DDGIVolumeDesc", swap(bindings(cb), rhi.BIND_STRUCTURED_SRV, 0, None), groups),
                          ("t12 = the BLAS nodes", swap(bindings(cb), rhi.BIND_STRUCTURED_SRV, 12, None), groups),
                          ("t1 = the RGBA16_FLOAT", swap(bindings(cb), rhi.BIND_TEXTURE_SRV, 1, None), groups),
                          ("not an array", swap(bindings(cb), rhi.BIND_TEXTURE_SRV, 1, TEX_SRV(1, plain)), groups),
                          ("is 4x4 with 2 slices", swap(bindings(cb), rhi.BIND_TEXTURE_SRV, 1, TEX_SRV(1, other)), groups),
                          ("array texture", swap(bindings(cb), rhi.BIND_TEXTURE_SRV, 1, TEX_SRV(1, rg)), groups),
                          ("declares no array texture there", bindings(cb) + [TEX_SRV(2, p.irr)], groups)]
            else:
                flag, word = (I.kDDGIFlag_Classification, "relocation \\(bit 0\\) off") if name == RELOCATION else (I.kDDGIFlag_Relocation, "classification \\(bit 1\\) off")
                cases += [("u3 = the RGBA16_FLOAT", swap(bindings(cb), rhi.BIND_TEXTURE_UAV, 3, None), groups),
                          ("without the UAV bit", swap(bindings(cb), rhi.BIND_TEXTURE_UAV, 3, TEX_UAV(3, ro.data, 0)), groups),
                          ("not an array", swap(bindings(cb), rhi.BIND_TEXTURE_UAV, 3, TEX_UAV(3, plain, 0)), groups),
                          ("is 4x4 with 2 slices", swap(bindings(cb), rhi.BIND_TEXTURE_UAV, 3, TEX_UAV(3, other, 0)), groups),
                          ("array texture", swap(bindings(cb), rhi.BIND_TEXTURE_UAV, 3, TEX_UAV(3, rg, 0)), groups),
                          ("declares no array texture there", swap(bindings(cb), rhi.BIND_TEXTURE_UAV, 3, TEX_UAV(2, p.data, 0)), groups),
                          (word, bindings(block_with(flags=flag)), groups), (word, bindings(block_with(flags=0)), groups)]
            for match, b, g in cases:
                with pytest.raises(rhi.TrhipError, match=match) as e:
                    cl.dispatch(name, b, g)
                assert name in str(e.value), (match, str(e.value))
    finally:
        cl.close()
        for r in made:
            r.release()
        p.release(); ro.release()


# ---- 4. what fails without this feature -------------------------------------------------------------------------------------------------
def test_the_feature_is_there():
    from toyrenderer_amd import host, rhi
    from toyrenderer_amd.frame import FrameDriver
    names = rhi.shader_names()
    for n in (FIXED, RELOCATION, CLASSIFICATION):
        assert n in names
    for setting in ("relocate", "classify", "min_frontface_distance", "fixed_ray_backface_threshold"):
        assert setting in ddgi.UPDATE_DEFAULTS
    assert ddgi.UPDATE_DEFAULTS["relocate"] is False and ddgi.UPDATE_DEFAULTS["classify"] is False
    assert "data_uav" in inspect.signature(ddgi.Volume.upload).parameters and hasattr(FrameDriver, "download_ddgi_fixed_rays")
    assert I.kDDGIFixedRays == 32 and "probeMinFrontfaceDistance" in I.DDGIUpdateConsts.fields
    assert "trhost_set_ddgi_probe_placement" in host.HOST_SYMBOLS and hasattr(host.load(), "trhost_set_ddgi_probe_placement")
    assert hasattr(host.Renderer, "set_ddgi_probe_placement")
