"""The two probe traces ("giprobetrace_CS_ProbeTrace", "giprobetrace_CS_ProbeTraceFixedRays"; csrc/k_giprobetrace.hip,
csrc/k_giprobeplacement.hip) and with them rw::closestHit (csrc/ray_walk.hip.h) on the GPU, on scenes that can tell a wrong walk apart:
the cases of tests/ddgi_update_scenes.py TRACE_CASES, every word against tests/ddgi_update_ref.c and tests/ddgi_placement_ref.c.
tests/test_gpu_ddgi_update.py and tests/test_gpu_ddgi_placement.py run the same kernels on the Cornell fixture (3 instances, unit
scales, no mirror, face-constant normals, no emissive material, every index valid) and on one identity cube; here the instances are
rotated, scaled non-uniformly and mirrored, the vertex normals differ across a triangle, candidates tie in t, materials are emissive,
NaN, infinite or past the buffer, instances are in no list, the TLAS has 1 to 257 leaves and is refitted to moved instances, TMax
cuts hits off and the shadow ray is axis-parallel.  tests/test_ddgi_update_ref.py holds the preconditions (what the reference's rays
meet in each case, with the measured counts); profiles/ddgi/trace_mutations.txt the negative controls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_placement_ref as DP  # noqa: E402
import ddgi_update_ref as DU  # noqa: E402
import ddgi_update_scenes as US  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from ddgi_passes import CLASSIFICATION, RAY_SENTINEL, RELOCATION, Placement, Update, city_trace_scene, city_volume, refitted_structure, trace_case  # noqa: E402
from suite_support import bare_gpu_scene, dev, gpu_scene, ref_library, same, sm, unflagged_leaves  # noqa: E402, F401
from toyrenderer_amd import gltf_lite  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
dp = ref_library(DP)                              # holds tests/ddgi_update_ref.c too
INACTIVE = (4, 13)                                # the probes "attributes" switches off


def _bits(data):
    return np.ascontiguousarray(data).view(np.uint16)


def _scene_on_the_gpu(dev, c):
    """The case's scene with the structure built from its rest transforms; a moved case's instances are uploaded behind that, so
    the refit the passes record is what moves the boxes."""
    gs = bare_gpu_scene(dev, c.sc)
    if c.inst is not c.sc["instances"]:
        gs.instances.upload(c.inst)
    return gs


def _refit_equals_the_reference(sm, c, gs):
    nodes, records = refitted_structure(gs)
    want_nodes, want_records = SR.refit(sm, c.acc, c.inst)
    assert nodes.tobytes() == want_nodes.tobytes(), f"{c.name}: TLAS nodes after the refit"
    assert records.tobytes() == want_records.tobytes(), f"{c.name}: TLAS instances after the refit"


# ---- 1. the probe trace ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(US.TRACE_CASES))
def test_probe_trace_matches_the_reference(dev, sm, dp, name):
    """The refit, then the trace, in one command list, over ray records pre-filled with a sentinel: every word of the records equals
    DU.trace(..., DU.WALK), and the TLAS nodes and instance records read back equal SR.refit byte for byte.  "attributes" also
    switches two probes of its seeded volume off: their records keep the sentinel and every other probe's are written (the query
    of the recursive term skips a switched-off probe, so their colours differ from the all-active reference's)."""
    c = trace_case(sm, dp, name)
    vol, want = c.volume(), c.rays
    if name == "attributes":
        cx, cy, cz = vol.counts
        for p in INACTIVE:
            vol.data[p // (cx * cz), (p // cx) % cz, p % cx, 3] = 1.0
        want, kinds = DU.trace(dp, c.k, vol, c.scene, DU.WALK, c.init)
        active = np.setdiff1d(np.arange(len(want)), INACTIVE)
        assert np.all(want[list(INACTIVE)] == RAY_SENTINEL) and np.array_equal(kinds[active], c.kinds[active]) and np.all(want[active, :, 3] != RAY_SENTINEL)
    gs = _scene_on_the_gpu(dev, c)
    u = Update(dev, vol, gs, uav=False)
    try:
        got = u.run_trace(c.k)
        _refit_equals_the_reference(sm, c, gs)
        same(got.view(np.uint32), want.view(np.uint32), f"{name}: ray records")
    finally:
        u.release(); gs.release()


# ---- 2. the fixed-ray trace, relocation and classification on its distances -----------------------------------------------------------------
FIXED_VOLUMES = {"33 probes": US.fixed_ray_volume, "1 probe": lambda: US.trace_volume((1, 1, 1), (0.0, 2.0, -7.5), (0.0, 2.0, -7.5), seeded=False)}


@pytest.mark.parametrize("volume", list(FIXED_VOLUMES))
@pytest.mark.parametrize("name", US.FIXED_RAY_CASES)
def test_fixed_ray_trace_matches_the_reference(dev, sm, dp, name, volume):
    """The fixed-ray trace over 3 x 1 x 11 = 33 probes (the ragged last wave holds one probe) and over one probe: every distance
    equals DP.trace_fixed; then relocation on those distances and classification on the relocated data equal DP.relocate and
    DP.classify, as tests/test_gpu_ddgi_placement.py has it on the Cornell fixture.  A rotation is in the block: the fixed rays
    must not take it.  MEASURED on the reference (taken moves / probes switched off; the volumes are as specified, not tuned):
    33 probes: tlas 65 3 / 12, tlas 257 6 / 6, moved 3 / 20, attributes 3 / 12, and 0 / 33 over "shared planes", whose cubes lie
    units away from the nearest probe: all but 14 of its 1056 rays miss, no probe moves (branch C with a zero offset) and every
    probe is switched off because nothing is within a cell.  The 1 probe volume takes NO move in any case (branch B refused over
    tlas 65 and attributes, branch C with a zero offset otherwise) and switches its probe off only over moved and shared planes
    (0 / 1); over tlas 65, tlas 257 and attributes it gives neither (0 / 0): there it checks the trace and the passes' unchanged
    data alone."""
    c = trace_case(sm, dp, name)
    vol = FIXED_VOLUMES[volume]()
    k = DP.consts(rotation=US.rotation(3))
    gs = _scene_on_the_gpu(dev, c)
    p = Placement(dev, vol, gs)
    try:
        got = p.run_fixed(k)
        _refit_equals_the_reference(sm, c, gs)
        want = DP.trace_fixed(dp, k, vol, c.scene)
        same(got.view(np.uint32), want.view(np.uint32), f"{name}, {volume}: fixed-ray distances")
        moved, branches = DP.relocate(dp, k, vol, want)
        same(_bits(p.run_place(k, [RELOCATION])), _bits(moved), f"{name}, {volume}: data after relocation")
        vol.data = moved
        switched, reasons = DP.classify(dp, k, vol, want)
        same(_bits(p.run_place(k, [CLASSIFICATION])), _bits(switched), f"{name}, {volume}: data after classification")
        taken = int(np.count_nonzero(np.isin(branches, (DP.A_TAKEN, DP.B_TAKEN, DP.C_TAKEN))))
        print(f"{name}, {volume}: {taken} moves taken, {int(np.count_nonzero(reasons != DP.ACTIVE))} probes switched off")
    finally:
        p.release(); gs.release()


@pytest.mark.parametrize("which", ["probe trace", "fixed rays"])
def test_a_leaf_whose_instance_has_no_flags_is_skipped(dev, sm, dp, which):
    """suite_support.unflagged_leaves: 7 instances of "attributes" keep their leaves, boxes and object-from-world rows and lose their
    flags (the builder gives such an instance no leaf, so in "attributes" itself the walk's `flags == 0` rule decides nothing).  The
    arrays are uploaded over the ones set_raytracing() built; the refit in front of the trace leaves those records alone (asserted:
    the structure read back equals the reference's, byte for byte).  Each trace skips them: the ray records equal the reference,
    which equals the "attributes" records, and the fixed-ray distances over the 33-probe volume equal DP.trace_fixed.  MEASURED on
    the reference: hit, those leaves would change 15 of the 4608 records and 4 of the 1056 distances."""
    c = trace_case(sm, dp, "attributes")
    sc, acc, off = unflagged_leaves(sm)
    scene = DU.Scene(sm, acc)
    gs = bare_gpu_scene(dev, sc)
    gs.rt["tlas_nodes"].upload(acc.tlas["nodes"])
    gs.rt["tlas_instances"].upload(acc.tlas["records"])
    vol = c.volume() if which == "probe trace" else US.fixed_ray_volume()
    u = Update(dev, vol, gs, uav=False) if which == "probe trace" else Placement(dev, vol, gs)
    try:
        if which == "probe trace":
            got, want = u.run_trace(c.k), c.rays
        else:
            k = DP.consts(rotation=US.rotation(3))
            got, want = u.run_fixed(k), DP.trace_fixed(dp, k, vol, scene)
        nodes, records = refitted_structure(gs)
        assert nodes.tobytes() == scene.nodes.tobytes() and records.tobytes() == scene.records.tobytes(), "the structure after the refit"
        assert np.all(records["flags"][off] == 0)
        same(got.view(np.uint32), want.view(np.uint32), f"unflagged leaves: {which}")
    finally:
        u.release(); gs.release()


# ---- 3. one frame-level case ----------------------------------------------------------------------------------------------------------------
def test_city_frames_with_animation(dev, oracle, sm, dp, tmp_path):
    """The generated city (137 instances) at 48 x 27 through FrameDriver(lighting=True, ddgi=volume, ddgi_update=...), a cleared
    3 x 2 x 3 volume over the city's bounds: two updates, with three instances' world matrices changed in between (one pushed
    aside, one turned and carried 20 units up out of its rest box, one scaled non-uniformly).  After each, the ray records
    equal the reference trace (DU.WALK; tests/test_ddgi_update_ref.py checks it against brute force on the first frame) over the
    frame's own instances and download_ddgi() equals DU.update of the state before."""
    from toyrenderer_amd.frame import FrameDriver
    s, c, v, mats, sc, bounds = city_trace_scene(tmp_path, oracle)
    gs = gpu_scene(dev, s, sc["instances"], v, mats)
    gs.set_raytracing(c.indices, c.meshSpecific)
    acc = SR.Accel(sc)
    vol = city_volume(bounds)
    view = gltf_lite.view_of(s.cameras[0], (48, 27))
    drv = FrameDriver(dev, gs, view, record_capacity=4096, culling_flags=7, lighting=True, dir_light=(SS.unit((0.2, 0.35, -0.9)), 2.5), ddgi=vol,
                      ddgi_update=dict(seed=21, hysteresis=0.7))
    try:
        state = vol.copy()
        instances = sc["instances"].copy()
        seen = []
        for f in range(2):
            if f == 1:
                instances["m_PrevWorldMatrix"] = instances["m_WorldMatrix"]
                rest = instances["m_WorldMatrix"].astype(np.float64)
                instances["m_WorldMatrix"][3] = (rest[3] @ SS.world_matrix(position=(2.5, 0.0, 0.0))).astype(F)
                instances["m_WorldMatrix"][40] = (rest[40] @ SS.world_matrix(axis=(0.2, 1.0, 0.1), angle=0.7, position=(-1.0, 20.0, 3.0))).astype(F)
                instances["m_WorldMatrix"][90] = (SS.world_matrix(scale=(1.5, 0.5, 1.0)).astype(np.float64) @ rest[90]).astype(F)
                gs.instances.upload(instances)
            drv.record(); drv.run(); drv.results()
            k = drv.ddgi_update_consts
            assert drv.ddgi_updates == f + 1
            want_rays = DU.update(dp, k, state, DU.Scene(sm, acc, instances))       # state: one reference update further
            same(drv.download_ddgi_rays().view(np.uint32), want_rays.view(np.uint32), f"city update {f}: ray records")
            got = drv.download_ddgi()
            same(got.irradiance, state.irradiance, f"city update {f}: irradiance")
            same(_bits(got.distance), _bits(state.distance), f"city update {f}: distance")
            same(_bits(got.data), _bits(state.data), f"city update {f}: probe data")
            seen.append(want_rays)
        assert np.count_nonzero(seen[0][..., 3] < 1e27) > 200 and np.count_nonzero(seen[0][..., 3] < 0) > 10, "the rays meet the city, back faces among them"
    finally:
        drv.release(); gs.release()
