"""tests/ddgi_update_ref.c on the CPU: the definition of the DDGI probe update ("giprobetrace_CS_ProbeTrace" and the two
"ProbeBlendingCS_DDGIProbeBlendingCS" passes).  The closest-hit walk of the product's node arrays against brute force over every
triangle, the face rule, the encodings the lighting pass's query assumes, the hysteresis, which probes are left alone, the
borders, a float64 restatement of the two blends, and what the cases of tests/ddgi_blend_scenes.py reach, counted from the
reference's own rule words.  tests/test_gpu_ddgi_update.py, tests/test_gpu_ddgi_trace_scenes.py and
tests/test_gpu_ddgi_blend_rules.py hold the kernels to the same reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_blend_scenes as BS  # noqa: E402
import ddgi_placement_ref as DP  # noqa: E402
import ddgi_update_ref as DU  # noqa: E402
import ddgi_update_scenes as US  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from ddgi_passes import city_trace_scene, city_volume, trace_case  # noqa: E402
from ref_build import layout_probe  # noqa: E402
from suite_support import ref_library, same, sm, unflagged_leaves  # noqa: E402, F401
from toyrenderer_amd import ddgi  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

F = np.float32
du = ref_library(DU)
dp = ref_library(DP)                              # holds tests/ddgi_update_ref.c too: the trace cases share one handle with the GPU file
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (-0.0, 0, -1)], F)

# Float64 agreement (test_blends_agree_with_float64): the largest differences MEASURED with US.blend_volume(seed 3) and
# US.blend_rays(seed 4) under rotation seed 2; the test asserts them plus one code for the float32 summation order
# (profiles/ddgi/README.md records them).
MEASURED_IRRADIANCE_CODES = 1                  # 7 of 1080 channels differ, each by one code
MEASURED_DISTANCE_STEPS = 0.501                # of a binary16 step: the store's own rounding and no more
# test_blend_cases_agree_with_float64 leaves out texels whose compared quantity is this close to a threshold: the float32 chain's
# reach (256 products and sums at 2^-24 each, the soft pow at 2^-22 relative, on values below 1)
FLOAT32_REACH = 2e-5


class _Words:
    """Lets BS.irradiance_tile address a plain array of the irradiance texture's shape."""

    def __init__(self, irradiance, counts):
        self.irradiance, self.counts = irradiance, counts


@pytest.fixture(scope="module")
def scenes(sm):
    made = {}

    def get(name):
        if name not in made:
            made[name] = DU.Scene(sm, SR.Accel(US.SCENES[name]()))
        return made[name]
    return get


# ---- 1. the closest hit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(US.SCENES))
def test_closest_hit_walk_equals_brute_force(du, scenes, name):
    """Every ray of every origin: the walk's (instance, triangle, t bits, barycentric bits, face bit) equal brute force over every
    triangle of every instance.  The walk does not prune, so this holds as long as the box test never rejects a box whose
    triangle the triangle test accepts.  In "shared planes" equal t occurs and the tie rule decides."""
    scene = scenes(name)
    dirs = np.concatenate([DU.ray_directions(du, DU.consts(rotation=US.rotation(1))), DU.ray_directions(du, DU.consts()), AXES])
    hits = ties = 0
    for o in US.ORIGINS[name]:
        origins = np.broadcast_to(np.asarray(o, F), dirs.shape)
        brute, t = DU.closest(du, scene, origins, dirs, DU.BRUTE)
        walk, _ = DU.closest(du, scene, origins, dirs, DU.WALK)
        same(walk.view(np.uint32), brute.view(np.uint32), f"{name} from {o}")
        hit = brute["inst"] != DU.MISS
        assert np.all(brute["t"][hit] > 0)
        hits += int(hit.sum()); ties += t
        # a shorter TMax only removes hits
        near, _ = DU.closest(du, scene, origins, dirs, DU.WALK, tmax=1.0)
        want = np.where(hit & (brute["t"] < 1.0), brute["inst"], DU.MISS)
        assert np.array_equal(near["inst"], want)
    assert hits > 20
    if name == "shared planes":
        assert ties >= 1
        both = DU.closest(du, scene, [(3.0, 0.25, 0.0)], [(-1.0, 0.0, 0.0)], DU.WALK)[0]
        assert both["inst"][0] == 0 and both["t"][0] == 2.0              # instances 0 and 1 both at t = 2: the lower index wins


def test_instances_without_flags_are_skipped_and_alpha_instances_are_hit(du, sm):
    """flags == 0 (an instance in neither list) is skipped; a ForceNonOpaque instance commits like an opaque one, whatever its
    material's alpha says (RAY_FLAG_FORCE_OPAQUE)."""
    sc = US.shared_planes()
    sc["materials"]["m_ConstAlbedo"][:, 3] = 0.0                         # every alpha test would fail
    scene = DU.Scene(sm, SR.Accel(sc))
    hit = DU.closest(du, scene, [(8.0, 0.0, 0.0)], [(-1.0, 0.0, 0.0)], DU.WALK)[0]
    assert hit["inst"][0] == 2 and hit["t"][0] == 3.0
    sc["alphaMaskIds"] = np.zeros(0, np.uint32)                          # instance 2 in no list: flags 0
    scene = DU.Scene(sm, SR.Accel(sc))
    for mode in (DU.BRUTE, DU.WALK):
        hit = DU.closest(du, scene, [(8.0, 0.0, 0.0)], [(-1.0, 0.0, 0.0)], mode)[0]
        assert hit["inst"][0] == 0 and hit["t"][0] == 7.0


# ---- 2. the face rule --------------------------------------------------------------------------------------------------------------
def _single_probe(origin, spacing=(1.0, 1.0, 1.0)):
    return ddgi.Volume(origin, spacing, (1, 1, 1), normal_bias=0.02, view_bias=0.1, relocation=False, classification=False).reset()


def test_face_rule(du, scenes):
    """Front is decided in object space from the sign of the watertight test's det.  A probe inside a closed cube whose triangles
    face outward gets 256 back faces; a probe inside the Cornell box, whose walls face inward, at least 200 front faces."""
    p, idx = US.cube()
    tri = p[idx.reshape(-1, 3)]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert np.all((normal * tri.mean(1)).sum(-1) > 0), "the cube's triangles face outward"
    for rot in (None, US.rotation(3)):
        k = DU.consts(rotation=rot)
        rays, kinds = DU.trace(du, k, _single_probe((0.1, -0.2, 0.3)), scenes("closed cube"))
        assert np.all(kinds == DU.KIND_BACK) and np.all(rays[..., 3] < 0) and np.all(rays[..., :3] == 0)
        hits, _ = DU.closest(du, scenes("closed cube"), np.broadcast_to(F((0.1, -0.2, 0.3)), (DU.RAYS, 3)), DU.ray_directions(du, k), DU.WALK)
        same(rays[0, :, 3].view(np.uint32), (F(-0.2) * hits["t"]).view(np.uint32), "back face: -0.2f * t")
        rays, kinds = DU.trace(du, k, _single_probe((0.0, 1.0, 0.0)), scenes("cornell"))
        front = np.count_nonzero((kinds == DU.KIND_LIT) | (kinds == DU.KIND_SHADOWED))
        assert front >= 200, front
    # a mirrored instance does not flip the rule: instance 2 of "shared planes" is the cube mirrored in y, still back from inside
    rays, kinds = DU.trace(du, DU.consts(max_ray_distance=0.9), _single_probe((4.0, 0.0, 0.0), (0.5, 0.5, 0.5)), scenes("shared planes"))
    assert np.count_nonzero(kinds == DU.KIND_MISS) > 0 and np.all((kinds == DU.KIND_BACK) | (kinds == DU.KIND_MISS))
    rays, kinds = DU.trace(du, DU.consts(), _single_probe((4.0, 0.0, 0.0)), scenes("shared planes"))
    assert np.all(kinds == DU.KIND_BACK)


def test_trace_walk_equals_brute_force_and_takes_every_branch(du, scenes):
    """The whole trace over the Cornell fixture, records and all: the walk equals brute force, with cleared and with seeded volume
    contents; misses, back faces, lit and shadowed front faces all occur; an inactive probe's records keep what they held."""
    scene = scenes("cornell")
    k = DU.consts(light=US.LIGHT, rotation=US.rotation(7))
    seen = set()
    for name in US.CORNELL_VOLUMES:
        for seeded in (False, True):
            vol = US.cornell_volume(name, seeded)
            init = np.full((int(np.prod(vol.counts)), DU.RAYS, 4), 7.5, F)
            walk, kinds = DU.trace(du, k, vol, scene, DU.WALK, init)
            brute, _ = DU.trace(du, k, vol, scene, DU.BRUTE, init)
            same(walk.view(np.uint32), brute.view(np.uint32), f"{name} seeded={seeded}")
            _, inactive = DU.probe_positions(du, vol)
            assert np.all(walk[inactive] == 7.5) and np.all(kinds[inactive] == 0xFF) and np.all(kinds[~inactive] != 0xFF)
            assert inactive.sum() == (2 if seeded and name == "3x2x4" else 0)
            seen |= set(int(x) for x in np.unique(kinds[~inactive]))
            front = (kinds == DU.KIND_LIT) | (kinds == DU.KIND_SHADOWED)
            assert np.all(walk[front][:, :3] >= 0) and np.all(walk[front][:, :3] <= 1) and np.all(walk[front][:, 3] > 0)
            if seeded:
                cleared, kinds0 = DU.trace(du, k, vol.copy().reset(), scene, DU.WALK, init)     # the same probes over cleared textures
                assert np.array_equal(kinds0, kinds) and np.count_nonzero(walk[front][:, :3] != cleared[front][:, :3]) > 100, "the recursive term is there"
    assert seen == {DU.KIND_MISS, DU.KIND_BACK, DU.KIND_LIT, DU.KIND_SHADOWED}


# ---- 2b. preconditions of the GPU trace cases (US.TRACE_CASES), on the reference alone --------------------------------------------
# What tests/test_gpu_ddgi_trace_scenes.py can tell apart depends on what the reference's rays meet.  These are conditions on the
# inputs, not measurements of the kernels: a scene that misses one is changed, not the bound.  KINDS: KIND_MISS, KIND_BACK, KIND_LIT,
# KIND_SHADOWED.
BIG = ["tlas 64", "tlas 65", "tlas 257"]
ROTATED, SCALED, MIRRORED, ALPHA = (lambda i: i % 3 != 0), (lambda i: i % 4 == 1), (lambda i: i % 5 == 2), (lambda i: i % 10 == 7)      # SS.scattered's rules


def _kinds(kinds):
    return [int(np.count_nonzero(kinds == x)) for x in (DU.KIND_MISS, DU.KIND_BACK, DU.KIND_LIT, DU.KIND_SHADOWED)]


def _front(kinds):
    return (kinds == DU.KIND_LIT) | (kinds == DU.KIND_SHADOWED)


def _on(hits, rule):
    """bool like hits: the ray's hit is on an instance for which rule(index) holds."""
    inst = hits["inst"]
    table = np.array([bool(rule(i)) for i in range(int(inst[inst != DU.MISS].max()) + 1 if np.any(inst != DU.MISS) else 1)])
    return (inst != DU.MISS) & table[np.where(inst != DU.MISS, inst, 0)]


@pytest.mark.parametrize("name", list(US.TRACE_CASES))
def test_trace_cases_walk_equals_brute_force(sm, dp, name):
    """Every case of US.TRACE_CASES: the records of the walk over the refitted node arrays equal brute force over every triangle,
    word for word, and so do the closest hits of the probes' own rays.  MEASURED: true in all 18 cases."""
    c = trace_case(sm, dp, name)
    brute, kinds = DU.trace(dp, c.k, c.volume(), c.scene, DU.BRUTE, c.init)
    same(c.rays.view(np.uint32), brute.view(np.uint32), f"{name}: records, walk against brute force")
    assert np.array_equal(kinds, c.kinds)
    same(c.hits(dp, DU.WALK).view(np.uint32), c.hits(dp, DU.BRUTE).view(np.uint32), f"{name}: hits, walk against brute force")
    print(f"{name}: kinds {_kinds(c.kinds)}")


@pytest.mark.parametrize("name", BIG)
def test_trace_cases_large_scattered_scenes_meet_every_kind_of_instance(sm, dp, name):
    """At least 50 records of each kind; at least 100 front-face hits each on rotated and on non-uniformly scaled instances, 50 on
    mirrored ones, 30 on alpha-list ones; at least 40 distinct instances hit.  MEASURED (miss / back / lit / shadowed; front hits
    on rotated / scaled / mirrored / alpha; distinct): tlas 64: 3568 / 379 / 483 / 178; 296 / 261 / 120 / 61; 60.
    tlas 65: 3552 / 279 / 639 / 138; 254 / 264 / 130 / 61; 62.  tlas 257: 2172 / 740 / 881 / 815; 661 / 504 / 298 / 96; 216."""
    c = trace_case(sm, dp, name)
    hits, front = c.hits(dp), _front(c.kinds)
    counts = [int(np.count_nonzero(front & _on(hits, rule))) for rule in (ROTATED, SCALED, MIRRORED, ALPHA)]
    distinct = len(np.unique(hits["inst"][hits["inst"] != DU.MISS]))
    print(f"{name}: kinds {_kinds(c.kinds)}, front hits on rotated / scaled / mirrored / alpha {counts}, {distinct} distinct instances")
    assert min(_kinds(c.kinds)) >= 50, _kinds(c.kinds)
    assert counts[0] >= 100 and counts[1] >= 100 and counts[2] >= 50 and counts[3] >= 30, counts
    assert distinct >= 40
    assert np.array_equal(front, (hits["inst"] != DU.MISS) & (hits["front"] == 1)) and np.array_equal(c.kinds == DU.KIND_MISS, hits["inst"] == DU.MISS)


@pytest.mark.parametrize("name", ["tlas 1", "tlas 2", "tlas 3"])
def test_trace_cases_small_scattered_scenes_are_hit(sm, dp, name):
    """At least one hit.  MEASURED: 13, 75, 73."""
    c = trace_case(sm, dp, name)
    n = int(np.count_nonzero(c.kinds != DU.KIND_MISS))
    print(f"{name}: {n} hits")
    assert n >= 1


def test_trace_case_moved_differs_from_the_rest_pose(sm, dp):
    """At least 300 records differ from the trace of the same scene at rest.  MEASURED: 699; 22 of the 65 instances moved, each out
    of the box its TLAS leaf was built with."""
    c, rest = trace_case(sm, dp, "moved"), trace_case(sm, dp, "tlas 65")
    n = int(np.count_nonzero(np.any(c.rays.view(np.uint32) != rest.rays.view(np.uint32), axis=-1)))
    moved = np.flatnonzero(np.any(c.inst["m_WorldMatrix"] != c.sc["instances"]["m_WorldMatrix"], axis=(1, 2)))
    print(f"moved: {n} records differ, {len(moved)} instances moved")
    assert n >= 300 and len(moved) == 22
    assert not np.array_equal(SR.refit(sm, c.acc, c.inst)[0]["lo"], SR.refit(sm, c.acc)[0]["lo"]), "the refit moved the boxes"


def test_trace_case_shared_planes_ties_and_the_tie_shows(sm, dp):
    """At least 100 rays meet instances 0 and 1 at the same t (found by tracing once more with instance 0 in no list: a ray whose
    hit is instance 0 at t and then instance 1 at the same t); on at least 50 of them the record changes when instance 1 wins
    (another triangle: other normals; the volume is seeded so that the recursive term shows them).  MEASURED: 292 ties, 102 of
    them with a record that changes, all front faces."""
    c = trace_case(sm, dp, "shared planes")
    sc = dict(c.sc)
    sc["opaqueIds"] = np.array([1], np.uint32)                           # instance 0 in no list: flags == 0
    other = DU.Scene(sm, SR.Accel(sc))
    first, second = c.hits(dp), c.hits(dp, scene=other)
    tie = (first["inst"] == 0) & (second["inst"] == 1) & (first["t"] == second["t"])
    alt, _ = DU.trace(dp, c.k, c.volume(), other, DU.WALK, c.init)
    shows = tie & np.any(alt.view(np.uint32) != c.rays.view(np.uint32), axis=-1)
    print(f"shared planes: {int(tie.sum())} ties, {int(shows.sum())} show, {int((shows & _front(c.kinds)).sum())} of them front faces")
    assert tie.sum() >= 100 and shows.sum() >= 50


def test_trace_case_attributes_reaches_every_attribute(sm, dp):
    """Front-face hits: at least 50 on instances whose material index is past the buffer, 100 on the emissive material and 100 on
    the one with a NaN albedo; at least 8 rays would end on an instance the case takes out of the lists were it listed, none does,
    and no record holds a NaN.  MEASURED: 115 / 267 / 326 front hits (and 16 on the material with an infinite emissive), 15 rays."""
    c = trace_case(sm, dp, "attributes")
    hits, front = c.hits(dp), _front(c.kinds)
    mat = c.sc["instances"]["m_MaterialDataIdx"]
    counts = [int(np.count_nonzero(front & _on(hits, rule))) for rule in (US.ATTR_PAST, lambda i: mat[i] == 1, lambda i: mat[i] == 0, lambda i: mat[i] == 4)]
    listed = DU.Scene(sm, SR.Accel(US.attributes(listed=True)))
    would = int(np.count_nonzero(_on(c.hits(dp, scene=listed), US.ATTR_UNLISTED)))
    print(f"attributes: front hits on past-the-buffer / emissive / NaN albedo / infinite emissive {counts}, {would} rays would end on an unlisted instance")
    assert sorted(set(int(m) for m in mat[[i for i in range(len(mat)) if US.ATTR_PAST(i)]])) == [5, 0xFFFFFFFF] and len(c.sc["materials"]) == 5
    assert counts[0] >= 50 and counts[1] >= 100 and counts[2] >= 100 and counts[3] >= 1, counts
    assert would >= 8
    assert np.count_nonzero(_on(hits, US.ATTR_UNLISTED)) == 0
    assert not np.isnan(c.rays).any()


def test_unflagged_leaves_are_skipped_and_would_be_hit(sm, dp):
    """The builder leaves an instance that is in neither list out of the tree, so in "attributes" no leaf names one and the walk's
    `flags == 0` rule decides nothing there.  suite_support.unflagged_leaves is the structure where it decides: 7 instances keep
    their leaves, boxes and matrices and lose their flags.  The walk over it equals brute force and equals the "attributes"
    records word for word (another tree, the same answer), and every one of the 7 has a leaf whose box the refit left alone.
    MEASURED: the 15 rays of the test above are the ones that would end on them."""
    c = trace_case(sm, dp, "attributes")
    sc, acc, off = unflagged_leaves(sm)
    scene = DU.Scene(sm, acc)
    assert len(off) == 7 and np.all(scene.records["flags"][off] == 0) and np.all(scene.records["leaf_node"][off] < len(scene.nodes))
    assert np.all(scene.nodes["leaf"][scene.records["leaf_node"][off]] == off) and np.all(np.any(scene.records["object_from_world"][off] != 0, axis=(1, 2)))
    assert scene.nodes.tobytes() == acc.tlas["nodes"].tobytes() and scene.records.tobytes() == acc.tlas["records"].tobytes(), "a second refit changes nothing"
    for mode in (DU.WALK, DU.BRUTE):
        rays, _ = DU.trace(dp, c.k, c.volume(), scene, mode, c.init)
        same(rays.view(np.uint32), c.rays.view(np.uint32), f"unflagged leaves, mode {mode}: the records of attributes")


@pytest.mark.parametrize("tmax", [2.0, 4.0])
def test_trace_cases_tmax_cuts_hits_off(sm, dp, tmax):
    """At least 100 rays that hit in the unbounded trace at t >= tmax are misses here.  MEASURED: 601 and 328."""
    c, free = trace_case(sm, dp, f"tmax {tmax:g}"), trace_case(sm, dp, "tlas 65")
    far = free.hits(dp)
    cut = (far["inst"] != DU.MISS) & (far["t"] >= F(tmax))
    print(f"tmax {tmax:g}: {int(cut.sum())} hits cut off")
    assert cut.sum() >= 100 and np.all(c.kinds[cut] == DU.KIND_MISS) and np.array_equal(c.kinds[~cut], free.kinds[~cut])


def test_trace_case_light_x_has_both_front_kinds(sm, dp):
    """An axis-parallel shadow ray (boxHit's branch without a reciprocal): at least 100 lit and 100 shadowed records.
    MEASURED: 395 and 382."""
    c = trace_case(sm, dp, "light x")
    print(f"light x: kinds {_kinds(c.kinds)}")
    assert _kinds(c.kinds)[2] >= 100 and _kinds(c.kinds)[3] >= 100
    assert tuple(c.k["m_DirectionalLightVector"][0]) == (1.0, 0.0, 0.0)


def test_fixed_ray_volume_over_tlas_65_meets_every_kind(sm, dp):
    """The 33-probe volume of the GPU file's fixed-ray cases over "tlas 65": at least 50 misses, 50 back faces and 50 front faces
    among its 1056 distances, and the walk equals brute force.  MEASURED: 645 / 116 / 295."""
    c = trace_case(sm, dp, "tlas 65")
    k, vol = DP.consts(rotation=US.rotation(3)), US.fixed_ray_volume()
    d = DP.trace_fixed(dp, k, vol, c.scene)
    same(d.view(np.uint32), DP.trace_fixed(dp, k, vol, c.scene, DU.BRUTE).view(np.uint32), "fixed rays: walk against brute force")
    counts = [int(np.count_nonzero(d == DP.MISS_DISTANCE)), int(np.count_nonzero(d < 0)), int(np.count_nonzero((d > 0) & (d != DP.MISS_DISTANCE)))]
    print(f"fixed rays over tlas 65: miss / back / front {counts}")
    assert d.shape == (33, DP.FIXED) and min(counts) >= 50 and sum(counts) == d.size


def test_city_trace_walk_equals_brute_force(sm, dp, oracle, tmp_path):
    """The first frame of the GPU file's city case (137 instances at rest, the cleared 3 x 2 x 3 volume over the city's bounds, all
    4608 rays): the walk the GPU is held to equals brute force.  The whole first frame is used, not a one-probe volume: brute force
    takes about 5 s.  MEASURED kinds: 4215 / 14 / 305 / 74."""
    s, c, v, mats, sc, bounds = city_trace_scene(tmp_path, oracle)
    scene, vol = DU.Scene(sm, SR.Accel(sc)), city_volume(bounds)
    k = DU.consts(light=(SS.unit((0.2, 0.35, -0.9)), 2.5), rotation=ddgi.random_rotation(np.random.default_rng([21, 0])), hysteresis=0.7)
    walk, kinds = DU.trace(dp, k, vol, scene, DU.WALK)
    brute, _ = DU.trace(dp, k, vol, scene, DU.BRUTE)
    print(f"city: kinds {_kinds(kinds)}")
    same(walk.view(np.uint32), brute.view(np.uint32), "city: records, walk against brute force")
    assert min(_kinds(kinds)) >= 5


# ---- 3. the encodings ------------------------------------------------------------------------------------------------------------------
def test_all_miss_probe_stores_what_the_query_assumes(du, scenes):
    """A probe all of whose rays miss, on a cleared volume: every interior irradiance texel is round(1023 * 0.5 ^ (1 / gamma)) +- 1
    code in all three channels (the blend stores half the weighted mean, gamma-encoded; the query squares pow(texel, gamma / 2) and
    multiplies by 2 pi), and the distance is min(1e27, 1.5 * |spacing|) / 2 with half its square's mean beside it."""
    vol = _single_probe((10.0, 0.0, 0.0), (0.8, 1.1, 0.9))
    k = DU.consts(max_ray_distance=2.0, rotation=US.rotation(5))
    rays, kinds = DU.trace(du, k, vol, scenes("closed cube"))
    assert np.all(kinds == DU.KIND_MISS)
    same(rays.view(np.uint32), np.broadcast_to(np.array([1.0, 1.0, 1.0, 1e27], F), rays.shape).view(np.uint32), "miss records")
    irr, dist = DU.blend(du, k, vol, rays)
    want = int(np.rint(1023.0 * 0.5 ** (1.0 / vol.gamma)))
    codes = DU.unpack10(irr)[0][DU.interior_mask(irr.shape[1:], 8)]
    assert np.all(np.abs(codes - want) <= 1), (codes.min(), codes.max(), want)
    assert np.all(irr >> 30 == 3)
    d = min(1e27, 1.5 * float(np.linalg.norm(np.asarray(vol.spacing, np.float64)))) / 2.0
    inner = dist[0][DU.interior_mask(dist.shape[1:3], 16)].astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(d)) - 10)                             # one binary16 step at d
    assert np.all(np.abs(inner[:, 0] - d) <= ulp), (inner[:, 0].min(), inner[:, 0].max(), d)
    d2 = 2.0 * d * d
    assert np.all(np.abs(inner[:, 1] - d2) <= 2.0 ** (np.floor(np.log2(d2)) - 10))


def test_texel_directions_invert_the_querys_octahedral_encode(du):
    """octDecode of an interior texel's centre, encoded again by the query's oct(), lands on that centre."""
    for n in (6, 14):
        d = DU.texel_directions(du, n)
        assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=-1), 1.0, atol=1e-6)
        uv = np.zeros((n, n, 2), F)
        flat = np.ascontiguousarray(d.reshape(-1, 3))
        out = np.zeros((n * n, 2), F)
        du.dg_oct_n(flat.ctypes.data, n * n, out.ctypes.data)
        centre = (2.0 * np.arange(n) + 1.0) / n - 1.0
        uv = out.reshape(n, n, 2).astype(np.float64)
        assert np.allclose(uv[..., 0], centre[None, :], atol=1e-6) and np.allclose(uv[..., 1], centre[:, None], atol=1e-6)


def test_ray_directions_are_unit_and_cover_the_sphere(du):
    for rot in (None, US.rotation(1)):
        d = DU.ray_directions(du, DU.consts(rotation=rot)).astype(np.float64)
        assert np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-6)
        assert np.all(np.abs(d.mean(0)) < 0.01)                           # spherical Fibonacci: balanced
        for axis in np.eye(3):
            assert np.count_nonzero(d @ axis > 0.5) in range(56, 73)      # a quarter of the sphere's area: 64 of 256
    r = US.rotation(1).astype(np.float64)
    assert np.allclose(DU.ray_directions(du, DU.consts(rotation=US.rotation(1))), DU.ray_directions(du, DU.consts()).astype(np.float64) @ r.T, atol=1e-6)


# ---- 4. the hysteresis -----------------------------------------------------------------------------------------------------------------
def test_darkening_reaches_black_in_a_bounded_number_of_updates(du):
    """An all-one texel under radiance 0.  With the 1/1024 rule every update lowers the stored code by at least one (the step is at
    least min(1/1024, |delta|) and 1023 / 1024 of a code rounds to one), so black is reached within 1023 updates; without the rule
    the step (1 - h) * delta falls below half a code and the texel stalls above black."""
    for h in (0.5, 0.97):
        k = DU.consts(hysteresis=h)
        for rule in (True, False):
            code, updates = np.array([1023, 1023, 1023]), 0
            while code.max() > 0 and updates < 3000:
                prev = (code.astype(F) / F(1023.0)).astype(F)
                out = DU.ease_radiance(du, k, np.zeros(3, F), prev, rule)
                new = np.array([int(du.du_unorm10(float(x))) for x in out])
                assert np.all(new <= code)
                if rule:
                    assert np.all(new < code)
                code, updates = new, updates + 1
            print(f"hysteresis {h} rule {rule}: {updates} updates, code {code.max()}")
            if rule:
                assert code.max() == 0 and updates <= 1023
            elif h == 0.97:
                assert code.max() > 0, "without the rule the texel stalls"


def test_ease_radiance_rules(du):
    k = DU.consts()
    res = np.array([0.3, 0.6, 0.9], F)
    same(DU.ease_radiance(du, k, res, np.zeros(3, F)), res, "a cleared texel takes the estimate whole")
    prev = np.array([0.5, 0.5, 0.5], F)
    near = prev + F(0.01)
    assert np.allclose(DU.ease_radiance(du, k, near, prev), prev + 0.5 * 0.01, atol=1e-6)                    # plain hysteresis
    far = prev + np.array([0.3, 0.0, 0.0], F)                                                                 # > both thresholds: h 0, a quarter
    assert np.allclose(DU.ease_radiance(du, k, far, prev), prev + np.array([0.075, 0, 0]), atol=1e-6)
    mid = prev + np.array([0.15, 0.0, 0.0], F)                                                                # > brightness only: h stays
    assert np.allclose(DU.ease_radiance(du, k, mid, prev), prev + np.array([0.5 * 0.25 * 0.15, 0, 0]), atol=1e-6)


# ---- 5. the blends ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blended(du):
    vol = US.blend_volume()
    rays = US.blend_rays(vol)
    k = DU.consts(rotation=US.rotation(2))
    irr, dist = DU.blend(du, k, vol, rays)
    return vol, rays, k, irr, dist


def _tile(a, probe, counts, n):
    cx, cy, cz = counts
    x, y, z = probe % cx, probe // (cx * cz), (probe // cx) % cz
    return a[y, z * n:(z + 1) * n, x * n:(x + 1) * n]


def test_inactive_and_back_facing_probes_are_left_alone(du, blended):
    vol, rays, k, irr, dist = blended
    assert np.count_nonzero(rays[US.BLEND_24_BACK, :, 3] < 0) == 24 and np.count_nonzero(rays[US.BLEND_25_BACK, :, 3] < 0) == 25
    for p in range(int(np.prod(vol.counts))):
        changed_i = not np.array_equal(_tile(irr, p, vol.counts, 8), _tile(vol.irradiance, p, vol.counts, 8))
        changed_d = not np.array_equal(_tile(dist, p, vol.counts, 16).view(np.uint16), _tile(vol.distance, p, vol.counts, 16).view(np.uint16))
        left = p in (US.BLEND_INACTIVE, US.BLEND_25_BACK)
        assert changed_i == (not left) and changed_d == (not left), (p, changed_i, changed_d)
    # the same probe with classification off is blended
    on = vol.copy()
    on.classification = False
    irr2, _ = DU.blend(du, k, on, rays)
    assert not np.array_equal(_tile(irr2, US.BLEND_INACTIVE, vol.counts, 8), _tile(vol.irradiance, US.BLEND_INACTIVE, vol.counts, 8))


def test_borders_follow_fill_borders(blended):
    vol, rays, k, irr, dist = blended
    same(irr, ddgi.fill_borders(irr.copy(), 6), "irradiance borders")
    same(dist.view(np.uint16), ddgi.fill_borders(dist.copy(), 14).view(np.uint16), "distance borders")
    assert np.all(irr[DU.interior_mask(irr.shape[1:], 8)[None].repeat(irr.shape[0], 0)] >> 30 == 3)
    dark = DU.unpack10(_tile(irr, US.BLEND_DARK, vol.counts, 8))[1:7, 1:7]
    before = DU.unpack10(_tile(vol.irradiance, US.BLEND_DARK, vol.counts, 8))[1:7, 1:7]
    assert np.all(dark <= before) and np.all(dark[before > 0] < before[before > 0]), "radiance 0 darkens every non-black channel"


def test_blends_agree_with_float64(du, blended):
    """A float64 numpy restatement of both blends from the same float32 inputs against the C reference: the largest difference in
    stored irradiance codes and in binary16 steps of the stored distances is measured and printed, and must not exceed the
    recorded measurement plus one code (the float32 summation order of 256 terms)."""
    vol, rays, k, irr, dist = blended
    irr64, dist64, touched = DU.blend64(du, k, vol, rays)
    assert touched.sum() == int(np.prod(vol.counts)) - 2
    m8 = np.broadcast_to(DU.interior_mask(irr.shape[1:], 8), irr.shape) & ~np.isnan(irr64[..., 0])
    diff = np.abs(DU.unpack10(irr)[m8] - np.rint(irr64[m8]))
    m16 = np.broadcast_to(DU.interior_mask(dist.shape[1:3], 16), dist.shape[:3]) & ~np.isnan(dist64[..., 0])
    got, want = dist[m16].astype(np.float64), dist64[m16]
    step = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14))) - 10)
    ulps = np.abs(got - want) / step
    print(f"float64 agreement: irradiance max {diff.max():.0f} codes over {diff.size} channels ({np.count_nonzero(diff)} differ); "
          f"distance max {ulps.max():.3f} binary16 steps over {ulps.size} values")
    assert m8.sum() == touched.sum() * 36 and m16.sum() == touched.sum() * 196
    assert diff.max() <= MEASURED_IRRADIANCE_CODES + 1
    assert ulps.max() <= MEASURED_DISTANCE_STEPS + 1


# ---- 5b. the blends on both sides of every rule: what the cases of tests/ddgi_blend_scenes.py reach ------------------------------------------
# Every count below comes from the rule words of DU.blend_rules: the reference's own binary32 decisions.
def _count(rules, bit):
    return int(np.count_nonzero(np.asarray(rules) & np.uint32(bit)))


def _radiance_rules(du, names):
    return [step[4] for name in names for step in BS.blend_case(du, name).steps]


def test_rule_exports_leave_the_textures_as_the_blends_do(du, blended):
    """du_blend_radiance_rules and du_blend_distance_rules are the blends' own function bodies: the textures equal DU.blend's word
    for word, every rule word is written, and the left-alone bit is set on exactly the two probes that are left alone."""
    vol, rays, k, irr, dist = blended
    irr2, dist2, rr, dr = DU.blend_rules(du, k, vol, rays)
    same(irr2, irr, "irradiance"); same(dist2.view(np.uint16), dist.view(np.uint16), "distance")
    assert not np.any(rr == 0xFFFFFFFF) and not np.any(dr == 0xFFFFFFFF)
    for rules in (rr, dr):
        left = np.flatnonzero(rules.reshape(len(rules), -1)[:, 0] & 1)
        assert list(left) == [US.BLEND_INACTIVE, US.BLEND_25_BACK] and np.all((rules[left] == 1)) and not np.any(np.delete(rules, left, 0) & 1)


def test_blend_cases_ladders_put_texels_one_code_apart_on_both_sides_of_each_threshold(du):
    """Pairs of texels of one tile whose previous codes on the ladder's channel differ by one and of which one takes the
    threshold and the other does not: at least 8 per threshold; each channel decides the fmax of the three |delta| on at least
    16 texels; with both thresholds 0 every texel takes both, with both infinite none does.  MEASURED over the 16 ladder cases:
    84 pairs at the irradiance threshold, 84 at the brightness threshold (6 per case with finite thresholds: one per tile whose
    ladder straddles it); x / y / z decide 3464 / 3454 / 3450 texels; the 1/1024 floor gives the step on 1553 texels and |delta|
    on 6600."""
    pairs = {DU.R_IRRADIANCE: 0, DU.R_BRIGHTNESS: 0}
    decides = np.zeros(4, np.int64)
    floor = cap = 0
    for name in BS.LADDER_CASES:
        c = BS.blend_case(du, name)
        k, rays, irr, dist, rr, dr = c.steps[0]
        decides += np.bincount((rr >> DU.R_MAX_SHIFT & 3).reshape(-1), minlength=4)
        floor, cap = floor + _count(rr, DU.any_channel(DU.R_FLOOR)), cap + _count(rr, DU.any_channel(DU.R_CAP))
        for p in range(len(rr)):
            codes = DU.unpack10(BS.irradiance_tile(c.vol, p)).reshape(36, 3)[:, p // len(BS.LADDER_OFFSETS)]
            order = np.argsort(codes)
            assert np.all(np.diff(codes[order]) == 1)
            for bit in pairs:
                pairs[bit] += int(np.count_nonzero(np.diff((rr[p].reshape(36)[order] & bit).astype(np.int64))))
        if "thresholds 0" in name:
            assert _count(rr, DU.R_IRRADIANCE) == _count(rr, DU.R_BRIGHTNESS) == rr.size
        if "thresholds inf" in name:
            assert _count(rr, DU.R_IRRADIANCE) == _count(rr, DU.R_BRIGHTNESS) == 0
    print(f"ladders: pairs one code apart on opposite sides: irradiance {pairs[DU.R_IRRADIANCE]}, brightness {pairs[DU.R_BRIGHTNESS]}; fmax decided by x / y / z on {[int(d) for d in decides[1:]]} texels; "
          f"floor binds on {floor} texels, |delta| on {cap}")
    assert pairs[DU.R_IRRADIANCE] >= 8 and pairs[DU.R_BRIGHTNESS] >= 8
    assert decides[0] == 0 and decides[1:].min() >= 16
    assert floor >= 16 and cap >= 16


def test_blend_case_dark_reaches_black(du):
    """Radiance 0 for 12 updates at h = 0.97: every previous code of BS.DARK_CODES is there; under "darker" a channel whose delta is
    exactly 0 has sign(step) == 0, and the floor gives the step; after the last update every non-black channel has fallen by at
    least one code per update (or reached 0).  MEASURED at update 0: darker on 684 of 720 texels (the 36 others are the cleared
    tile), sign(step) == 0 on 648, the floor binding on 432; after 12 updates the codes are 0 but for 512 -> 166 and 1023 -> 177."""
    c = BS.blend_case(du, "dark")
    assert len(c.steps) == BS.DARK_UPDATES == 12
    before = DU.unpack10(c.vol.irradiance)
    assert {tuple(int(v) for v in DU.unpack10(BS.irradiance_tile(c.vol, p))[0, 0]) for p in range(20)} == set(BS.DARK_CODES)
    rr = c.steps[0][4]
    print(f"dark, update 0: darker {_count(rr, DU.R_DARKER)}, sign 0 {_count(rr, DU.any_channel(DU.R_SIGN_ZERO))}, floor {_count(rr, DU.any_channel(DU.R_FLOOR))}")
    assert _count(rr, DU.R_DARKER) >= 600 and _count(rr, DU.any_channel(DU.R_SIGN_ZERO)) >= 600 and _count(rr, DU.any_channel(DU.R_FLOOR)) >= 100
    prev = before
    for step in c.steps:
        now = DU.unpack10(step[2])
        assert np.all(now <= np.maximum(prev - 1, 0)), "one code per update at least"
        prev = now
    assert np.all(prev <= np.maximum(before - 12, 0))
    print(f"dark, after 12 updates: 512 -> {sorted(set(prev[before == 512]))}, 1023 -> {sorted(set(prev[before == 1023]))}, largest of the others {prev[before <= 8].max()}")
    assert prev[before <= 8].max() == 0


def test_blend_cases_bright_and_below_zero_reach_both_clamps(du):
    """Stores above 1 over cleared tiles (the estimate whole), seeded tiles and tiles at code 1023, an estimate of 1e6 and more, a
    negative sum, and stores below 0.  MEASURED (texels with a channel clamped at 1, per update): gamma 5: 222 / 228 / 0 / 324 of 324,
    gamma 1: 259 / 298 / 0 / 324 (43 of them on the seeded tiles in update 0; 6 at gamma 5); the negative sums give res == 0 exactly on all 324; "below zero" clamps 280 of 324 texels at 0."""
    for name in ("bright gamma 5", "bright gamma 1"):
        c = BS.blend_case(du, name)
        one = [_count(s[4], DU.any_channel(DU.R_CLAMP_ONE)) for s in c.steps]
        print(f"{name}: texels clamped at 1 per update {one}")
        assert c.steps[0][4][:3].all() and all(_count(c.steps[0][4][p], DU.R_PREV_ZERO) == 36 for p in range(3)), "cleared tiles"
        assert all(_count(c.steps[0][4][p], DU.R_CLAMP_ONE << p) == 36 for p in range(3)), "the cleared tiles store res > 1 on the bright channel"
        seeded = _count(c.steps[0][4][3:6], DU.any_channel(DU.R_CLAMP_ONE))
        print(f"{name}: {seeded} texels of the seeded tiles eased to above 1 in update 0")
        assert (seeded >= 16 or name != "bright gamma 1") and _count(c.steps[0][4][6:], DU.any_channel(DU.R_CLAMP_ONE)) == 108
        assert one[3] == 324 and one[2] == 0 and _count(c.steps[2][4], DU.R_DARKER) == 324
        assert not np.any(DU.unpack10(c.steps[2][2])[DU.unpack10(c.steps[1][2]) == 0]), "a negative sum is black, not a NaN"
    zero = _count(BS.blend_case(du, "below zero").steps[0][4], DU.any_channel(DU.R_CLAMP_ZERO))
    print(f"below zero: {zero} texels clamped at 0")
    assert zero >= 16


def test_blend_cases_records_reach_nan_sums_and_the_back_face_limit(du):
    """The ten probes of BS.records: only the one with exactly 25 records of -2^-149 is left alone (the ones with -0.0 are blended);
    NaN sums on at least 16 texels.  MEASURED: 54 texels with a NaN sum per update (36 behind the NaN radiance channel, 18 facing away
    from the infinite ray), 72 with a NaN anywhere; the smallest sumW the skip leaves, on the texel whose 24 nearest rays are back
    faces: 42.3 against 64.0 without the skip (the floor is 2.56e-7: see DESIGN.md 9, unreachable)."""
    for name in ("records cleared", "records seeded"):
        c = BS.blend_case(du, name)
        for i, (k, rays, irr, dist, rr, dr) in enumerate(c.steps):
            assert list(np.flatnonzero(rr[:, 0, 0] & 1)) == [BS.REC_25_SUBNORMAL] == list(np.flatnonzero(dr[:, 0, 0] & 1))
            assert np.count_nonzero(rays[BS.REC_25_SUBNORMAL, :, 3] < 0) == 25 and np.count_nonzero(rays[BS.REC_24_AND_NEG_ZERO, :, 3] < 0) == 24
            assert np.count_nonzero(np.signbit(rays[BS.REC_24_AND_NEG_ZERO, :, 3])) == 34 and np.count_nonzero(rays[BS.REC_24_NEAREST, :, 3] < 0) == 24
            print(f"{name}, update {i}: NaN sums {_count(rr, DU.R_SUM_NAN)}, any NaN {_count(rr, DU.R_NAN)}")
            assert _count(rr, DU.R_SUM_NAN) >= 16 and _count(rr[BS.REC_INF], DU.R_SUM_NAN) >= 8 and _count(rr[BS.REC_NAN_CHANNEL], DU.R_SUM_NAN) == 36
            assert _count(dr[BS.REC_NAN_W], 1 << DU.D_CLIPPED_SHIFT | 0x1FF << DU.D_CLIPPED_SHIFT) == 196 and np.all(dr[BS.REC_ZERO_W] >> DU.D_CLIPPED_SHIFT == 0)
    c = BS.blend_case(du, "records cleared")
    k, rays = c.steps[0][0], c.steps[0][1]
    w = np.maximum(0.0, DU.texel_directions(du, 6).astype(np.float64) @ DU.ray_directions(du, k).astype(np.float64).T)
    kept = (w * ~(rays[BS.REC_24_NEAREST, :, 3] < 0)).sum(-1)
    print(f"records: sumW at texel {BS.REC_TEXEL} with its 24 nearest rays skipped {kept[BS.REC_TEXEL[1], BS.REC_TEXEL[0]]:.2f}, unskipped {w.sum(-1)[BS.REC_TEXEL[1], BS.REC_TEXEL[0]]:.2f}")
    assert kept.argmin() == BS.REC_TEXEL[1] * 6 + BS.REC_TEXEL[0] and kept.min() > 16.0


def test_blend_cases_distance_range_leaves_binary16_at_both_ends(du):
    """"distance far": at least 100 infinite halves after update 1; after update 2 (index 1) the infinities survive
    (res + 0.9 * (inf - res)); update index 2, at h = 0, turns them into 0x7E00 (0 * inf) and the next eases from NaN texels.
    "distance tiny": at least 100 subnormal halves.  "distance huge": the squared distance is a NaN everywhere.  "distance exponents": the (0, v) and (v, 0) texels are not cleared texels,
    (-0.0, -0.0) is, and at exponent 30000 sumW is at its floor.  MEASURED: far: texels with an infinite half 328 / 342 / 93 / 96,
    with a NaN half 0 / 0 / 342 / 342 (of 784); a SURVIVING INFINITY after update 2, no 0x7E00 before h = 0; tiny: all 784 texels
    subnormal in both updates; huge: every texel holds (inf, NaN); exponents: sumW at its floor on 0 / 0 / 0 / 0 / 736 texels."""
    far = BS.blend_case(du, "distance far")
    inf, nan = [_count(s[5], DU.D_STORE_INF) for s in far.steps], [_count(s[5], DU.D_STORE_NAN) for s in far.steps]
    print(f"distance far: texels with an infinite half {inf}, with a NaN half {nan}")
    halves = far.steps[0][3].view(np.uint16)
    assert np.count_nonzero((halves & 0x7FFF) == 0x7C00) >= 100 and inf[0] >= 100
    assert _count(far.steps[1][5], DU.D_PREV_INF) >= 100 and inf[1] >= 100 and nan[1] == 0, "the infinity survives an update at h = 0.9"
    assert nan[2] >= 100 and np.count_nonzero(far.steps[2][3].view(np.uint16) == 0x7E00) >= 100 and _count(far.steps[3][5], DU.D_PREV_NAN) >= 100
    assert 0 < inf[0] < far.steps[0][5].size, "finite and infinite texels side by side"
    tiny = BS.blend_case(du, "distance tiny")
    sub = [_count(s[5], DU.D_STORE_SUBNORMAL) for s in tiny.steps]
    print(f"distance tiny: texels with a subnormal half {sub}")
    assert min(sub) >= 100
    ex = BS.blend_case(du, "distance exponents")
    floor = [_count(s[5], DU.D_SUMW_FLOOR) for s in ex.steps]
    print(f"distance exponents: sumW at its floor on {floor} texels")
    assert [float(s[0]["probeDistanceExponent"][0]) for s in ex.steps] == list(BS.EXPONENTS)
    assert [_count(ex.steps[0][5][p], DU.D_PREV_ZERO) for p in range(4)] == [0, 0, 196, 0]
    assert floor[4] >= 100 and floor[3] == 0
    huge = BS.blend_case(du, "distance huge")
    halves = huge.steps[0][3].view(np.uint16)[DU.interior_mask(huge.steps[0][3].shape[1:3], 16)[None]]
    assert np.all(halves[..., 0] == 0x7C00) and np.all(halves[..., 1] == 0x7E00), "d * d overflows binary32: (d * d) * w is inf * 0 on the rays that face away"
    clipped = [int((s[5] >> DU.D_CLIPPED_SHIFT).max()) for s in far.steps]
    assert min(clipped) >= 1, "rays beyond maxDistance"


def test_every_radiance_rule_is_taken_and_not_taken_across_the_blend_cases(du):
    """Every radiance rule bit is set on at least 16 texels and clear on at least 16 across BS.BLEND_CASES; every distance bit
    likewise.  MEASURED of 25 092 radiance words: left alone 144, prev == 0 5130, irradiance 6725, brightness 11 494, darker 12 900, NaN 288, floor
    1232 / 1329 / 1396 (x / y / z), |delta| 7404 / 7337 / 6882, sign 0 3695 / 3714 / 3695, clamped at 1 554 / 549 / 552, at 0 153 / 165 / 163; of
    136 612 distance words: sumW floor 736, store infinite 1643, NaN 1468, subnormal 1568, prev infinite 1155, prev NaN 734; the radiance sumW floor has no bit: it is unreachable
    (DESIGN.md 9)."""
    rr = np.concatenate([s[4].reshape(-1) for name in BS.BLEND_CASES for s in BS.blend_case(du, name).steps])
    dr = np.concatenate([s[5].reshape(-1) for name in BS.BLEND_CASES for s in BS.blend_case(du, name).steps])
    bits = [("left alone", DU.R_LEFT_ALONE), ("prev == 0", DU.R_PREV_ZERO), ("irradiance threshold", DU.R_IRRADIANCE), ("brightness threshold", DU.R_BRIGHTNESS), ("darker", DU.R_DARKER),
            ("NaN", DU.R_NAN), ("NaN sum", DU.R_SUM_NAN)]
    for what, bit in (("floor", DU.R_FLOOR), ("|delta| cap", DU.R_CAP), ("sign 0", DU.R_SIGN_ZERO), ("clamped at 1", DU.R_CLAMP_ONE), ("clamped at 0", DU.R_CLAMP_ZERO)):
        bits += [(f"{what} {'xyz'[c]}", bit << c) for c in range(3)]
    for what, bit in bits:
        n = _count(rr, bit)
        print(f"radiance, {what}: {n} of {rr.size}")
        assert 16 <= n <= rr.size - 16, what
    for what, bit in (("left alone", DU.D_LEFT_ALONE), ("prev == (0, 0)", DU.D_PREV_ZERO), ("sumW floor", DU.D_SUMW_FLOOR), ("store inf", DU.D_STORE_INF), ("store NaN", DU.D_STORE_NAN),
                      ("store subnormal", DU.D_STORE_SUBNORMAL), ("prev inf", DU.D_PREV_INF), ("prev NaN", DU.D_PREV_NAN)):
        n = _count(dr, bit)
        print(f"distance, {what}: {n} of {dr.size}")
        assert 16 <= n <= dr.size - 16, what


@pytest.mark.parametrize("name", BS.TRACED)
def test_blend_cases_behind_the_traces_meet_saturated_records_and_nothing_beyond(sm, dp, name):
    """Three chained reference updates of the trace case under a light of strength 8.  The floors first set for this case (an
    infinite record and 16 NaN sums in "attributes", 16 channels stored above 1) CANNOT be met behind the project's own trace,
    whatever the scene or the light: a record is saturate(rgb), so an infinite emissive arrives as 1.0 and a NaN as 0.0, no sum
    holds a NaN, and an estimate is at most (1 / 2) ^ (1 / gamma) = 0.871, code 891.  Hostile records reach the blends
    from a supplied buffer only (BS.records, BS.bright).  What the strong light does reach is asserted instead: at least 16
    record channels saturated at exactly 1.0 per update, every record finite and within [0, 1], no rule bit for a NaN or a clamp,
    and both thresholds taken and not taken.  MEASURED per update, record channels at 1.0 (the misses' (1, 1, 1)
    among them): attributes 11027 / 11063 / 11091, tlas 65 10652 / 10678 / 10732 of 13824; thresholds taken on 442 to 540 of 648 texels."""
    c = trace_case(sm, dp, name)
    state = c.volume()
    rules = []
    for step in range(BS.TRACED_UPDATES):
        k = BS.traced_consts(name, step)
        rays, _ = DU.trace(dp, k, state, c.scene, DU.WALK, c.init)
        irr, dist, rr, dr = DU.blend_rules(dp, k, state, rays)
        state.irradiance, state.distance = irr, dist
        ones = int(np.count_nonzero(rays[..., :3] == 1.0))
        print(f"{name}, update {step}: {ones} record channels at 1.0, thresholds taken {_count(rr, DU.R_IRRADIANCE)} / {_count(rr, DU.R_BRIGHTNESS)} of {rr.size}")
        assert np.isfinite(rays).all() and rays[..., :3].min() >= 0.0 and rays[..., :3].max() <= 1.0 and ones >= 16
        assert _count(rr, DU.R_NAN | DU.any_channel(DU.R_CLAMP_ONE) | DU.any_channel(DU.R_CLAMP_ZERO)) == 0
        rules.append(rr)
    rules = np.concatenate(rules)
    for bit in (DU.R_IRRADIANCE, DU.R_BRIGHTNESS):
        assert 16 <= _count(rules, bit) <= rules.size - 16


@pytest.mark.parametrize("name", BS.FINITE_CASES)
def test_blend_cases_agree_with_float64(du, name):
    """The float64 restatement on the finite cases (the ladders, "dark", "bright" below 1e30, "below zero"), every update from the
    state the reference left: stored codes within MEASURED_IRRADIANCE_CODES + 1 and distances within MEASURED_DISTANCE_STEPS + 1
    binary16 steps.  Left out: texels at which float64 decides a threshold otherwise than the reference's rule bits say, or
    within FLOAT32_REACH of one; at most 5 % of a case's texels (a condition: the ladders put few codes that close)."""
    c = BS.blend_case(du, name)
    texels = left_out = 0
    worst = worst_d = 0.0
    for step, (k, rays, irr, dist, rr, dr) in enumerate(c.steps):
        if np.abs(rays[..., :3]).max() >= 1e30:
            continue
        vol = c.before(step)
        irr64, dist64, touched, taken, margin = DU.blend64(du, k, vol, rays, decisions=True)
        assert touched.all()
        m8 = np.broadcast_to(DU.interior_mask(irr.shape[1:], 8), irr.shape)
        ref_bits = np.zeros(irr.shape, np.uint32)
        for p in range(len(rr)):
            BS.irradiance_tile(_Words(ref_bits, vol.counts), p)[...] = rr[p] & (DU.R_IRRADIANCE | DU.R_BRIGHTNESS)
        out = m8 & ((taken != ref_bits) | (margin < FLOAT32_REACH))
        keep = m8 & ~out
        texels, left_out = texels + int(m8.sum()), left_out + int(out.sum())
        worst = max(worst, float(np.abs(DU.unpack10(irr)[keep] - np.rint(irr64[keep])).max()))
        m16 = np.broadcast_to(DU.interior_mask(dist.shape[1:3], 16), dist.shape[:3])
        got, want = dist[m16].astype(np.float64), dist64[m16]
        worst_d = max(worst_d, float((np.abs(got - want) / 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14))) - 10)).max()))
    print(f"{name}: float64 agreement: irradiance max {worst:.0f} codes over {texels - left_out} texels, {left_out} left out; distance max {worst_d:.3f} binary16 steps")
    assert left_out <= texels * 0.05
    assert worst <= MEASURED_IRRADIANCE_CODES + 1
    assert worst_d <= MEASURED_DISTANCE_STEPS + 1


# ---- 6. the interface ------------------------------------------------------------------------------------------------------------------
def test_layout_and_helpers(tmp_path):
    out = layout_probe(tmp_path, [("size", "sizeof(interop::DDGIUpdateConsts)"), ("rot", "offsetof(interop::DDGIUpdateConsts, rayRotation)"),
                                  ("max", "offsetof(interop::DDGIUpdateConsts, probeMaxRayDistance)"), ("bright", "offsetof(interop::DDGIUpdateConsts, probeBrightnessThreshold)"),
                                  ("rays", "(size_t)interop::kDDGIRaysPerProbe"), ("limit", "(size_t)interop::kDDGIBackfaceRayLimit")])
    dt = I.DDGIUpdateConsts
    assert int(out["size"]) == 96 == dt.itemsize == I.SIZES["DDGIUpdateConsts"]
    assert (int(out["rot"]), int(out["max"]), int(out["bright"])) == (dt.fields["rayRotation"][1], dt.fields["probeMaxRayDistance"][1], dt.fields["probeBrightnessThreshold"][1])
    assert int(out["rays"]) == I.kDDGIRaysPerProbe == 256 and int(out["limit"]) == I.kDDGIBackfaceRayLimit == int(np.float32(256) * np.float32(0.1))
    r = ddgi.random_rotation(np.random.default_rng(1)).astype(np.float64)
    assert r.shape == (3, 3) and np.allclose(r @ r.T, np.eye(3), atol=1e-6) and np.linalg.det(r) > 0.999
    assert not np.array_equal(r, ddgi.random_rotation(np.random.default_rng(2)))
    v = ddgi.Volume.uniform((0, 0, 0), (1, 1, 1), (2, 2, 2))
    v.data[0, 0, 0] = (0.1, 0.2, 0.3, 1.0)
    data = v.data.copy()
    assert v.reset() is v and not v.irradiance.any() and not v.distance.view(np.uint16).any() and np.array_equal(v.data, data)
    u = ddgi.check_update_settings(dict(seed=3, hysteresis=0.9))
    assert u["seed"] == 3 and u["hysteresis"] == 0.9 and u["distance_exponent"] == 50.0 and u["irradiance_threshold"] == 0.2 and u["brightness_threshold"] == 0.1
    for bad in (dict(speed=1), dict(hysteresis=1.5), dict(hysteresis=float("nan")), dict(seed=-1), dict(distance_exponent=-1.0)):
        with pytest.raises(ValueError, match="ddgi_update"):
            ddgi.check_update_settings(bad)
