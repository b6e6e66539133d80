"""tests/ddgi_update_ref.c on the CPU: the definition of the DDGI probe update ("giprobetrace_CS_ProbeTrace" and the two
"ProbeBlendingCS_DDGIProbeBlendingCS" passes).  The closest-hit walk of the product's node arrays against brute force over every
triangle, the face rule, the encodings the lighting pass's query assumes, the hysteresis, which probes are left alone, the
borders, and a float64 restatement of the two blends.  tests/test_gpu_ddgi_update.py holds the kernels to the same reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_update_ref as DU  # noqa: E402
import ddgi_update_scenes as US  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from ref_build import layout_probe  # noqa: E402
from suite_support import ref_library, same, sm  # noqa: E402, F401
from toyrenderer_amd import ddgi  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

F = np.float32
du = ref_library(DU)
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (-0.0, 0, -1)], F)

# Float64 agreement (test_blends_agree_with_float64): the largest differences MEASURED with US.blend_volume(seed 3) and
# US.blend_rays(seed 4) under rotation seed 2; the test asserts them plus one code for the float32 summation order
# (profiles/ddgi/README.md records them).
MEASURED_IRRADIANCE_CODES = 1                  # 7 of 1080 channels differ, each by one code
MEASURED_DISTANCE_STEPS = 0.501                # of a binary16 step: the store's own rounding and no more


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
