"""Scenes, volumes and ray buffers of the DDGI update tests (tests/test_ddgi_update_ref.py on the CPU, tests/test_gpu_ddgi_update.py on
the GPU): the Cornell fixture, two instances of one cube that share face planes (equal t, so the tie rule decides), a closed cube
around a probe, and the shadow tests' scattered and degenerate scenes; small volumes over them; seeded ray records for the blends.
TRACE_CASES lists what tests/test_gpu_ddgi_trace_scenes.py traces on the GPU and what the CPU file checks the preconditions of."""
import numpy as np

import shadow_scenes as SS
from toyrenderer_amd import ddgi
from toyrenderer_amd import interop as I

F = np.float32
RAYS = I.kDDGIRaysPerProbe
LIGHT = (SS.unit((0.3, 0.8, -0.52)), 3.0)        # towards the sun, as the lighting tests have it


def cube(half=1.0):
    """A closed cube around the origin, 12 triangles, wound like the Cornell fixture's walls but facing OUTWARD: from inside every
    triangle is a back face."""
    h = half
    p = np.array([(-h, -h, -h), (h, -h, -h), (h, h, -h), (-h, h, -h), (-h, -h, h), (h, -h, h), (h, h, h), (-h, h, h)], F)
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]      # cross(v1 - v0, v2 - v0) points outward
    idx = [(a, b, c, a, c, d) for a, b, c, d in quads]
    return p, np.array(idx, np.uint32).reshape(-1)


def closed_cube():
    return SS.make_scene([cube(1.0)], [(0, SS.world_matrix(), 0, "opaque")])


def shared_planes():
    """Two instances of one cube, the second moved by half an edge along y (a power of two, so object-space arithmetic stays exact
    for rays from round positions): their x and z faces lie in the same planes and overlap, so a ray through the overlap meets both
    at the same t; and a third, mirrored one further away."""
    return SS.make_scene([cube(1.0)], [(0, SS.world_matrix(position=(0.0, 0.0, 0.0)), 0, "opaque"), (0, SS.world_matrix(position=(0.0, 0.5, 0.0)), 1, "opaque"),
                                       (0, SS.world_matrix(scale=(1.0, -1.0, 1.0), position=(4.0, 0.0, 0.0)), 2, "alpha")])


SCENES = {"cornell": SS.cornell, "shared planes": shared_planes, "closed cube": closed_cube, "scattered": lambda: SS.scattered(65),
          "degenerate": lambda: SS.single(SS.with_degenerates(), scale=(4.0, 2.0, 5.0), position=(0.0, 0.0, 0.0))}

# origins of the closest-hit rays per scene (every origin shoots the 256 rotated ray directions and the six axis directions)
ORIGINS = {"cornell": [(0.0, 1.0, 0.0), (0.4, 0.3, -0.2), (-0.6, 1.6, 0.5), (0.0, 1.0, 3.0)],
           "shared planes": [(3.0, 0.25, 0.0), (-2.5, 0.125, 0.5), (0.0, 0.25, -3.0), (0.0, 0.0, 0.0), (2.0, 0.75, 0.25)],
           "closed cube": [(0.0, 0.0, 0.0), (0.3, -0.2, 0.6), (3.0, 0.1, 0.2)],
           "scattered": [(0.0, 2.0, -7.0), (3.0, 0.0, -4.0), (-5.0, 5.0, -12.0)],
           "degenerate": [(0.0, 3.0, 0.0), (0.5, -2.0, 0.3)]}


def rotation(seed):
    return ddgi.random_rotation(np.random.default_rng([seed, 99]))


# name -> (counts, spacing, origin): volumes over the Cornell fixture (about 2 units across around (0, 1, 0)); the probes stay off
# the walls.  "3x2x4" reaches outside the box, so some probes see the walls' backs and some rays miss.
CORNELL_VOLUMES = {"2x2x2": ((2, 2, 2), (0.9, 0.8, 0.7), (0.03, 0.95, 0.05)),
                   "3x2x4": ((3, 2, 4), (0.83, 0.77, 0.71), (-0.04, 1.02, 0.35))}


def cornell_volume(name, seeded=False, seed=5):
    """Cleared (Volume.reset) or with seeded contents: random irradiance and distances, relocation offsets on some probes and, in
    "3x2x4", two inactive probes."""
    counts, spacing, origin = CORNELL_VOLUMES[name]
    v = ddgi.Volume(origin, spacing, counts, normal_bias=0.02, view_bias=0.1, gamma=5.0, relocation=True, classification=True).reset()
    if seeded:
        rng = np.random.default_rng([seed, sum(counts)])
        cx, cy, cz = counts
        v.irradiance[...] = ddgi.pack_unorm10(rng.uniform(0.15, 1.0, v.irradiance.shape + (3,)))
        mean = rng.uniform(0.3, 1.4, v.distance.shape[:-1])
        v.distance[..., 0] = (mean * 0.5).astype(np.float16)
        v.distance[..., 1] = (mean * mean * rng.uniform(1.0, 1.5, mean.shape) * 0.5).astype(np.float16)
        moved = rng.random((cy, cz, cx)) < 0.4
        v.data[..., :3] = np.where(moved[..., None], rng.uniform(-0.2, 0.2, (cy, cz, cx, 3)), 0.0).astype(np.float16)
        if name == "3x2x4":
            v.data[0, 1, 2, 3] = v.data[1, 3, 0, 3] = 1.0
        v.fill_borders()
    return v


def blend_volume(seed=3):
    """The volume of the blend tests, 3 x 2 x 2 probes: seeded texels, with probe 1's irradiance and probe 2's distance tiles zero
    (previously zero texels) and probe 4 inactive."""
    v = ddgi.Volume((0.0, 0.0, 0.0), (0.8, 1.1, 0.9), (3, 2, 2), normal_bias=0.02, view_bias=0.1, gamma=5.0, relocation=True, classification=True)
    rng = np.random.default_rng([seed, 12])
    q = rng.integers(0, 1024, v.irradiance.shape + (3,), dtype=np.uint32)
    v.irradiance[...] = q[..., 0] | q[..., 1] << np.uint32(10) | q[..., 2] << np.uint32(20) | np.uint32(3 << 30)
    mean = rng.uniform(0.05, 1.5, v.distance.shape[:-1])
    v.distance[..., 0] = mean.astype(np.float16)
    v.distance[..., 1] = (mean * mean * rng.uniform(1.0, 1.3, mean.shape)).astype(np.float16)
    v.irradiance[0, 0:8, 8:16] = 0
    v.distance[0, 0:16, 32:48] = 0
    v.data[0, 1, 1, 3] = 1.0                                         # probe 4 = (x 1, y 0, z 1)
    return v.fill_borders()


BLEND_INACTIVE, BLEND_24_BACK, BLEND_25_BACK, BLEND_ALL_MISS, BLEND_DARK = 4, 5, 6, 7, 8


def blend_rays(volume, seed=4):
    """float32 [numProbes, 256, 4]: seeded radiance in [0, 1.2) and distances, about 5 % of them negative (back faces); probe 5 has
    exactly 24 negative distances, probe 6 exactly 25, probe 7 only misses ((1, 1, 1), 1e27), probe 8 radiance 0."""
    n = int(np.prod(volume.counts))
    rng = np.random.default_rng([seed, n])
    r = np.zeros((n, RAYS, 4), F)
    r[..., :3] = rng.uniform(0.0, 1.2, (n, RAYS, 3))
    r[..., 3] = rng.uniform(0.05, 2.5, (n, RAYS))
    back = rng.random((n, RAYS)) < 0.05
    back[:, 200:] = False
    for p in range(n):
        while back[p].sum() > 20:
            back[p, np.flatnonzero(back[p])[0]] = False
    for p, count in ((BLEND_24_BACK, 24), (BLEND_25_BACK, 25)):
        back[p] = False
        back[p, rng.choice(RAYS, count, replace=False)] = True
    r[..., 3] = np.where(back, -0.2 * r[..., 3], r[..., 3])
    r[..., :3] = np.where(back[..., None], 0.0, r[..., :3])
    r[BLEND_ALL_MISS] = (1.0, 1.0, 1.0, 1e27)
    r[BLEND_DARK, :, :3] = 0.0
    r[BLEND_DARK, :, 3] = np.abs(r[BLEND_DARK, :, 3])
    return r


# ---- the cases of the trace on scenes that tell a wrong walk apart (tests/test_gpu_ddgi_trace_scenes.py) -------------------------------
def with_normals(sc, seed=31):
    """A copy of a scene dict whose every vertex carries a seeded unit normal packed as the trace's unpackNormal reads it (10 bits
    each, x in bits 20-29).  SS.make_scene leaves m_PackedNormal at 0: one constant normal, under which neither the barycentric
    interpolation nor the space the normal lives in can show."""
    rng = np.random.default_rng([seed, len(sc["vertices"])])
    n = rng.normal(size=(len(sc["vertices"]), 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    q = np.rint((n * 0.5 + 0.5) * 1023.0).astype(np.uint32)
    out = dict(sc)
    out["vertices"] = sc["vertices"].copy()
    out["vertices"]["m_PackedNormal"] = (q[:, 0] << 20) | (q[:, 1] << 10) | q[:, 2]
    return out


def trace_volume(counts, lo, hi, seeded=True):
    """A volume whose first probe stands at `lo` and whose last at `hi` (an axis with one probe: at lo), relocation and
    classification on; cleared, or filled by DU.seeded_volume(vol, 9)."""
    import ddgi_update_ref as DU
    lo, hi, c = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(counts)
    spacing = np.where(c > 1, (hi - lo) / np.maximum(c - 1, 1), 1.0)
    origin = np.where(c > 1, (lo + hi) * 0.5, lo)
    v = ddgi.Volume(tuple(origin), tuple(spacing), tuple(counts), normal_bias=0.02, view_bias=0.1, gamma=5.0, relocation=True, classification=True).reset()
    return DU.seeded_volume(v, 9) if seeded else v


def scattered_volume(seeded=True):
    """3 x 2 x 3 probes over the region SS.scattered fills: 18 probes, 4608 rays."""
    return trace_volume((3, 2, 3), (-5.0, 0.0, -12.0), (5.0, 5.0, -3.0), seeded)


def fixed_ray_volume():
    """3 x 1 x 11 = 33 probes of spacing (4, 1, 0.9) around (0, 2, -7.5): the last wave of the fixed-ray trace holds one probe."""
    return trace_volume((3, 1, 11), (-4.0, 2.0, -12.0), (4.0, 2.0, -3.0), seeded=False)


def moved_instances(sc, seed=17):
    """The scene's instances with every third translated by a seeded offset in [-8, 8]^3: out of the boxes the TLAS was built with."""
    rng = np.random.default_rng([seed, len(sc["instances"])])
    inst = sc["instances"].copy()
    for i in range(0, len(inst), 3):
        inst["m_WorldMatrix"][i][3, :3] += rng.uniform(-8.0, 8.0, 3).astype(F)
    return inst


ATTR_PAST = lambda i: i % 7 == 3                  # noqa: E731   a material index past the buffer
ATTR_UNLISTED = lambda i: i % 9 == 4              # noqa: E731   in neither id list: flags == 0
ATTR_INF = lambda i: i % 13 == 6 and not ATTR_PAST(i)      # noqa: E731   the row whose emissive is +inf


def attributes(listed=False):
    """SS.scattered(65) with seeded normals and the attributes the Cornell fixture lacks: material 1 emissive, material 0 with a NaN
    in its albedo, a fifth row with an infinite emissive on a few instances, material indices one past the buffer and 0xFFFFFFFF in
    turn on the instances with i % 7 == 3, and the instances with i % 9 == 4 in neither id list (listed=True: left in, for the
    precondition that rays would otherwise end on them)."""
    sc = with_normals(SS.scattered(65))
    m = np.zeros(5, I.MaterialData)
    m[:4] = sc["materials"]
    m[4] = sc["materials"][1]
    m["m_ConstEmissive"][1] = (0.4, 0.0, 2.0)
    m["m_ConstAlbedo"][0, :3] = (0.95, 0.2, np.nan)
    m["m_ConstEmissive"][4] = (np.inf, np.inf, np.inf)
    inst = sc["instances"].copy()
    past = 0
    for i in range(len(inst)):
        if ATTR_INF(i):
            inst["m_MaterialDataIdx"][i] = 4
        if ATTR_PAST(i):
            inst["m_MaterialDataIdx"][i] = (len(m), 0xFFFFFFFF)[past % 2]
            past += 1
    sc["materials"], sc["instances"] = m, inst
    if not listed:
        sc["opaqueIds"] = np.array([i for i in sc["opaqueIds"] if not ATTR_UNLISTED(int(i))], np.uint32)
        sc["alphaMaskIds"] = np.array([i for i in sc["alphaMaskIds"] if not ATTR_UNLISTED(int(i))], np.uint32)
    return sc


def _trace_consts(**kw):
    import ddgi_update_ref as DU
    return DU.consts(**{"light": LIGHT, "rotation": rotation(7), **kw})


def _trace_cases():
    scattered = lambda n: (lambda: with_normals(SS.scattered(n)))      # noqa: E731
    cases = {f"tlas {n}": (scattered(n), None, scattered_volume, _trace_consts()) for n in SS.TLAS_COUNTS}
    cases["cleared"] = (scattered(65), None, lambda: scattered_volume(False), _trace_consts())
    cases["moved"] = (scattered(65), moved_instances, scattered_volume, _trace_consts())
    cases["shared planes"] = (lambda: with_normals(shared_planes()), None, lambda: trace_volume((3, 2, 3), (-3.0, 0.0, -3.0), (3.0, 0.5, 3.0)),
                              _trace_consts(light=((1.0, 0.0, 0.0), 2.0)))
    cases["degenerate"] = (lambda: with_normals(SCENES["degenerate"]()), None, lambda: trace_volume((2, 2, 2), (-2.0, -2.5, -2.0), (2.0, 3.0, 2.0)), _trace_consts())
    cases["attributes"] = (attributes, None, scattered_volume, _trace_consts())
    for tmax in (2.0, 4.0):
        cases[f"tmax {tmax:g}"] = (scattered(65), None, scattered_volume, _trace_consts(max_ray_distance=tmax))
    for name in ("down", "up", "x", "negzero"):
        cases[f"light {name}"] = (scattered(65), None, scattered_volume, _trace_consts(light=(SS.LIGHTS[name], 3.0)))
    cases["one probe"] = (scattered(65), None, lambda: trace_volume((1, 1, 1), (0.0, 2.5, -7.5), (0.0, 2.5, -7.5)), _trace_consts())
    return cases


# name -> (scene maker, moved instances (a function of the scene) or None, volume maker, DDGIUpdateConsts)
TRACE_CASES = _trace_cases()
FIXED_RAY_CASES = ["tlas 65", "tlas 257", "moved", "shared planes", "attributes"]
