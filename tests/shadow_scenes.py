"""Seeded scenes, cameras and images for the shadow mask tests (tests/test_shadowmask_ref.py on the CPU, tests/test_gpu_shadowmask.py
on the GPU): a few hundred triangles at most, so that brute force over every texel takes milliseconds.

A scene is a dict: vertices (RawVertexFormat), indices (uint32, per mesh relative to its first vertex), meshData (m_GlobalVertexBufferIdx
and m_GlobalIndexBufferIdx set), index_counts (uint32 per mesh), instances (BasePassInstanceConstants), opaqueIds, alphaMaskIds,
materials (MaterialData).  CASES lists what both test files run.

WALK_CASES are the directed scenes of tests/test_gpu_shadow_walk_scenes.py: each sits on one rule of the any-hit walk (occluded() in
csrc/k_shadowmask.hip) or of the refit, where the seeded CASES do not; tests/test_shadowmask_ref.py asserts that it does."""
import os

import numpy as np

import shadowmask_ref as SR
from toyrenderer_amd import accel, synth
from toyrenderer_amd import interop as I

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
L = 4                                               # the BLAS leaf capacity (asserted against the builder by the CPU tests)


# ---- meshes: (positions float32 [n, 3], indices uint32 [3 t]) ------------------------------------------------------------------------
def strip(n_tris, seed=0, size=1.0):
    """n_tris triangles of a jittered ribbon in the plane y = 0, about `size` wide."""
    rng = np.random.default_rng([seed, n_tris])
    n = n_tris + 2
    x = np.linspace(-size, size, (n + 1) // 2)
    p = np.zeros((n, 3), F)
    p[0::2, 0], p[1::2, 0] = x[:len(p[0::2])], x[:len(p[1::2])]
    p[0::2, 2], p[1::2, 2] = -0.5 * size, 0.5 * size
    p[:, 1] = rng.uniform(-0.05, 0.05, n) * size
    idx = np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n_tris)], np.uint32)
    return p, idx.reshape(-1)


def blob(n_tris, seed):
    """n_tris random triangles of edge about 0.4 in the unit cube around the origin."""
    rng = np.random.default_rng([seed, 77])
    c = rng.uniform(-1.0, 1.0, (n_tris, 1, 3))
    p = (c + rng.uniform(-0.2, 0.2, (n_tris, 3, 3))).astype(F).reshape(-1, 3)
    return p, np.arange(3 * n_tris, dtype=np.uint32)


def with_degenerates(seed=3):
    """A blob of 24 triangles with zero-area ones among them: a repeated vertex, three collinear points, three equal points; and a
    triangle with a NaN and one with an infinite vertex (never hit; left out of the tree)."""
    p, idx = blob(24, seed)
    p = p.copy()
    p[3 * 2 + 1] = p[3 * 2]                                          # repeated vertex
    p[3 * 5 + 2] = p[3 * 5] + (p[3 * 5 + 1] - p[3 * 5]) * F(0.5)     # collinear
    p[3 * 9 + 1] = p[3 * 9 + 2] = p[3 * 9]                           # a point
    p[3 * 13, 1] = np.nan
    p[3 * 17 + 2, 0] = np.inf
    return p, idx


def tetrahedron():
    p = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], F) * F(0.5)
    return p, np.array([0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2], np.uint32)


def quad(half=1.0):
    p = np.array([(-half, 0, -half), (half, 0, -half), (half, 0, half), (-half, 0, half)], F)
    return p, np.array([0, 1, 2, 0, 2, 3], np.uint32)


def collinear_growing(n=4096):
    """The hostile mesh of the depth bound: n zero-area triangles on one line whose size grows geometrically, so that a midpoint split
    peels off one triangle per level."""
    x = np.cumsum(np.geomspace(1e-6, 1e3, n + 2)).astype(F)
    p = np.zeros((n + 2, 3), F)
    p[:, 0] = x
    idx = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1).astype(np.uint32)
    return p, idx.reshape(-1)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def world_matrix(scale=(1, 1, 1), axis=(0, 1, 0), angle=0.0, position=(0, 0, 0)):
    """Row vectors: scale, then rotate, then translate (a negative scale mirrors)."""
    W = np.eye(4)
    W[:3, :3] = np.diag(np.asarray(scale, np.float64)) @ rotation(axis, angle)
    W[3, :3] = position
    return W.astype(F)


def materials(n=4):
    m = synth.materials(5, n)
    m["m_ConstAlbedo"][:, 3] = 1.0
    m["m_AlphaCutoff"] = 0.5
    return m


def make_scene(meshes, placements, mats=None):
    """meshes: [(positions, indices)]; placements: [(mesh index, world matrix, material index, "opaque" | "alpha" | None)]."""
    v = np.zeros(sum(len(p) for p, _ in meshes), I.RawVertexFormat)
    md = np.zeros(len(meshes), I.MeshData)
    counts = np.zeros(len(meshes), np.uint32)
    idx, vat, iat = [], 0, 0
    for m, (p, i) in enumerate(meshes):
        v["m_Position"][vat:vat + len(p)] = p
        md["m_GlobalVertexBufferIdx"][m], md["m_GlobalIndexBufferIdx"][m], md["m_NumLODs"][m] = vat, iat, 1
        counts[m] = len(i)
        idx.append(np.asarray(i, np.uint32))
        vat += len(p); iat += len(i)
    inst = np.zeros(len(placements), I.BasePassInstanceConstants)
    opaque, alpha = [], []
    for k, (m, W, mat, lst) in enumerate(placements):
        inst["m_WorldMatrix"][k] = inst["m_PrevWorldMatrix"][k] = W
        inst["m_MeshDataIdx"][k], inst["m_MaterialDataIdx"][k] = m, mat
        if lst == "opaque":
            opaque.append(k)
        elif lst == "alpha":
            alpha.append(k)
    return dict(vertices=v, indices=np.concatenate(idx) if idx else np.zeros(0, np.uint32), meshData=md, index_counts=counts, instances=inst,
                opaqueIds=np.array(opaque, np.uint32), alphaMaskIds=np.array(alpha, np.uint32), materials=materials() if mats is None else mats)


def single(mesh, scale=(6.0, 1.0, 8.0), position=(0.0, 4.0, -7.0), **kw):
    """One instance of one mesh, above the region the test camera looks at."""
    return make_scene([mesh], [(0, world_matrix(scale=scale, axis=(0.2, 1.0, 0.1), angle=0.4, position=position, **kw), 0, "opaque")])


def scattered(n, seed=11):
    """n instances of three small meshes between the camera's region and the light: every third rotated, every fourth scaled
    non-uniformly, every fifth mirrored; a tenth of them in the alpha-mask list (materials 2 and 3: below and above the cutoff)."""
    rng = np.random.default_rng([seed, n])
    meshes = [tetrahedron(), blob(9, seed), strip(5, seed)]
    mats = materials()
    mats["m_ConstAlbedo"][2, 3], mats["m_ConstAlbedo"][3, 3] = 0.25, 0.75
    placements = []
    for i in range(n):
        scale = np.array([1.3, 1.3, 1.3]) * rng.uniform(0.6, 1.4)
        if i % 4 == 1:
            scale = scale * np.array([2.0, 0.4, 1.0])
        if i % 5 == 2:
            scale = scale * np.array([1.0, -1.0, 1.0])
        W = world_matrix(scale=scale, axis=rng.normal(size=3), angle=rng.uniform(0, 6.28) if i % 3 else 0.0,
                         position=(rng.uniform(-6, 6), rng.uniform(-1, 6), rng.uniform(-13, -2)))
        lst, mat = ("alpha", 2 + (i // 10) % 2) if i % 10 == 7 else ("opaque", i % 2)
        placements.append((i % 3, W, mat, lst))
    return make_scene(meshes, placements, mats)


def cornell():
    """tests/golden/cornell_scene.npz with its rest transforms applied and its index buffer rebuilt from the LOD-0 meshlets: all
    walls coplanar and axis-aligned, so every wall's box has no thickness."""
    import json

    from suite_support import cornell_fixture
    from toyrenderer_amd import cached_scene, gltf_lite
    with open(os.path.join(HERE, "golden", "cornell_materials.json")) as f:
        cm = json.load(f)
    _, s, camera = cornell_fixture()
    s.materials = gltf_lite.material_table([{"pbrMetallicRoughness": {"baseColorFactor": c, "metallicFactor": 0}} for c in cm["baseColorFactor"]])
    s.primMaterial = np.array(cm["primitiveMaterial"], np.uint32)
    inst = gltf_lite.apply_materials(s)
    inst["m_WorldMatrix"] = inst["m_PrevWorldMatrix"] = node_world_matrices(s.nodes)[s.primToNode]
    c = cached_scene.from_scene(s)
    return dict(vertices=s.vertices, indices=c.indices, meshData=c.meshData, index_counts=c.meshSpecific["m_NumIndices"], instances=inst, opaqueIds=s.opaqueIds,
                alphaMaskIds=s.alphaMaskIds, materials=s.materials, loaded=s, camera=camera, cached=c)


def node_world_matrices(nodes):
    """MakeWorldMatrix up the parent chain in float64, rounded once (the tests that need the kernel's bits run the kernel)."""
    def local(n):
        x, y, z, w = (float(v) for v in n["m_Rotation"])
        R = np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y + 2 * z * w, 2 * x * z - 2 * y * w], [2 * x * y - 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z + 2 * x * w],
                      [2 * x * z + 2 * y * w, 2 * y * z - 2 * x * w, 1 - 2 * x * x - 2 * y * y]])
        M = np.eye(4)
        M[:3, :3] = R
        S = np.diag(np.append(n["m_Scale"].astype(np.float64), 1.0))
        T = np.eye(4); T[3, :3] = n["m_Position"]
        return M @ S @ T
    out = np.zeros((len(nodes), 4, 4), F)
    for i in range(len(nodes)):
        W, p = local(nodes[i]), int(nodes[i]["m_ParentNodeIdx"])
        while p != 0xFFFFFFFF:
            W, p = W @ local(nodes[p]), int(nodes[p]["m_ParentNodeIdx"])
        out[i] = W
    return out


# ---- camera, images, constants ---------------------------------------------------------------------------------------------------------
EYE = (0.0, 1.5, 4.0)


def noise_image(seed=1):
    """uint8 [128, 128, 4]: random bytes, with the byte pairs that make MapToCone's offset (0, 0) impossible in bytes (127.5) left
    out and the corners 0 and 255 among the first texels."""
    rng = np.random.default_rng([seed, 128])
    n = rng.integers(0, 256, (128, 128, 4), dtype=np.uint64).astype(np.uint8)
    n[0, 0, :2], n[0, 1, :2], n[0, 2, :2], n[0, 3, :2] = (0, 0), (255, 255), (0, 255), (255, 0)
    return n


def images(W, H, seed, far_share=0.1):
    """(depth float32 [H, W], GBufferA uint32 [H, W, 4]): positions 2 to 12 units in front of the camera (reverse-Z, infinite far:
    depth = near / distance along the view axis), a share of far texels (0.0f; one of them -0.0f), random normal words."""
    rng = np.random.default_rng([seed, W, H])
    depth = (F(0.1) / rng.uniform(2.0, 12.0, (H, W)).astype(F)).astype(F)
    far = rng.random((H, W)) < far_share
    depth[far] = 0.0
    flat = depth.reshape(-1)
    if len(flat) > 3:
        flat[1], flat[2] = 0.0, -0.0
    g = rng.integers(0, 1 << 32, (H, W, 4), dtype=np.uint64).astype(np.uint32)
    return depth, g


def consts(W, H, light=(0.0, -1.0, 0.0), soft=True, frame_counter=0, ray_start_offset=0.01, diameter=accel.DEFAULT_SUN_ANGULAR_DIAMETER, eye=EYE, yaw=0.0):
    v = synth.make_view(eye=eye, yaw=yaw, render=(W, H))
    s = dict(soft=soft, sun_angular_diameter=diameter, ray_start_offset=ray_start_offset)
    return accel.shadow_consts(I.clip_to_world(v.worldToView, v.viewToClip), light, eye, W, H, s, frame_counter)


def unit(v):
    v = np.asarray(v, np.float64)
    return tuple(float(x) for x in (v / np.linalg.norm(v)).astype(F))


# The light vector is the direction TOWARDS the sun (the ray's direction).
LIGHTS = {"down": (0.0, -1.0, 0.0), "up": (0.0, 1.0, 0.0), "x": (1.0, 0.0, 0.0), "negzero": (-0.0, 1.0, -0.0), "generic": unit((0.3, 0.8, -0.52))}
SIZES = [(1, 1), (7, 5), (8, 8), (9, 9), (67, 35)]
TLAS_COUNTS = [1, 2, 3, 64, 65, 257]
BLAS_SHAPES = {"one triangle": lambda: single(strip(1)), "L": lambda: single(strip(L)), "L+1": lambda: single(strip(L + 1)), "2L+1": lambda: single(strip(2 * L + 1)),
               "degenerate": lambda: single(with_degenerates(), scale=(4.0, 2.0, 5.0)), "cornell": cornell}

# (name, scene maker, (W, H), light, soft, frame counter)
CASES = []
for _name, _mk in BLAS_SHAPES.items():
    CASES.append((f"blas {_name}", _mk, (67, 35), "generic" if _name == "cornell" else "up", True, 3))
for _n in TLAS_COUNTS:
    CASES.append((f"tlas {_n}", (lambda n=_n: scattered(n)), (67, 35), "generic", True, 5))
for _s in SIZES:
    CASES.append((f"size {_s[0]}x{_s[1]}", (lambda: scattered(40)), _s, "generic", False, 0))
for _l in LIGHTS:
    for _soft in (False, True):
        CASES.append((f"light {_l} soft {_soft}", (lambda: scattered(65)), (33, 17), _l, _soft, 7))
for _f in (0, 1, 255, 256):
    CASES.append((f"frame {_f}", (lambda: scattered(33)), (33, 17), "generic", True, _f))


def case_inputs(case):
    """(scene, consts, depth, gbuffer, noise) of one CASES entry; the Cornell case looks through the fixture's own camera."""
    name, mk, (W, H), light, soft, frame = case
    sc = mk()
    seed = sum(ord(c) for c in name)
    depth, g = images(W, H, seed)
    if "camera" in sc:
        from toyrenderer_amd import gltf_lite
        cam = sc["camera"]
        v = gltf_lite.view_of(cam, (W, H))
        k = accel.shadow_consts(I.clip_to_world(v.worldToView, v.viewToClip), LIGHTS[light], cam.position, W, H,
                                dict(soft=soft, sun_angular_diameter=accel.DEFAULT_SUN_ANGULAR_DIAMETER, ray_start_offset=0.01), frame)
        rng = np.random.default_rng(seed)
        depth = np.where(depth == 0, depth, (F(cam.znear) / rng.uniform(4.05, 5.95, (H, W))).astype(F))       # inside the box
    else:
        k = consts(W, H, LIGHTS[light], soft, frame)
    return sc, k, depth, g, noise_image()


# ---- the directed scenes of the walk ---------------------------------------------------------------------------------------------------------
# name -> maker(sm) -> dict(sc, k, depth, g, noise, moved: the instances uploaded after the structure was built or None, singular: the
# instances whose world matrix has no inverse, info: what the preconditions need).  sm is tests/shadowmask_ref.c's library: the TMin
# ladder is built from the texels' own rays.
TMIN = 0.25                                         # the ladder's m_RayStartOffset
RUNGS = (0.25, 0.5, 0.9, 1.1, 2.0, 4.0)             # a rung's triangles lie at t = rung * TMIN on their texel's ray
PER_RUNG = 24
LADDER_INSTANCES = {"scale 1": dict(), "scale 0.25": dict(scale=(0.25, 0.25, 0.25)), "scale 4": dict(scale=(4.0, 4.0, 4.0)),
                    "rotated": dict(axis=(0.3, 1.0, 0.2), angle=0.9), "mirrored": dict(scale=(1.0, -1.0, 1.0), axis=(0.1, 0.2, 1.0), angle=0.3)}
LADDER_SCALE = {"scale 1": 1.0, "scale 0.25": 0.25, "scale 4": 4.0, "rotated": 1.0, "mirrored": 1.0}


def _walk_case(sc, W, H, light, soft, name, ray_start_offset=0.01, frame=3, **extra):
    depth, g = images(W, H, sum(ord(c) for c in name))
    return dict(sc=sc, k=consts(W, H, light, soft, frame, ray_start_offset=ray_start_offset), depth=depth, g=g, noise=noise_image(), moved=None, singular=(), info={}, **extra)


def ladder(sm, variant, soft):
    """One triangle of circumradius 0.01 per chosen texel, across that texel's own ray (SR.texel_rays) at t = rung * TMIN, PER_RUNG
    texels per rung, all in one instance placed by LADDER_INSTANCES[variant].  A texel is chosen only if its triangle's centre is
    farther than 0.03 from every other texel's ray, so a ray meets its own triangle or none."""
    name = f"ladder {variant} soft {soft}"
    W, H = 67, 35
    c = _walk_case(None, W, H, LIGHTS["generic"], soft, "ladder", ray_start_offset=TMIN)
    valid, o, d, _ = SR.texel_rays(sm, c["k"], c["depth"], c["g"], c["noise"])
    at = np.flatnonzero(valid.reshape(-1))
    O, D = o.reshape(-1, 3)[at].astype(np.float64), d.reshape(-1, 3)[at].astype(np.float64)
    rng = np.random.default_rng([41, int(soft)])
    chosen, rungs, tris = [], [], []
    for i in rng.permutation(len(at)):
        rung = RUNGS[len(chosen) % len(RUNGS)]
        centre = O[i] + rung * TMIN * D[i]
        v = centre - O
        off = np.linalg.norm(v - np.sum(v * D, 1, keepdims=True) * D / np.sum(D * D, 1, keepdims=True), axis=1)
        off[i] = np.inf
        if off.min() < 0.03:
            continue
        e = np.eye(3)[np.argmin(np.abs(D[i]))]
        u = np.cross(D[i], e); u /= np.linalg.norm(u)
        w = np.cross(D[i], u); w /= np.linalg.norm(w)
        a = rng.uniform(0, 2 * np.pi) + np.arange(3) * (2 * np.pi / 3)
        tris.append(centre + 0.01 * (np.cos(a)[:, None] * u + np.sin(a)[:, None] * w))
        chosen.append(int(at[i])); rungs.append(rung)
        if len(chosen) == PER_RUNG * len(RUNGS):
            break
    assert len(chosen) == PER_RUNG * len(RUNGS), f"{name}: only {len(chosen)} texels stand clear of their neighbours"
    Wm = world_matrix(position=(0.5, 1.0, -5.0), **LADDER_INSTANCES[variant])
    M = Wm.astype(np.float64)
    p = ((np.concatenate(tris) - M[3, :3]) @ np.linalg.inv(M[:3, :3])).astype(F)
    c["sc"] = make_scene([(p, np.arange(len(p), dtype=np.uint32))], [(0, Wm, 0, "opaque")])
    c["info"] = dict(texels=np.array(chosen), rungs=np.array(rungs), scale=LADDER_SCALE[variant])
    return c


def far_roof(height, inner_scale, soft):
    """Two triangles 2e11 wide at `height` over everything, the light straight up: the mesh 2e11 / inner_scale wide in an instance
    of scale inner_scale (1e11: the unit quad, scaled in its plane only, as the alpha test's roof is)."""
    if inner_scale == 1e11:
        mesh, scale = quad(1.0), (1e11, 1.0, 1e11)
    else:
        mesh, scale = quad(1e11 / inner_scale), (inner_scale,) * 3
    sc = make_scene([mesh], [(0, world_matrix(scale=scale, position=(0.0, height, 0.0)), 0, "opaque")])
    return _walk_case(sc, 33, 17, LIGHTS["up"], soft, "far roof")


SINGULAR = {"scale (1, 0, 1)": (1.0, 0.0, 1.0), "scale 0": (0.0, 0.0, 0.0), "scale 1e-20": (1e-20,) * 3, "scale 1e15": (1e15,) * 3}
SINGULAR_INSTANCE = 3


def singular(which, lst, soft):
    """scattered(8) with instance 3's world matrix replaced by a scale that has no inverse in binary32 (or, 1e15, a barely finite
    one) at the instance's place; lst "alpha": that instance in the alpha-mask list with material 3, which passes the alpha test."""
    sc = scattered(8)
    i = SINGULAR_INSTANCE
    pos = sc["instances"]["m_WorldMatrix"][i][3, :3].copy()
    sc["instances"]["m_WorldMatrix"][i] = sc["instances"]["m_PrevWorldMatrix"][i] = world_matrix(scale=SINGULAR[which], position=pos)
    if lst == "alpha":
        sc["opaqueIds"] = sc["opaqueIds"][sc["opaqueIds"] != i]
        sc["alphaMaskIds"] = np.sort(np.append(sc["alphaMaskIds"], np.uint32(i))).astype(np.uint32)
        sc["instances"]["m_MaterialDataIdx"][i] = 3
    c = _walk_case(sc, 33, 17, LIGHTS["generic"], soft, "singular")
    c["singular"] = (i,) if which != "scale 1e15" else ()
    return c


def chain(n=64):
    """The hostile scene of the TLAS's depth: instances along the light's direction from the world's origin (binary32 keeps small
    distances apart there), in groups whose distance grows by 2.4 from group to group, each group an eighth of what is left below it
    (at least one): the builder's midpoint split peels one group per level for as long as it trusts its heuristic.  Mirrors
    collinear_growing() for the BLAS.  Unrotated tetrahedra and quads: their boxes are symmetric, so a box's centre is the instance's
    position whatever its scale, which stays between 0.05 and 1.5 although the nearest group is 1e-6 from the origin: instances
    that shrink with their distance would be far smaller than any shadow ray can resolve (profiles/shadowmask/README.md, "An open
    question")."""
    sizes, left = [], n
    while left:
        sizes.append(max(left // 8, 1)); left -= sizes[-1]
    sizes = sizes[::-1]                                                       # the nearest group first
    rng = np.random.default_rng([13, n])
    light = np.array(LIGHTS["generic"], np.float64)
    placements, dist = [], 1e4 * 2.4 ** -len(sizes)
    for size in sizes:
        dist *= 2.4
        for j in range(size):
            d = dist * (1.0 + 0.02 * j)
            jitter = 0.05 * d * rng.uniform(-1, 1, 2)
            k = len(placements)
            W = world_matrix(scale=np.array([1.0, 1.0, 1.0]) * float(np.clip(0.1 * d, 0.05, 1.5)), position=light * d + np.array([jitter[0], 0.0, jitter[1]]))
            placements.append((k % 2, W, k % 2, "opaque"))
    return make_scene([tetrahedron(), quad(1.0)], placements)


def moved_tenth(sc, seed=17):
    """The scene's instances with every tenth one (i % 10 == 3) carried 10 to 20 units away, out of its rest box."""
    rng = np.random.default_rng([seed, len(sc["instances"])])
    moved = sc["instances"].copy()
    for i in range(3, len(moved), 10):
        v = rng.normal(size=3)
        moved["m_PrevWorldMatrix"][i] = moved["m_WorldMatrix"][i]
        moved["m_WorldMatrix"][i][3, :3] += (v / np.linalg.norm(v) * rng.uniform(10.0, 20.0)).astype(F)
    return moved


def large(which, moved, soft):
    """scattered(513), scattered(1025) (a refit level of 378 inner nodes: the one workgroup of 256 threads strides it twice) or the
    chain; moved: moved_tenth() is uploaded after the structure was built, so the refit changes boxes on every level."""
    sc = chain() if which == "chain" else scattered(int(which))
    c = _walk_case(sc, 33, 17, LIGHTS["generic"], soft, "large")
    if moved:
        c["moved"] = moved_tenth(sc)
    return c


PAST_MATERIALS = {"numMaterials": 4, "0xFFFFFFFF": 0xFFFFFFFF}


def past_material_roof(lst, which, soft):
    """The alpha test's roof over everything with a material index past the 4 materials: in the alpha-mask list it casts nothing
    (material 0, which a clamped index would read, passes the alpha test), in the opaque list the index is never read."""
    roof = world_matrix(scale=(60.0, 1.0, 60.0), position=(0.0, 30.0, 0.0))
    speck = world_matrix(scale=(0.01, 0.01, 0.01), position=(0.0, -50.0, 0.0))
    sc = make_scene([quad(1.0), tetrahedron()], [(1, speck, 0, "opaque"), (0, roof, PAST_MATERIALS[which], lst)])
    return _walk_case(sc, 33, 17, LIGHTS["up"], soft, "past material")


EDGE_LIGHTS = {"zero": (0.0, 0.0, 0.0), "two equal largest": unit((1.0, 1.0, 0.0))}


def edge_light(which, soft):
    """scattered(65) under the zero vector (every ray is NaN) or under a light whose two largest components are equal (the
    triangle test's choice of the ray's largest axis meets a tie)."""
    return _walk_case(scattered(65), 33, 17, EDGE_LIGHTS[which], soft, "edge light")


WALK_CASES = {}
for _soft in (False, True):
    _s = "soft" if _soft else "hard"
    for _v in LADDER_INSTANCES:
        WALK_CASES[f"ladder {_v} {_s}"] = (lambda sm, v=_v, soft=_soft: ladder(sm, v, soft))
    for _n, (_h, _i) in {"tmax roof at 5e9": (5e9, 1e11), "tmax roof at 2e10": (2e10, 1e11), "tmax roof at 5e9 scale 1e3": (5e9, 1e3),
                      "tmax roof at 2e10 scale 1e3": (2e10, 1e3)}.items():
        WALK_CASES[f"{_n} {_s}"] = (lambda sm, h=_h, i=_i, soft=_soft: far_roof(h, i, soft))
    for _w in SINGULAR:
        for _l in ("opaque", "alpha"):
            WALK_CASES[f"singular {_w} {_l} {_s}"] = (lambda sm, w=_w, lst=_l, soft=_soft: singular(w, lst, soft))
    for _w, _m in (("513", False), ("1025", False), ("1025", True), ("chain", False), ("chain", True)):
        WALK_CASES[f"tlas {_w}{' moved' if _m else ''} {_s}"] = (lambda sm, w=_w, m=_m, soft=_soft: large(w, m, soft))
    for _l in ("alpha", "opaque"):
        for _w in PAST_MATERIALS:
            WALK_CASES[f"material {_w} {_l} {_s}"] = (lambda sm, lst=_l, w=_w, soft=_soft: past_material_roof(lst, w, soft))
    WALK_CASES[f"light zero {_s}"] = (lambda sm, soft=_soft: edge_light("zero", soft))
WALK_CASES["light two equal largest hard"] = (lambda sm: edge_light("two equal largest", False))
