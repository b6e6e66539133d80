"""Scenes and textures for the material-texture tests (tests/test_material_textures_ref.py, tests/test_gpu_material_textures.py):
a handful of quads, each its own instance, mesh and meshlet, in front of synth.make_view()'s camera at 80 x 56 pixels."""
import numpy as np

from toyrenderer_amd import interop as I
from toyrenderer_amd import synth

RENDER = (80, 56)                      # not a multiple of the resolve's 16 x 16 tile
NONE = 0xFFFFFFFF
ALBEDO, NORMAL, MR, EMISSIVE = (I.MaterialFlag_UseAlbedoTexture, I.MaterialFlag_UseNormalTexture,
                                I.MaterialFlag_UseMetallicRoughnessTexture, I.MaterialFlag_UseEmissiveTexture)
SLOTS = ("m_AlbedoTexture", "m_NormalTexture", "m_MetallicRoughnessTexture", "m_EmissiveTexture")
RGBA8, SRGBA8 = 10, 11


def pack_normal(n):
    n = np.asarray(n, np.float64)
    q = np.round((n / np.linalg.norm(n) * 0.5 + 0.5) * 1023.0).astype(np.uint32)
    return int(q[0] << 20 | q[1] << 10 | q[2])


def quad(p00, p10, p01, p11, uv00, uv10, uv01, uv11, material=0, grid=1, world=None, normal=(0.0, 0.0, 1.0)):
    """A bilinear patch of grid x grid cells (2 grid^2 triangles): object-space corners, their texture coordinates, the material
    index and the instance's world matrix (row vectors; default: the identity)."""
    return dict(p=np.array([p00, p10, p01, p11], np.float64), uv=np.array([uv00, uv10, uv01, uv11], np.float64), material=material,
                grid=grid, world=np.eye(4) if world is None else np.asarray(world, np.float64), normal=normal)


def build(quads):
    """(scene dict, vertices, vertex ids, triangles, records, visible list) of the quads, one instance / mesh / meshlet each."""
    n = len(quads)
    inst, md, ml = np.zeros(n, I.BasePassInstanceConstants), np.zeros(n, I.MeshData), np.zeros(n, I.MeshletData)
    verts, vids, tris = [], [], []
    for i, q in enumerate(quads):
        g = q["grid"]
        assert (g + 1) ** 2 <= 64 and 2 * g * g <= 96
        ts = np.linspace(0.0, 1.0, g + 1)
        v = np.zeros((g + 1) ** 2, I.RawVertexFormat)
        for r, b in enumerate(ts):
            for c, a in enumerate(ts):
                wgt = np.array([(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b])
                v["m_Position"][r * (g + 1) + c] = (wgt @ q["p"]).astype(np.float32)
                v["m_TexCoord"][r * (g + 1) + c] = (wgt @ q["uv"]).astype(np.float16).view(np.uint16)
        if callable(q["normal"]):
            v["m_PackedNormal"] = [q["normal"](j) for j in range(len(v))]
        else:
            v["m_PackedNormal"] = pack_normal(q["normal"])
        t = []
        for y in range(g):
            for x in range(g):
                a = y * (g + 1) + x
                t += [a | (a + 1) << 8 | (a + g + 1) << 16, (a + 1) | (a + g + 2) << 8 | (a + g + 1) << 16]
        ml["m_VertexAndTriangleCount"][i] = len(v) | len(t) << 8
        ml["m_MeshletVertexIDsBufferIdx"][i] = len(vids)
        ml["m_MeshletIndexIDsBufferIdx"][i] = len(tris)
        vids += list(range(sum(len(x) for x in verts), sum(len(x) for x in verts) + len(v)))
        tris += t
        verts.append(v)
        inst["m_WorldMatrix"][i] = q["world"].astype(np.float32)
        inst["m_PrevWorldMatrix"][i] = q["world"].astype(np.float32)
        inst["m_MeshDataIdx"][i] = i
        inst["m_MaterialDataIdx"][i] = q["material"]
        md["m_NumLODs"][i] = 1
        md["m_MeshLODDatas"]["m_NumMeshlets"][i][0] = 1
        md["m_MeshLODDatas"]["m_MeshletDataBufferIdx"][i][0] = i
    rec = np.zeros(n, I.MeshletAmplificationData)
    rec["m_InstanceConstIdx"] = np.arange(n)
    lst = (np.arange(n, dtype=np.uint32) << 5)
    return (dict(instances=inst, meshData=md, meshlets=ml), np.concatenate(verts), np.array(vids, np.uint32), np.array(tris, np.uint32), rec, lst)


def material(flags=0, albedo=(0.9, 0.7, 0.5, 1.0), emissive=(0.0, 0.0, 0.0), indices=(NONE,) * 4, wrap=(1, 1, 1, 1)):
    m = np.zeros(1, I.MaterialData)
    m["m_ConstAlbedo"], m["m_ConstEmissive"], m["m_MaterialFlags"] = albedo, emissive, flags
    m["m_ConstRoughness"], m["m_ConstMetallic"] = 0.3, 0.6                 # never read (Q13)
    for s, d, w in zip(SLOTS, indices, wrap):
        m[s]["m_GlobalIndex"] = NONE
        m[s]["m_DescriptorIndex"] = d
        m[s]["m_IsWrapSampler"] = w
        m[s]["m_FeedbackTextureDescriptorIndex"] = NONE
        m[s]["m_MinMapTextureDescriptorIndex"] = NONE
    return m


def random_mips(seed, w, h, mips, lo=0, hi=256):
    """Independent random bytes in every level: a wrong level shows."""
    r = np.random.default_rng([seed, w, h])
    return [r.integers(lo, hi, (max(h >> k, 1), max(w >> k, 1), 4), dtype=np.uint16).astype(np.uint8) for k in range(mips)]


def normal_mips(seed, w, h, mips):
    """x, y mostly inside the unit disc; texel (0, 0) of level 0 outside it (1 - dot(xy, xy) < 0: a NaN z, kept)."""
    m = random_mips(seed, w, h, mips, 70, 186)
    m[0][0, 0, :2] = (250, 5)
    return m


def solid_mips(colours, w=8, h=8):
    """Level k all of colours[k] (r, g, b), alpha 255."""
    return [np.tile(np.array(list(c) + [255], np.uint8), (max(h >> k, 1), max(w >> k, 1), 1)) for k, c in enumerate(colours)]


def standard_textures():
    """The tests' table, as (mips, format): 0 albedo sRGB 8 x 8 x 4 mips, 1 normal 8 x 8 x 4, 2 metallic-roughness 8 x 8 x 4, 3 emissive
    sRGB 8 x 8 x 4, 4 the non-square 12 x 5 x 4 mips (UNORM), 5 a 1 x 1, 6 the albedo again as UNORM."""
    a = random_mips(1, 8, 8, 4)
    return [(a, SRGBA8), (normal_mips(2, 8, 8, 4), RGBA8), (random_mips(3, 8, 8, 4), RGBA8), (random_mips(4, 8, 8, 4), SRGBA8),
            (random_mips(5, 12, 5, 4), RGBA8), (random_mips(6, 1, 1, 1), SRGBA8), (a, RGBA8)]


def view(eye=(0.0, 0.0, 0.0), prev_eye=(0.05, -0.02, 0.1), render=RENDER):
    return synth.make_view(eye=eye, prev_eye=prev_eye, render=render)


def facing(z=-3.0, half=1.0, uv_lo=-1.5, uv_hi=2.5, material=0, grid=2, centre=(0.0, 0.0), world=None, normal=(0.3, -0.2, 1.0)):
    """A camera-facing square of side 2 * half at depth z."""
    cx, cy = centre
    return quad((cx - half, cy - half, z), (cx + half, cy - half, z), (cx - half, cy + half, z), (cx + half, cy + half, z),
                (uv_lo, uv_hi), (uv_hi, uv_hi), (uv_lo, uv_lo), (uv_hi, uv_lo), material, grid, world, normal)


def floor(material=0, repeats=12.0):
    """A floor at y = -0.6 from z = -1 to z = -40: seen at a grazing angle, the footprint's ratio runs from about 1 to far beyond 16."""
    return quad((-3.0, -0.6, -1.0), (3.0, -0.6, -1.0), (-3.0, -0.6, -40.0), (3.0, -0.6, -40.0),
                (0.0, 0.0), (3.0, 0.0), (0.0, repeats), (3.0, repeats), material, grid=6, normal=(0.0, 1.0, 0.0))


def ortho_consts(render):
    """BasePassConstants of an orthographic view with w = 1: clip.xy = world.xy, depth 0.5.  On a 64 x 64 target every quantity
    of the resolve of a quad with corners at (+-1, +-1) is a dyadic number: the derivatives are exact."""
    k = np.zeros(1, I.BasePassConstants)
    M = np.eye(4, dtype=np.float32)
    M[2, 2], M[3, 2] = 0.0, 0.5
    k["m_WorldToClip"], k["m_PrevWorldToClip"] = M, M
    k["m_NearPlane"] = 0.1
    k["m_OutputResolution"] = render
    return k


def textured_gltf():
    """(gltf dict, blobs, images): three quads in front of a camera, with NORMAL and TEXCOORD_0 (floats, UVs in [-1.5, 2.5]), two
    samplers (REPEAT, CLAMP_TO_EDGE), four textures over three images (8 x 8, 12 x 5, 1 x 1), and three materials: all four
    textures through the repeating sampler, a clamped base colour alone (the non-square image), and a texture-free one."""
    r = np.random.default_rng(11)
    images = [r.integers(0, 256, (8, 8, 4), dtype=np.uint16).astype(np.uint8), r.integers(0, 256, (5, 12, 4), dtype=np.uint16).astype(np.uint8),
              np.array([[[200, 120, 40, 255]]], np.uint8)]
    images[0][..., :2] = 70 + images[0][..., :2] % 116                      # also read as a normal map: x, y inside the unit disc
    g = 3
    ts = np.linspace(-1.0, 1.0, g + 1)
    pos = np.array([(x, y, 0.0) for y in ts for x in ts], np.float32)
    nrm = np.tile(np.array([0.2, -0.1, 0.97], np.float32) / np.float32(np.linalg.norm([0.2, -0.1, 0.97])), (len(pos), 1)).astype(np.float32)
    uv = np.array([(0.5 + 2.0 * x, 0.5 - 2.0 * y) for y in ts for x in ts], np.float32)
    idx = []
    for y in range(g):
        for x in range(g):
            a = y * (g + 1) + x
            idx += [a, a + 1, a + g + 1, a + 1, a + g + 2, a + g + 1]
    idx = np.array(idx, np.uint16)
    blob = pos.tobytes() + nrm.tobytes() + uv.tobytes() + idx.tobytes()
    o1, o2, o3 = pos.nbytes, pos.nbytes + nrm.nbytes, pos.nbytes + nrm.nbytes + uv.nbytes
    views = [{"buffer": 0, "byteOffset": 0, "byteLength": pos.nbytes}, {"buffer": 0, "byteOffset": o1, "byteLength": nrm.nbytes},
             {"buffer": 0, "byteOffset": o2, "byteLength": uv.nbytes}, {"buffer": 0, "byteOffset": o3, "byteLength": idx.nbytes}]
    accessors = [{"bufferView": 0, "componentType": 5126, "count": len(pos), "type": "VEC3", "min": pos.min(0).tolist(), "max": pos.max(0).tolist()},
                 {"bufferView": 1, "componentType": 5126, "count": len(pos), "type": "VEC3"},
                 {"bufferView": 2, "componentType": 5126, "count": len(pos), "type": "VEC2"},
                 {"bufferView": 3, "componentType": 5123, "count": len(idx), "type": "SCALAR"}]
    prim = lambda m: {"attributes": {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2}, "indices": 3, "material": m}   # noqa: E731
    materials = [{"name": "all four", "pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.8, 0.7, 1.0], "baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 1}},
                  "normalTexture": {"index": 0}, "emissiveTexture": {"index": 1}, "emissiveFactor": [1.0, 0.5, 0.25]},
                 {"name": "clamped base colour", "pbrMetallicRoughness": {"baseColorTexture": {"index": 2}}},
                 {"name": "plain", "pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.4, 0.6, 1.0]}, "emissiveFactor": [0.5, 0.5, 0.5]},
                 {"name": "one texel", "pbrMetallicRoughness": {"baseColorTexture": {"index": 3}}}]
    q = float(np.sin(0.2)), float(np.cos(0.2))
    gltf = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0, 1, 2, 3, 4]}],
            "nodes": [{"mesh": 0, "translation": [-1.1, 0.4, -4.0], "rotation": [0.0, q[0], 0.0, q[1]]},
                      {"mesh": 1, "translation": [1.2, 0.3, -4.5], "scale": [1.0, 0.8, 1.0]},
                      {"mesh": 2, "translation": [0.0, -1.3, -3.5], "rotation": [-q[0], 0.0, 0.0, q[1]]},
                      {"mesh": 3, "translation": [0.1, 1.6, -6.0], "scale": [0.6, 0.6, 1.0]},
                      {"camera": 0, "name": "camera"}],
            "cameras": [{"type": "perspective", "perspective": {"yfov": 0.8, "znear": 0.1, "aspectRatio": 80 / 56}}],
            "meshes": [{"primitives": [prim(m)]} for m in range(4)], "materials": materials,
            "samplers": [{"wrapS": 10497, "wrapT": 10497}, {"wrapS": 33071, "wrapT": 33071}],
            "textures": [{"source": 0, "sampler": 0}, {"source": 1}, {"source": 1, "sampler": 1}, {"source": 2, "sampler": 0}],
            "images": [{"uri": "a.png"}, {"uri": "b.png"}, {"uri": "c.png"}],
            "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(blob)}]}
    return gltf, [blob], images
