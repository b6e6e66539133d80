"""Scene ingestion (toyrenderer_amd/gltf_lite.py) and BASELINE.json configs[0]: "cornell.gltf (~1k meshlets) scalar
C++ frustum+cone cull on CPU -- plumbing + bit-exact ref, no GPU".  The reference's asset cannot travel, so the test
runs on tests/golden/cornell_scene.npz (the scene DERIVED from it by tests/golden/make_cornell.py, in the path's wire
formats, plus the oracle's outputs) and re-derives the fixture's scene from the fixture's own geometry through the
loader.  The meshlet partition / bounds are this build's own (meshoptimizer absent): parity with the reference itself
is unpinned."""
import json
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from suite_support import cornell_fixture, cpu_cull  # noqa: E402
from toyrenderer_amd import gltf_lite  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402


@pytest.mark.parametrize("flags", [5, 7])
def test_cornell_cpu_cull_matches_fixture(oracle, flags):
    z, scene, camera = cornell_fixture()
    assert len(scene.instances) == 3 and 3 <= len(scene.meshlets) <= 4, "cornell: 3 primitives, 3-4 meshlets"
    view = gltf_lite.view_of(camera, (1920, 1080))
    inst, ref = cpu_cull(oracle, scene, view, flags)
    assert np.array_equal(inst["m_WorldMatrix"], z[f"world_{flags}"]), "node transforms -> world matrices"
    # node 0 of the asset is rotated by 90 degrees about x (quaternion (0.7071069, 0, 0, 0.7071066))
    assert abs(float(inst["m_WorldMatrix"][0][1][2]) - 1.0) < 1e-5 and abs(float(inst["m_WorldMatrix"][0][2][1]) + 1.0) < 1e-5
    for s in (0, 1):
        if f"f{flags}_s{s}_records" not in z.files:
            assert not ref.passRan[s] or len(ref.records[s]) == 0
            continue
        assert np.array_equal(ref.records[s].view(np.uint32).reshape(-1, 3), z[f"f{flags}_s{s}_records"])
        assert np.array_equal(ref.visMask[s], z[f"f{flags}_s{s}_visMask"])
        assert np.array_equal(ref.visibleList[s], z[f"f{flags}_s{s}_visibleList"])
    # the open side of the box faces the camera at (0, 1, 5): every primitive is submitted, nothing is cone-culled away entirely
    assert int(ref.dispatchArgs[0][0]) == 3 and int(ref.drawArgs[0][0]) >= 3


def _write_gltf_of_fixture(tmp_path, scene, camera):
    """The fixture's scene written back as a .gltf + .bin laid out as the asset is: per primitive
    POSITION, NORMAL (unpacked from R10G10B10A2), TEXCOORD_0 (the loader ignores it; zeros) and uint16 indices, an index
    accessor shared by primitives with equal index lists, the camera on the mesh-less node that carries its pose, and any
    other mesh-less node as a KHR_lights_punctual light.  A primitive's index list is the triangles of its LOD-0 meshlets
    in order: build_meshlets partitions greedily in index order, so its meshlets concatenate back to the list it was
    given.  Returns the path and the per-primitive (vertex count, index count)."""
    blob, views, accessors, shared, counts = bytearray(), [], [], {}, []

    def accessor(a, component, kind):
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": a.nbytes})
        accessors.append({"bufferView": len(views) - 1, "componentType": component, "count": len(a), "type": kind})
        blob.extend(a.tobytes())
        return len(accessors) - 1

    bases = scene.meshData["m_GlobalVertexBufferIdx"].astype(np.int64)
    ends = np.append(bases[1:], len(scene.vertices))
    mask = set(scene.alphaMaskIds.tolist())
    prims = []
    for k, (md, base, end) in enumerate(zip(scene.meshData, bases, ends)):
        v = scene.vertices[base:end]
        pn = v["m_PackedNormal"].astype(np.uint32)
        q = np.stack([(pn >> 20) & 0x3FF, (pn >> 10) & 0x3FF, pn & 0x3FF], 1).astype(np.float32)
        tris = []
        first, count = int(md["m_MeshLODDatas"]["m_MeshletDataBufferIdx"][0]), int(md["m_MeshLODDatas"]["m_NumMeshlets"][0])
        for m in scene.meshlets[first:first + count]:
            nv, nt = int(m["m_VertexAndTriangleCount"]) & 0xFF, int(m["m_VertexAndTriangleCount"]) >> 8
            vids = scene.meshletVertexIds[int(m["m_MeshletVertexIDsBufferIdx"]):][:nv].astype(np.int64) - base
            packed = scene.meshletTriangles[int(m["m_MeshletIndexIDsBufferIdx"]):][:nt]
            tris.append(vids[np.stack([packed & 0xFF, (packed >> 8) & 0xFF, (packed >> 16) & 0xFF], 1)])
        idx = np.concatenate(tris).reshape(-1).astype(np.uint16)
        attrs = {"POSITION": accessor(np.ascontiguousarray(v["m_Position"]), 5126, "VEC3"),
                 "NORMAL": accessor(q / np.float32(1023.0) * np.float32(2.0) - np.float32(1.0), 5126, "VEC3"),
                 "TEXCOORD_0": accessor(np.zeros((len(v), 2), np.float32), 5126, "VEC2")}
        if idx.tobytes() not in shared:
            shared[idx.tobytes()] = accessor(idx, 5123, "SCALAR")
        prims.append({"attributes": attrs, "indices": shared[idx.tobytes()], "material": int(k in mask)})
        counts.append((len(v), len(idx)))
    nodes, meshes = [], []
    for i, n in enumerate(scene.nodes):
        node = {"translation": n["m_Position"].tolist(), "rotation": n["m_Rotation"].tolist(), "scale": n["m_Scale"].tolist(),
                "children": np.flatnonzero(scene.nodes["m_ParentNodeIdx"] == i).tolist()}
        mine = [prims[int(scene.instances["m_MeshDataIdx"][p])] for p in np.flatnonzero(scene.primToNode == i)]
        if mine:
            node["mesh"] = len(meshes)
            meshes.append({"primitives": mine})
        elif (n["m_Position"].tolist() == list(np.float32(camera.position)) and n["m_Rotation"].tolist() == list(np.float32(camera.orientation))
              and not any("camera" in m for m in nodes)):
            node["camera"] = 0
        else:
            node["extensions"] = {"KHR_lights_punctual": {"light": 0}}
        nodes.append(node)
    g = {"asset": {"version": "2.0"}, "extensionsUsed": ["KHR_lights_punctual"],
         "extensions": {"KHR_lights_punctual": {"lights": [{"type": "directional"}]}}, "scene": 0,
         "scenes": [{"nodes": [i for i, n in enumerate(scene.nodes) if n["m_ParentNodeIdx"] == 0xFFFFFFFF]}], "nodes": nodes,
         "cameras": [{"type": "perspective", "perspective": {"yfov": camera.yfov, "znear": camera.znear, "aspectRatio": camera.aspect}}],
         "materials": [{"alphaMode": "OPAQUE"}, {"alphaMode": "MASK"}], "meshes": meshes,
         "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(blob), "uri": "cornell.bin"}]}
    (tmp_path / "cornell.bin").write_bytes(bytes(blob))
    (tmp_path / "cornell.gltf").write_text(json.dumps(g))
    return str(tmp_path / "cornell.gltf"), counts


def test_fixture_is_what_the_loader_derives_from_its_geometry(tmp_path):
    z, scene, camera = cornell_fixture()
    path, counts = _write_gltf_of_fixture(tmp_path, scene, camera)
    # the fixture against the asset as SURVEY.md section 4 describes it: one mesh of 3 primitives with 74 / 4 / 4 vertices and
    # 90 / 6 / 6 indices in a 2 816-byte buffer, node 0 rotated by (0.7071069, 0, 0, 0.7071066)
    assert counts == [(74, 90), (4, 6), (4, 6)] and os.path.getsize(tmp_path / "cornell.bin") == 2816
    assert np.allclose(scene.nodes["m_Rotation"][0], (0.7071069, 0, 0, 0.7071066), atol=1e-7)
    fresh = gltf_lite.load(path)
    for name in ("instances", "meshData", "meshlets", "nodes", "vertices", "meshletVertexIds", "meshletTriangles"):
        assert getattr(fresh, name).tobytes() == getattr(scene, name).tobytes(), name
    assert np.array_equal(fresh.opaqueIds, scene.opaqueIds) and np.array_equal(fresh.primToNode, scene.primToNode)
    assert len(fresh.alphaMaskIds) == 0 and len(fresh.cameras) == 1
    c = fresh.cameras[0]
    assert (c.position, c.orientation, c.yfov, c.znear, c.aspect) == (camera.position, camera.orientation, camera.yfov, camera.znear, camera.aspect)
    assert c.position == (0.0, 1.0, 5.0) and abs(c.yfov - 0.3995965) < 1e-6 and abs(c.znear - 0.1) < 1e-7


def _write_gltf(tmp_path):
    """A generated two-node scene: a 12x12-vertex wavy grid (144 vertices -> several meshlets) under a rotated,
    scaled parent, and a masked single triangle on a child node."""
    n = 12
    xs, ys = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n))
    grid = np.stack([xs, ys, 0.1 * np.sin(3 * xs) * np.cos(2 * ys)], -1).reshape(-1, 3).astype(np.float32)
    idx = []
    for y in range(n - 1):
        for x in range(n - 1):
            a = y * n + x
            idx += [a, a + 1, a + n, a + 1, a + n + 1, a + n]
    idx = np.array(idx, np.uint16)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    blob = grid.tobytes() + idx.tobytes() + tri.tobytes()
    o1, o2 = len(grid.tobytes()), len(grid.tobytes()) + len(idx.tobytes())
    g = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}],
         "nodes": [{"mesh": 0, "children": [1], "rotation": [0, 0.38268343, 0, 0.92387953], "scale": [2, 2, 2], "translation": [0, 0, -10]},
                   {"mesh": 1, "translation": [1, 0, 0]}, {"camera": 0, "translation": [0, 0, 3]}],
         "cameras": [{"type": "perspective", "perspective": {"yfov": 0.8, "znear": 0.1, "aspectRatio": 1.5}}],
         "materials": [{"name": "opaque"}, {"name": "cutout", "alphaMode": "MASK"}],
         "meshes": [{"primitives": [{"attributes": {"POSITION": 0}, "indices": 1, "material": 0}]},
                    {"primitives": [{"attributes": {"POSITION": 2}, "material": 1}]}],
         "accessors": [{"bufferView": 0, "componentType": 5126, "count": len(grid), "type": "VEC3"},
                       {"bufferView": 1, "componentType": 5123, "count": len(idx), "type": "SCALAR"},
                       {"bufferView": 2, "componentType": 5126, "count": 3, "type": "VEC3"}],
         "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": o1}, {"buffer": 0, "byteOffset": o1, "byteLength": o2 - o1},
                         {"buffer": 0, "byteOffset": o2, "byteLength": len(tri.tobytes())}],
         "buffers": [{"byteLength": len(blob), "uri": "scene.bin"}]}
    (tmp_path / "scene.bin").write_bytes(blob)
    (tmp_path / "scene.gltf").write_text(json.dumps(g))
    return str(tmp_path / "scene.gltf"), grid, idx.reshape(-1, 3), tri


def test_loader_invariants_on_a_generated_file(tmp_path, oracle):
    path, grid, tris, tri = _write_gltf(tmp_path)
    s = gltf_lite.load(path)
    assert len(s.instances) == 2 and s.opaqueIds.tolist() == [0] and s.alphaMaskIds.tolist() == [1]
    assert s.primToNode.tolist() == [0, 1] and int(s.nodes[1]["m_ParentNodeIdx"]) == 0 and int(s.nodes[0]["m_ParentNodeIdx"]) == 0xFFFFFFFF
    md = s.meshData[0]
    n0 = int(md["m_MeshLODDatas"]["m_NumMeshlets"][0])
    assert 2 <= int(md["m_NumLODs"]) <= 8 and n0 >= 3 and int(s.meshData[1]["m_MeshLODDatas"]["m_NumMeshlets"][0]) == 1
    assert int(s.meshData[1]["m_NumLODs"]) == 1, "a single triangle pair cannot be simplified: one LOD (Visual.cpp:475-479)"
    covered = []
    for m in s.meshlets[:n0]:
        nv, nt = int(m["m_VertexAndTriangleCount"]) & 0xFF, int(m["m_VertexAndTriangleCount"]) >> 8
        assert 1 <= nv <= gltf_lite.MAX_MESHLET_VERTICES and 1 <= nt <= gltf_lite.MAX_MESHLET_TRIANGLES
        vids = s.meshletVertexIds[int(m["m_MeshletVertexIDsBufferIdx"]):][:nv]
        packed = s.meshletTriangles[int(m["m_MeshletIndexIDsBufferIdx"]):][:nt]
        local = np.stack([packed & 0xFF, (packed >> 8) & 0xFF, (packed >> 16) & 0xFF], 1)
        assert local.max() < nv
        covered.append(vids[local])
        c, r = m["m_BoundingSphere"][:3], float(m["m_BoundingSphere"][3])
        assert np.all(np.linalg.norm(grid[vids] - c, axis=1) <= r * (1 + 1e-5) + 1e-6), "meshlet vertices inside the bounding sphere"
        # the packed cone contains every triangle normal (decode as the shader does: basepass.hlsl:92-105)
        pk = int(m["m_ConeAxisAndCutoff"])
        axis = np.array([(pk & 0xFF), (pk >> 8) & 0xFF, (pk >> 16) & 0xFF], np.float64) / 255.0 * 2 - 1
        cutoff = (pk >> 24) / 255.0
        if cutoff < 1.0 and np.linalg.norm(axis) > 0:
            p = grid[vids].astype(np.float64)
            nrm = np.cross(p[local[:, 1]] - p[local[:, 0]], p[local[:, 2]] - p[local[:, 0]])
            nrm /= np.linalg.norm(nrm, axis=1)[:, None]
            ax = axis / np.linalg.norm(axis)
            assert np.all(nrm @ ax >= np.sqrt(max(0.0, 1 - cutoff * cutoff)) - 0.03), "triangle normals inside the cone"
    got = np.sort(np.sort(np.concatenate(covered), axis=1), axis=0)
    assert np.array_equal(got, np.sort(np.sort(tris.astype(np.uint32), axis=1), axis=0)), "every triangle in exactly one meshlet"
    assert np.all(np.linalg.norm(grid - md["m_BoundingSphere"][:3], axis=1) <= float(md["m_BoundingSphere"][3]) * (1 + 1e-5))
    # the camera sits on node 2 and the whole thing culls through the oracle (world matrices from the node chain)
    cam = s.cameras[0]
    assert cam.position == (0.0, 0.0, 3.0) and abs(cam.aspect - 1.5) < 1e-9
    view = gltf_lite.view_of(cam, (1200, 800))
    inst, ref = cpu_cull(oracle, s, view, 5)
    assert np.allclose(inst["m_WorldMatrix"][1][3][:3], [np.sqrt(2.0), 0.0, -10 - np.sqrt(2.0)], atol=1e-5), "child = parent TRS applied to (1,0,0)"
    lod = int(ref.records[0].view(I.MeshletAmplificationData)["m_MeshLOD"][0])     # the LOD the oracle selected for the grid at this distance
    n_lod = int(md["m_MeshLODDatas"]["m_NumMeshlets"][lod])
    assert ref.passRan[0] and ref.passRan[2] and int(ref.dispatchArgs[0][0]) == (n_lod + 31) // 32 and int(ref.dispatchArgs[2][0]) == 1
    assert 0 < int(ref.drawArgs[0][0]) <= n_lod


def test_lod_chain_contract(tmp_path):
    """Mesh::Initialize's LOD loop (Visual.cpp:326-491) with this build's own simplifier: <= 8 LODs, every LOD at most 85 %
    of the previous one's indices, m_Error starts at 0 and never decreases (each step at least 1.5x the previous error,
    :488), every LOD's meshlets partition exactly that LOD's triangles, uses only the mesh's own vertices and stays
    within the relative error bound 0.1 of the original surface (measured: vertices of LOD 0 against the LOD's
    triangles' planes is not needed -- a collapse keeps a subset of the vertices, so the bound is on the moved ones)."""
    from scene_gen import _grid, _sphere
    for pos, idx in (_sphere(16, 10), _grid(24, 0.05), _grid(2, 0.0)):
        idx = idx.astype(np.uint32)
        chain = gltf_lite.build_lod_chain(pos, idx)
        assert 1 <= len(chain) <= 8 and np.array_equal(chain[0][0], idx) and chain[0][1] == 0.0
        scale = gltf_lite.simplify_scale(pos)
        for k in range(1, len(chain)):
            (pi, pe), (ci, ce) = chain[k - 1], chain[k]
            f65, f85 = float(np.float32(0.65)), float(np.float32(0.85))     # the reference's float constants (Visual.cpp:337-338)
            assert len(ci) % 3 == 0 and 0 < len(ci) < int(len(pi) * f85), "kMinIndexReductionPercentage"
            assert len(ci) > (int(len(pi) * f65) // 3) * 3 - 6, "stops as soon as the target index count is reached (a collapse removes two triangles)"
            assert ce >= pe * 1.5 - 1e-7 and ce > 0 and ce <= 0.1 * scale * 1.5 ** 8
            assert ci.max() < len(pos) and set(np.unique(ci)) <= set(np.unique(idx)), "a LOD draws a subset of the mesh's vertices"
            t = ci.reshape(-1, 3)
            assert np.all((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])), "no degenerate triangles"
        if len(idx) == 6:
            assert len(chain) == 1
        else:
            assert len(chain) >= 3
    # KAT of the target index count (Visual.cpp:454: double(size) * 0.65f, truncated, rounded down to whole triangles): the
    # reference's constant is a FLOAT, 0.65f = 0.64999997615..., so 60 indices ask for 36, not 39
    asked = []
    def spy(positions, indices, target, err):
        asked.append((len(indices), target))
        return indices, 0.0                                      # "no reduction": the chain stops after one request
    for n, want in ((60, 36), (120, 75), (6000, 3897), (300, 192)):
        gltf_lite.build_lod_chain(np.zeros((n, 3), np.float32) + np.arange(n)[:, None], np.arange(n, dtype=np.uint32), simplifier=spy)
        assert asked[-1] == (n, want), asked[-1]
    # the simplifier alone: stops at the error bound when asked for more than the bound allows
    pos, idx = _sphere(16, 10)
    few, err = gltf_lite.simplify(pos, idx.astype(np.uint32), 30, 0.01)
    assert err <= 0.01 and len(few) > 30
    same, err0 = gltf_lite.simplify(pos, idx.astype(np.uint32), len(idx), 0.1)
    assert np.array_equal(same, idx.astype(np.uint32)) and err0 == 0.0


def test_loaded_scene_carries_the_lod_chain(tmp_path, oracle):
    """Generated city scene: the LODs land in MeshData (ranges, errors) and in the meshlet / geometry buffers; every LOD's
    meshlets cover exactly its triangles; the oracle's LOD selection (gpuculling.hlsl:39-57) picks coarser LODs for the
    far spheres than for the near ones."""
    from scene_gen import write_city_gltf
    s = gltf_lite.load(write_city_gltf(tmp_path))
    sphere = s.meshData[1]
    nl = int(sphere["m_NumLODs"])
    assert nl >= 3
    lods = sphere["m_MeshLODDatas"]
    errs = lods["m_Error"][:nl]
    assert errs[0] == 0 and np.all(np.diff(errs) > 0)
    counts = lods["m_NumMeshlets"][:nl].astype(np.int64)
    bases = lods["m_MeshletDataBufferIdx"][:nl].astype(np.int64)
    assert np.all(np.diff(bases) == counts[:-1]), "LOD meshlet ranges are consecutive (Visual.cpp:344)"
    assert counts[-1] < counts[0]
    tri_counts = []
    for k in range(nl):
        n_t = 0
        for m in s.meshlets[bases[k]:bases[k] + counts[k]]:
            nv, nt = int(m["m_VertexAndTriangleCount"]) & 0xFF, int(m["m_VertexAndTriangleCount"]) >> 8
            packed = s.meshletTriangles[int(m["m_MeshletIndexIDsBufferIdx"]):][:nt]
            assert max((packed & 0xFF).max(), ((packed >> 8) & 0xFF).max(), ((packed >> 16) & 0xFF).max()) < nv
            n_t += nt
        tri_counts.append(n_t)
    assert all(b < a * 0.85 for a, b in zip(tri_counts, tri_counts[1:]))
    view = gltf_lite.view_of(s.cameras[0], (1280, 720))
    inst, ref = cpu_cull(oracle, s, view, 1)
    rec = ref.records[0].view(I.MeshletAmplificationData)
    sphere_rec = rec[s.instances["m_MeshDataIdx"][rec["m_InstanceConstIdx"]] == 1]
    assert len(np.unique(sphere_rec["m_MeshLOD"])) >= 2, "near and far spheres use different LODs"
    z = -inst["m_WorldMatrix"][sphere_rec["m_InstanceConstIdx"], 3, 2]
    near, far = sphere_rec["m_MeshLOD"][z < np.percentile(z, 25)], sphere_rec["m_MeshLOD"][z > np.percentile(z, 75)]
    assert far.mean() > near.mean()
