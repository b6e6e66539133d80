"""Scenes for the visibility-buffer tests (tests/test_visibility_ref.py, tests/test_gpu_visibility.py)."""
import numpy as np

from toyrenderer_amd import gltf_lite, synth
from toyrenderer_amd import interop as I


def consts(view, prev_world_to_view=None):
    """BasePassConstants of the raster and the motion resolve: m_WorldToClip, m_PrevWorldToClip (from the view's
    prevWorldToView unless given), m_NearPlane, m_OutputResolution."""
    k = np.zeros(1, I.BasePassConstants)
    k["m_WorldToClip"] = I.world_to_clip(view.worldToView, view.viewToClip)
    prev = view.prevWorldToView if prev_world_to_view is None else prev_world_to_view
    k["m_PrevWorldToClip"] = I.world_to_clip(prev, view.viewToClip)
    k["m_NearPlane"] = view.nearPlane
    k["m_OutputResolution"] = (view.renderW, view.renderH)
    return k


def city(tmp_path, oracle, lods=True):
    from scene_gen import write_city_gltf
    s = gltf_lite.load(write_city_gltf(tmp_path), lods=lods)
    inst = s.instances.copy()
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]                 # static instances
    sc = dict(s.as_oracle()); sc["instances"] = inst
    return s, sc


def hostile_soup(seed: int, n_meshlets: int = 40):
    """Random meshlets whose vertices include points behind the camera, on the near plane, far off screen, at 1e30,
    infinities and NaNs, coincident vertices (degenerate triangles) and indices past the vertex count; some meshlets
    carry more than 128 triangles (out of contract: depth only).  Two instances, 4 records.
    Returns (scene dict, vertices, vertex ids, triangles, records, visible list)."""
    rng = np.random.default_rng(seed)
    verts, vids, tris, meshlets = [], [], [], np.zeros(n_meshlets, I.MeshletData)
    for m in range(n_meshlets):
        nv = int(rng.integers(3, 65))
        nt = int(rng.integers(129, 200)) if m % 7 == 3 else int(rng.integers(1, 97))
        base = len(verts)
        p = np.stack([rng.uniform(-6, 6, nv), rng.uniform(-4, 4, nv), rng.uniform(-30, 2, nv)], 1)
        kind = rng.integers(0, 12, nv)
        p[kind == 0] *= 1e30
        p[kind == 1, 2] = -0.1
        p[kind == 2, 0] = np.inf
        p[kind == 3, 1] = np.nan
        p[kind == 4] = p[0]
        verts += [tuple(x) for x in p.astype(np.float32)]
        meshlets[m]["m_MeshletVertexIDsBufferIdx"] = len(vids)
        vids += list(range(base, base + nv))
        meshlets[m]["m_MeshletIndexIDsBufferIdx"] = len(tris)
        hi = nv + (4 if m % 5 == 0 else 0)
        idx = rng.integers(0, hi, (nt, 3))
        tris += [int(a | (b << 8) | (c << 16)) for a, b, c in idx]
        meshlets[m]["m_VertexAndTriangleCount"] = nv | (nt << 8)
    v = np.zeros(len(verts), I.RawVertexFormat)
    v["m_Position"] = np.array(verts, np.float32)
    inst = np.zeros(2, I.BasePassInstanceConstants)
    inst["m_WorldMatrix"][0] = np.eye(4, dtype=np.float32)
    inst["m_WorldMatrix"][1] = np.diag([0.5, 2.0, 1.0, 1.0]).astype(np.float32)
    inst["m_WorldMatrix"][1][3, :3] = (1.0, -0.5, -3.0)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    inst["m_PrevWorldMatrix"][1][3, :3] = (1.25, -0.5, -3.0)
    md = np.zeros(1, I.MeshData)
    md["m_NumLODs"] = 1
    md["m_MeshLODDatas"]["m_NumMeshlets"][0][0] = n_meshlets
    rec = np.zeros(4, I.MeshletAmplificationData)
    rec["m_InstanceConstIdx"] = [0, 0, 1, 1]
    rec["m_MeshletGroupOffset"] = [0, 32, 0, 32]
    lst = np.array([(g << 5) | lane for g in range(4) for lane in range(32 if g % 2 == 0 else n_meshlets - 32)], np.uint32)
    lst = rng.permutation(lst)
    return dict(instances=inst, meshData=md, meshlets=meshlets), v, np.array(vids, np.uint32), np.array(tris, np.uint32), rec, lst


def inside_view(cam, render=(640, 360)):
    """The city camera moved inside the wall and turned: triangles cross the near plane."""
    P = synth.perspective_rh_reverse_z_infinite(cam.yfov, render[0] / render[1], cam.znear)
    V = synth.world_to_view((0.3, 0.0, -8.02), (0.0, float(np.sin(0.4)), 0.0, float(np.cos(0.4))))
    Vp = synth.world_to_view((0.35, 0.02, -8.0), (0.0, float(np.sin(0.41)), 0.0, float(np.cos(0.41))))
    return synth.View(V, Vp, P, float(np.float32(cam.znear)), *render)


def with_duplicates(s, sc, count):
    """The scene dict with instances 0..count-1 appended again (identical matrices: exact depth ties) and the records +
    visible list that draw every LOD-0 meshlet of every instance.  Returns (scene dict, records, list, original count)."""
    from types import SimpleNamespace

    from scene_gen import all_meshlets_visible
    inst = np.concatenate([sc["instances"], sc["instances"][:count]])
    sc = dict(sc); sc["instances"] = inst
    rec, lst = all_meshlets_visible(SimpleNamespace(instances=inst, meshData=s.meshData))
    return sc, rec, lst, len(inst) - count
