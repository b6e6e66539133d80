"""What the test modules share: the device and reference-library fixtures, the word-for-word comparison, the Cornell and city
scenes, and the helpers that compare or restate a whole frame.  A test module takes what it needs from here by name, as a
top-level module after its sys.path.insert (never as tests.suite_support: the fixtures and caches must exist once), and never
from another test module.  The compile helpers are in tests/ref_build.py.

This is not a test module, so pytest does not rewrite its asserts: every assert here says what it compared."""
import contextlib
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import alpha_test_ref as AT  # noqa: E402
import bloom_ref as BR  # noqa: E402
import ddgi_ref as DG  # noqa: E402
import gbuffer_ref as GR  # noqa: E402
import gtao_ref as GT  # noqa: E402
import lighting_ref as LR  # noqa: E402
import material_textures_ref as MT  # noqa: E402
import postprocess_ref as PR  # noqa: E402
import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SM  # noqa: E402
import sky_ref as SK  # noqa: E402
import visibility_ref as VR  # noqa: E402
from gbuffer_scenes import with_normals_and_materials  # noqa: E402
from toyrenderer_amd import gltf_lite, synth  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402
from visibility_scenes import city, consts  # noqa: E402

F = np.float32
GOLDEN = os.path.join(HERE, "golden", "cornell_scene.npz")
# the launchers libtrhip_probe.so exports (csrc/probe.hip), the last one without a device
PROBE_LAUNCHERS = ["probe_unary", "probe_div2", "probe_quotient", "probe_levels", "probe_step", "probe_filtered",
                   "probe_result_size"]
# the small scene of the parity tests
SMALL = synth.SceneSpec(num_meshes=24, num_instances=300, meshlets_lod0=70, jitter_meshlets=True, max_lods=5,
                        alpha_mask_fraction=0.15, seed=1234)


# ---- fixtures: imported by name; a module-scoped fixture is set up once per importing module ------------------------------------
@pytest.fixture(scope="module")
def dev():
    from toyrenderer_amd import rhi
    d = rhi.Device(0)
    yield d
    d.destroy()


def ref_library(wrapper):
    """A module-scoped fixture of a tests/*_ref.py wrapper's library, compiled into a pytest temporary directory."""
    @pytest.fixture(scope="module")
    def library(tmp_path_factory):
        return wrapper.load(tmp_path_factory.mktemp(wrapper.__name__))
    return library


vr, gr, lr, pr, bl, sk = ref_library(VR), ref_library(GR), ref_library(LR), ref_library(PR), ref_library(BR), ref_library(SK)
gt, sm, mt, at, dg = ref_library(GT), ref_library(SM), ref_library(MT), ref_library(AT), ref_library(DG)


# ---- small helpers ----------------------------------------------------------------------------------------------------------------
def same(got, want, what):
    """Equal shapes and equal words, or the count of differing words and the first of them."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {first}: got {got[first]}, want {want[first]}")


def bits(x):
    return np.asarray(x, F).reshape(-1).view(np.uint32)


def halves_to_words(h):
    h = np.ascontiguousarray(h, np.uint16)
    return (h[..., 0].astype(np.uint32) | h[..., 1].astype(np.uint32) << 16)


def kernel_constant(source_file, name):
    """The integer a kernel file of toyrenderer_amd/csrc declares as `name = N`."""
    src = open(os.path.join(ROOT, "toyrenderer_amd", "csrc", source_file)).read()
    return int(re.search(r"\b" + name + r" = (\d+)", src).group(1))


def raster_dispatch(dev, s, texels, alpha=False, table=True, slot=1):
    """One direct dispatch of the depth (texels=False) or the visibility instantiation of the compute rasteriser on a scene of
    tests/raster_path_scenes.py into cleared textures: (depth, vis or None).  alpha: the ALPHA_MASK_MODE=1 instantiation, with
    s.materials at t3 and, unless table=False or s.textures is None, s.textures at t19 (None: an entry left empty;
    raster_path_scenes.OTHER_FORMAT: an R8_UNORM texture)."""
    from toyrenderer_amd import rhi
    from toyrenderer_amd.rhi import CB, PUSH, SRV, TEX_TABLE, TEX_UAV
    W, H = s.render
    bufs = [dev.buffer_from(s.sc["instances"], "inst", uav=False), dev.buffer_from(s.v, "v", uav=False, min_bytes=20),
            dev.buffer_from(s.sc["meshData"], "md", uav=False), dev.buffer_from(s.sc["meshlets"], "ml", uav=False, min_bytes=32),
            dev.buffer_from(s.vid, "vid", uav=False), dev.buffer_from(s.tri, "tri", uav=False), dev.buffer_from(s.rec, "rec", min_bytes=12),
            dev.buffer_from(s.lst, "lst")]
    args = dev.create_buffer(12, "drawArgs", stride=12, indirect=True)
    args.upload(np.array([len(s.lst), 1, 1], np.uint32))
    depth = dev.create_texture(W, H, 1, rhi.FORMAT_R32_FLOAT, "Depth Buffer")
    vis = dev.create_texture(W, H, 1, rhi.FORMAT_RG32_UINT, "VisibilityBuffer") if texels else None
    made, tex_table, extra = [], None, []
    cl = dev.create_command_list()
    try:
        if alpha:
            bufs.append(dev.buffer_from(np.ascontiguousarray(s.materials, I.MaterialData), "materials", uav=False, min_bytes=124))
            extra.append(SRV(3, bufs[-1]))
            if table and s.textures is not None:
                tex_table = dev.create_texture_table(max(len(s.textures), 1))
                for i, t in enumerate(s.textures):
                    if t is None:
                        continue
                    made.append(dev.create_sampled_texture(t[0], t[1], f"material texture {i}") if isinstance(t, tuple)
                                else dev.create_texture(4, 4, 1, rhi.FORMAT_R8_UNORM, "another format", uav=False))
                    tex_table.set(i, made[-1])
                extra.append(TEX_TABLE(tex_table))
        name = "basepass_MS_Main_" + ("visibility" if texels else "depth") + (" ALPHA_MASK_MODE=1" if alpha else "")
        cl.open()
        cl.clear_texture_f32(depth, 0.0)
        cb = cl.constant_buffer(s.k, "BasePassConstants")
        geo = [CB(0, cb), SRV(0, bufs[0]), SRV(1, bufs[1]), SRV(2, bufs[2]), SRV(4, bufs[3]), SRV(5, bufs[4]), SRV(6, bufs[5]), SRV(7, bufs[6]),
               SRV(9, bufs[7]), TEX_UAV(0, depth, 0)] + extra
        if texels:
            cl.clear_texture_u32(vis, 0)
            cl.dispatch_indirect(name, geo + [TEX_UAV(1, vis, 0), PUSH(1)], args, push=np.array([slot], np.uint32))
        else:
            cl.dispatch_indirect(name, geo, args)
        cl.close()
        dev.execute(cl); dev.wait_idle()
        return depth.download_mip(0), vis.download_mip(0) if texels else None
    finally:
        cl.release(); depth.release(); args.release()
        if vis is not None:
            vis.release()
        if tex_table is not None:
            tex_table.release()
        for b in bufs + made:
            b.release()


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def cornell_fixture():
    """(npz, LoadedScene, camera) of tests/golden/cornell_scene.npz."""
    z = np.load(GOLDEN)                                  # allow_pickle=False (default): plain arrays only
    cam = z["camera"]
    camera = gltf_lite.Camera("fixture", tuple(cam[0:3]), tuple(cam[3:7]), float(cam[7]), float(cam[8]), float(cam[9]))
    scene = gltf_lite.LoadedScene(z["instances"].view(I.BasePassInstanceConstants).reshape(-1), z["meshData"].view(I.MeshData).reshape(-1),
                                  z["meshlets"].view(I.MeshletData).reshape(-1), z["opaqueIds"], z["alphaMaskIds"],
                                  z["nodes"].view(I.NodeLocalTransform).reshape(-1), z["primToNode"], [camera],
                                  z["vertices"].view(I.RawVertexFormat).reshape(-1) if "vertices" in z.files else np.zeros(0, I.RawVertexFormat),
                                  z["meshletVertexIds"] if "meshletVertexIds" in z.files else np.zeros(0, np.uint32),
                                  z["meshletTriangles"] if "meshletTriangles" in z.files else np.zeros(0, np.uint32))
    return z, scene, camera


def cpu_cull(oracle, scene, view, flags):
    """(instances with world matrices, the oracle's frame) of a loaded scene under a cleared HZB."""
    inst = scene.instances.copy()
    oracle.update_instance_consts(scene.nodes, scene.primToNode, inst)
    sc = dict(scene.as_oracle()); sc["instances"] = inst
    hzb = oracle.HzbTexture(*view.hzb_dims)
    depth = np.zeros((view.renderH, view.renderW), np.float32) if flags & 2 else None
    return inst, oracle.frame(sc, view.as_dict(), hzb, depth, cullingFlags=flags, maxGroups=65535, record_capacity=65535)


def lit_cornell(oracle):
    """The Cornell fixture with the materials of tests/golden/cornell_materials.json and world matrices: (s, instances, vertices,
    materials, camera).  The light and exposure are the caller's."""
    with open(os.path.join(HERE, "golden", "cornell_materials.json")) as f:
        cm = json.load(f)
    _, s, camera = cornell_fixture()
    mats = gltf_lite.material_table([{"pbrMetallicRoughness": {"baseColorFactor": c, "metallicFactor": 0}} for c in cm["baseColorFactor"]])
    s.materials, s.primMaterial = mats, np.array(cm["primitiveMaterial"], np.uint32)
    inst = gltf_lite.apply_materials(s)
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    return s, inst, s.vertices, mats, camera


def lit_city(oracle, tmp_path):
    """The generated city with seeded normals and materials: (s, instances, vertices, materials, camera)."""
    s, sc = city(tmp_path, oracle)
    v, sc, mats = with_normals_and_materials(s, sc)
    return s, sc["instances"], v, mats, s.cameras[0]


def gpu_scene(dev, s, inst, vertices=None, materials=None):
    """A GpuScene of a loaded scene with its geometry (the scene's own vertices unless given) and, if given, materials."""
    from toyrenderer_amd.frame import GpuScene
    gs = GpuScene(dev, inst, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
    gs.set_geometry(s.vertices if vertices is None else vertices, s.meshletVertexIds, s.meshletTriangles)
    if materials is not None:
        gs.set_materials(materials)
    return gs


def bare_gpu_scene(dev, sc):
    """A GpuScene of a tests/shadow_scenes.py dict: no meshlets (the single passes need none), geometry, materials, the structure."""
    from toyrenderer_amd.frame import GpuScene
    gs = GpuScene(dev, sc["instances"], sc["meshData"], None, sc["opaqueIds"], sc["alphaMaskIds"], num_meshlets=1)
    gs.set_geometry(sc["vertices"], np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    gs.set_materials(sc["materials"])
    gs.set_raytracing(sc["indices"], sc["index_counts"])
    return gs


@contextlib.contextmanager
def host_renderer(s, instances, geometry=None, materials=None, **kw):
    """A host.Renderer(**kw) with the scene, its nodes and, if given, geometry and materials loaded; shut down on exit."""
    from toyrenderer_amd import host
    r = host.Renderer(**kw)
    try:
        r.load_scene(instances, s.meshData, s.meshlets, s.opaqueIds, s.alphaMaskIds)
        r.load_nodes(s.nodes, s.primToNode)
        if geometry is not None:
            r.load_geometry(*geometry)
        if materials is not None:
            r.load_materials(materials)
        yield r
    finally:
        r.shutdown()


# ---- frames -------------------------------------------------------------------------------------------------------------------
def oracle_hzb(oracle, view, depth):
    hw, hh = view.hzb_dims
    h = oracle.HzbTexture(hw, hh)
    if depth is not None:
        h.build_from_depth(depth)
    return h


def upload_hzb(driver, hzb):
    driver.hzb.upload_chain(hzb.texels, hzb.offsets)


def compare_frame(got, ref, slots=(0, 1, 2, 3)):
    """The cull outputs of a GPU frame against the oracle's, pass slot by pass slot."""
    for s in slots:
        if not ref.passRan[s]:
            assert got[s] is None, f"slot {s} ran on the GPU but not in the oracle"
            continue
        g = got[s]
        assert g is not None, f"slot {s} did not run on the GPU"
        assert np.array_equal(g["dispatchArgs"], ref.dispatchArgs[s]), (s, g["dispatchArgs"], ref.dispatchArgs[s])
        assert g["validRecords"] == int(ref.validRecords[s]), f"slot {s}: {g['validRecords']} valid records, the oracle has {int(ref.validRecords[s])}"
        assert np.array_equal(g["records"].view(np.uint32), ref.records[s].view(np.uint32)), f"slot {s}: records differ"
        assert np.array_equal(g["visMask"], ref.visMask[s]), f"slot {s}: visibility masks differ"
        assert np.array_equal(g["drawArgs"], ref.drawArgs[s]), (s, g["drawArgs"], ref.drawArgs[s])
        assert np.array_equal(g["visibleList"], ref.visibleList[s]), f"slot {s}: visible lists differ"


def frame_reference(oracle, vr, gr, lr, sc, geo_v, view, mats, flags, mode, lighting_consts, record_capacity=4096, **kw):
    """gr_gbuffer followed by the lighting reference, from the oracle's frame."""
    W, H = view.renderW, view.renderH
    ref = oracle.frame(sc, view.as_dict(), oracle.HzbTexture(*view.hzb_dims), np.zeros((H, W), np.float32), cullingFlags=flags,
                       record_capacity=record_capacity, raster=(I.world_to_clip(view.worldToView, view.viewToClip), *geo_v), **kw)
    k = consts(view)
    geo = VR.Geometry(sc, *geo_v)
    vis, depth = VR.frame_visibility(vr, k, geo, ref, W, H)
    g, m = GR.frame_gbuffer(gr, k, geo, ref, vis, mats, mode)
    out = LR.lighting(lr, lighting_consts, g, depth, motion=halves_to_words(VR.to_half_bits(m)))
    return ref, vis, depth, g, m, out


def post_chain_reference(pr, drv, lighting_output, luminance, bloom=None):
    """One frame of the reference chain behind LightingOutput, from the driver's own parameter structs.  Returns (back buffer,
    histogram or None, luminance, exposure or None)."""
    hk, ak, pk = drv.post_consts
    hist = exposure = None
    if hk is not None:
        hist = PR.histogram(pr, lighting_output, hk)
        luminance, exposure = PR.adapt_exposure(pr, ak, hist, luminance)
    else:
        luminance = F(pk["m_ManualExposure"][0])
    return PR.post(pr, pk, lighting_output, bloom=bloom, luminance_in=luminance), hist, luminance, exposure


def op_counts(dev, drv):
    """{op: launches} of one recorded and run frame, from the back-end profile."""
    dev.profile_reset(); dev.profile_enable(True)
    try:
        drv.record(); drv.run(); drv.results()
        return {n: c for n, (c, _) in dev.profile().items()}
    finally:
        dev.profile_enable(False)


class _Recorder:
    """A proxy of rhi.CommandList that notes (method, shader name or None) of every command in order."""
    def __init__(self, cl):
        self.cl, self.seen = cl, []

    def __getattr__(self, name):
        fn = getattr(self.cl, name)

        def call(*a, **kw):
            self.seen.append((name, a[0] if name.startswith("dispatch") else None))
            return fn(*a, **kw)
        return call


def recorded(drv, every=False):
    """The ordered (method, shader) list of the commands FrameDriver.record() issues, taken by recording once more through a
    proxy; open, close and constant_buffer are left out unless every=True."""
    cl = drv.cl
    drv.cl = _Recorder(cl)
    try:
        drv.record()
        return [c for c in drv.cl.seen if every or c[0] not in ("open", "close", "constant_buffer")]
    finally:
        drv.cl = cl


def recorded_kinds(drv):
    """Counts of every command FrameDriver.record() issues, by rhi.CommandList method (all clear_texture* as one, all dispatch* as one)."""
    counts = {}
    for name, _ in recorded(drv, every=True):
        key = "clear_texture" if name.startswith("clear_texture") else "dispatch" if name.startswith("dispatch") else name
        counts[key] = counts.get(key, 0) + 1
    return counts


_SHADOW_REF = {}


def shadow_case_reference(sm, case):
    """(scene, accel, consts, depth, gbuffer, noise, brute-force mask, linear view depth) of one case of tests/shadow_scenes.py
    CASES, computed once."""
    if case[0] not in _SHADOW_REF:
        sc, k, depth, g, noise = SS.case_inputs(case)
        acc = SM.Accel(sc)
        mask, lvd, _ = SM.trace(sm, k, acc, depth, g, noise, SM.BRUTE)
        _SHADOW_REF[case[0]] = (sc, acc, k, depth, g, noise, mask, lvd)
    return _SHADOW_REF[case[0]]


# ---- leaves that name an instance without flags -----------------------------------------------------------------------------------------------
def unflagged_leaves(sm):
    """The builder gives an instance that is in neither id list no leaf, so on a structure it built the walk's `flags == 0` rule never
    decides.  This is the structure on which it does: "attributes" built with every instance listed and refitted once, then the
    instances of ddgi_update_scenes.ATTR_UNLISTED lose their flags in the TLAS records (and in the flags brute force reads), keeping their leaves,
    boxes and object-from-world rows; a refit leaves such a record alone.  Returns (scene dict, SM.Accel with these arrays, the
    instances that lost their flags)."""
    import ddgi_update_scenes as US
    sc = US.attributes(listed=True)
    acc = SM.Accel(sc)
    nodes, records = SM.refit(sm, acc)
    off = [i for i in range(len(records)) if US.ATTR_UNLISTED(i)]
    records["flags"][off] = 0
    acc.tlas["nodes"], acc.tlas["records"] = nodes, records
    acc.flags = np.array(acc.flags, np.uint32)
    acc.flags[off] = 0
    return sc, acc, off
