"""Expected pipeline statistics (include/trhip.h, trhip_pipeline_statistics) of one frame, derived from what the CPU oracle
computed for it and from the scene arrays -- no GPU, no back-end code.

Per basepass_AS_Main pass: G = min(X, validRecords, record capacity) groups -> 32 G amplification invocations; V visible
meshlets (draw args word 0) -> 96 V mesh invocations; MS primitives = the triangle counts ((m_VertexAndTriangleCount >> 8)
& 0xFF) of the visible meshlets, each resolved through its record and the mesh's LOD table.
CS invocations: groups x [numthreads] of every counted dispatch FrameDriver.record() issues, in its order."""
import numpy as np

FIELDS = ("IAVertices", "IAPrimitives", "VSInvocations", "GSInvocations", "GSPrimitives", "CInvocations", "CPrimitives",
          "PSInvocations", "HSInvocations", "DSInvocations", "CSInvocations", "ASInvocations", "MSInvocations", "MSPrimitives")

AS_THREADS = 32          # basepass.hlsl AS_Main [numthreads(32, 1, 1)]
MS_THREADS = 96          # kMeshletShaderThreadGroupSize
CULL_THREADS = 32        # gpuculling_CS_GPUCulling
LATE_ARGS_THREADS = 1    # gpuculling_CS_BuildLateCullIndirectArgs
MINMAX_THREADS = 64      # minmaxdownsample_CS_Main [numthreads(8, 8, 1)]
SPD_THREADS = 256        # ffx_spd_downsample_pass_CS


def zeros() -> dict:
    return {f: 0 for f in FIELDS}


def triangle_counts(meshlets) -> np.ndarray:
    return ((np.asarray(meshlets["m_VertexAndTriangleCount"], np.uint64) >> 8) & 0xFF).astype(np.int64)


def pass_counts(records, vis_mask, G, visible, instances, meshData, meshlets):
    """(ASInvocations, MSInvocations, MSPrimitives) of one basepass_AS_Main pass over records[:G] with masks vis_mask[:G]
    (records: n x 3 uint32 {instance, lod, group offset}, any dtype of that layout)."""
    G = int(G)
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 3)[:G].astype(np.int64)
    mask = np.asarray(vis_mask, np.uint32)[:G].astype(np.uint64)
    bits = ((mask[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & 1).astype(bool)
    assert int(bits.sum()) == int(visible), "the masks and the draw arguments disagree"
    mesh = np.asarray(instances["m_MeshDataIdx"], np.int64)[rec[:, 0]]
    lods = meshData["m_MeshLODDatas"]["m_MeshletDataBufferIdx"].astype(np.int64)     # [mesh, lod]
    base = lods[mesh, rec[:, 1]] + rec[:, 2]
    idx = (base[:, None] + np.arange(32, dtype=np.int64)[None, :])[bits]
    tri = triangle_counts(meshlets)
    return AS_THREADS * G, MS_THREADS * int(visible), int(tri[idx].sum())


def frame_stats(ref, scene: dict, *, flags: int, record_capacity: int, hzb_dims, freeze: bool = False) -> dict:
    """What a query around FrameDriver.record()'s whole list reports for the frame the oracle computed as `ref`
    (pyoracle.frame; scene: the dict given to it)."""
    out = zeros()
    occ = bool(flags & 2)
    n_op, n_am = len(scene["opaqueIds"]), len(scene["alphaMaskIds"])
    hw, hh = hzb_dims
    cs = 0

    def culling(late, am):
        nonlocal cs
        nb = n_am if am else n_op
        if nb == 0:
            return
        if not late:
            cs += -(-nb // 32) * CULL_THREADS
            if occ:
                cs += LATE_ARGS_THREADS
        elif occ:
            x, y, z = (int(v) for v in ref.lateArgs[int(am)])
            cs += x * y * z * CULL_THREADS

    def hzb():
        nonlocal cs
        if not freeze:
            cs += -(-hw // 8) * -(-hh // 8) * MINMAX_THREADS + -(-hw // 64) * -(-hh // 64) * SPD_THREADS

    culling(False, False)
    if occ:
        hzb()
        culling(True, False)
        culling(False, True)
        culling(True, True)
        hzb()
    else:
        culling(False, True)
    out["CSInvocations"] = cs
    for s in range(4):
        if not ref.passRan[s]:
            continue
        G = min(int(ref.dispatchArgs[s][0]), int(ref.validRecords[s]), int(record_capacity))
        a, m, p = pass_counts(ref.records[s], ref.visMask[s], G, int(ref.drawArgs[s][0]), scene["instances"], scene["meshData"],
                              scene["meshlets"])
        out["ASInvocations"] += a
        out["MSInvocations"] += m
        out["MSPrimitives"] += p
    return out
