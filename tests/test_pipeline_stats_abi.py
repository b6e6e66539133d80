"""Pipeline statistics queries on a CPU-only box: the C ABI and the host facade export them, trhip_pipeline_statistics has
D3D12_QUERY_DATA_PIPELINE_STATISTICS1's layout on both sides of ctypes, and the numpy derivation the GPU tests compare
against (tests/pipeline_stats_ref.py) gives the right numbers on a hand-built frame."""
import ctypes
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from toyrenderer_amd import interop as I

from . import pipeline_stats_ref as psr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "toyrenderer_amd", "lib")

TRHIP_NEW = ["trhip_pipeline_stats_create", "trhip_pipeline_stats_release", "trhip_cmd_begin_pipeline_stats",
             "trhip_cmd_end_pipeline_stats", "trhip_pipeline_stats_get"]
TRHOST_NEW = ["trhost_set_pipeline_statistics", "trhost_pipeline_statistics"]


def test_back_end_and_host_library_export_the_new_symbols():
    trhip = ctypes.CDLL(os.path.join(LIB, "libtrhip.so"))
    host = ctypes.CDLL(os.path.join(LIB, "libtoyrenderer_host.so"))
    for n in TRHIP_NEW:
        assert hasattr(trhip, n), n
    for n in TRHOST_NEW:
        assert hasattr(host, n), n
    from toyrenderer_amd import host as H
    from toyrenderer_amd import rhi
    assert set(TRHIP_NEW) <= set(rhi.ABI_SYMBOLS) and set(TRHOST_NEW) <= set(H.HOST_SYMBOLS)
    assert hasattr(H.Renderer, "set_pipeline_statistics") and hasattr(H.Renderer, "pipeline_statistics")


def test_trhost_header_declares_the_facade():
    text = open(os.path.join(ROOT, "include", "trhost.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+trhost_set_pipeline_statistics\s*\(\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"int\s+trhost_pipeline_statistics\s*\(\s*trhip_pipeline_statistics\s*\*\s*\w+\s*,\s*trhip_pipeline_statistics\s*\*\s*\w+\s*\)\s*;", text)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_struct_layout_matches_ctypes(tmp_path):
    """A g++-compiled probe prints sizeof / offsetof of trhip_pipeline_statistics: 112 bytes, 14 x u64 in D3D12 order, equal to
    the ctypes structure (and to nvrhi::PipelineStatistics of the host mirror, checked by a static_assert there)."""
    from toyrenderer_amd import rhi
    src = tmp_path / "probe.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "trhip.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(trhip_pipeline_statistics));']
    for f in rhi.PIPELINE_STATISTICS_FIELDS:
        lines.append(f'    printf("{f} %zu\\n", offsetof(trhip_pipeline_statistics, {f}));')
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == 112 == ctypes.sizeof(rhi.PipelineStatistics)
    assert list(rhi.PIPELINE_STATISTICS_FIELDS) == list(psr.FIELDS)
    for i, f in enumerate(psr.FIELDS):
        assert int(out[f]) == 8 * i == getattr(rhi.PipelineStatistics, f).offset, f


def _hand_built_scene():
    """Two meshes (mesh 1 with two LODs), three instances, 100 meshlets with triangle count i % 7 + 1 for meshlet i."""
    md = np.zeros(2, I.MeshData)
    md["m_MeshLODDatas"]["m_MeshletDataBufferIdx"][0, 0] = 0
    md["m_MeshLODDatas"]["m_NumMeshlets"][0, 0] = 40
    md["m_MeshLODDatas"]["m_MeshletDataBufferIdx"][1, 0] = 40
    md["m_MeshLODDatas"]["m_NumMeshlets"][1, 0] = 50
    md["m_MeshLODDatas"]["m_MeshletDataBufferIdx"][1, 1] = 90
    md["m_MeshLODDatas"]["m_NumMeshlets"][1, 1] = 10
    inst = np.zeros(3, I.BasePassInstanceConstants)
    inst["m_MeshDataIdx"] = [1, 0, 1]
    ml = np.zeros(100, I.MeshletData)
    ml["m_VertexAndTriangleCount"] = (np.arange(100) % 7 + 1).astype(np.uint32) << 8 | 9   # vertex counts must not leak in
    return dict(instances=inst, meshData=md, meshlets=ml, opaqueIds=np.arange(3, dtype=np.uint32),
                alphaMaskIds=np.zeros(0, np.uint32))


def test_reference_helper_on_a_hand_built_frame():
    sc = _hand_built_scene()
    tri = np.arange(100) % 7 + 1
    # early opaque pass: X = 4 groups, validRecords 3 (Q2): the 4th record is undefined and not counted
    rec = np.array([[0, 0, 0], [0, 0, 32], [1, 0, 32], [2, 1, 0], [9, 9, 9]], np.uint32)
    mask = np.array([0b1011, 1 << 17, 0xFF, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    # record 0: mesh 1 LOD 0 -> meshlets 40, 41, 43; record 1: meshlet 40 + 32 + 17 = 89; record 2: mesh 0 -> 32..39
    want_tri = tri[[40, 41, 43]].sum() + tri[89] + tri[32:40].sum()
    a, m, p = psr.pass_counts(rec, mask, 3, 3 + 1 + 8, sc["instances"], sc["meshData"], sc["meshlets"])
    assert (a, m, p) == (96, 96 * 12, int(want_tri))
    ref = SimpleNamespace(passRan=np.array([1, 1, 0, 0]), dispatchArgs=np.array([[4, 1, 1], [0, 1, 1], [0, 0, 0], [0, 0, 0]]),
                          validRecords=np.array([3, 0, 0, 0]), drawArgs=np.array([[12, 1, 1], [0, 1, 1], [0, 0, 0], [0, 0, 0]]),
                          records=[rec, rec[:0], None, None], visMask=[mask, mask[:0], None, None],
                          lateArgs=np.array([[2, 1, 1], [0, 1, 1]]))
    got = psr.frame_stats(ref, sc, flags=7, record_capacity=16, hzb_dims=(64, 32))
    hzb_cs = (8 * 4 * 64 + 1 * 1 * 256) * 2                       # minmax 8 x 4 groups of 64, SPD 1 x 1 of 256, twice
    cs = 32 * 1 + 1 + 2 * 32 + hzb_cs                              # early cull (3 ids: 1 group), late args, late cull (2 groups)
    assert got == dict(psr.zeros(), CSInvocations=cs, ASInvocations=96, MSInvocations=96 * 12, MSPrimitives=int(want_tri))
    with pytest.raises(AssertionError):
        psr.pass_counts(rec, mask, 3, 11, sc["instances"], sc["meshData"], sc["meshlets"])   # draw args disagree with the masks
