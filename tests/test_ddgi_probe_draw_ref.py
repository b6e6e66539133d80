"""The reference of the probe visualisation (tests/ddgi_probe_draw_ref.c) on its own: the unit sphere's table against both hosts',
cases small enough to check by hand, the scenes of tests/ddgi_probe_draw_scenes.py showing what they exist for, and the layout of
the constant block.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ddgi_probe_draw_ref as PD  # noqa: E402
import ddgi_probe_draw_scenes as S  # noqa: E402
from ref_build import layout_probe  # noqa: E402
from suite_support import ref_library  # noqa: E402
from toyrenderer_amd import ddgi  # noqa: E402
from toyrenderer_amd import interop as I  # noqa: E402

F = np.float32
pd = ref_library(PD)


# ---- the unit sphere ----------------------------------------------------------------------------------------------------------------------
def _areas(v, ix):
    """Twice the area vector of every triangle, float64 [156, 3]."""
    p = v["m_Normal"].astype(np.float64)[ix.reshape(-1, 3)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p.mean(1)


def test_the_sphere_table(pd):
    """91 vertices, 468 indices, 120 triangles with area; the Python host's table equals the reference library's byte for byte (the
    C++ host's: test_the_host_mirrors_table below); the sines are exact: RN(sqrt(3) / 2) is the binary32 nearest the float64 square
    root of 0.75, which IEEE rounds correctly."""
    v, ix = PD.unit_sphere(pd)
    assert len(v) == 91 == I.kUnitSphereVertices and len(ix) == 468 == I.kUnitSphereIndices and int(ix.max()) == 90
    hv, hix = ddgi.unit_sphere()
    assert hv.tobytes() == v.tobytes() and hix.tobytes() == ix.tobytes()
    cross, _ = _areas(v, ix)
    assert int(np.count_nonzero(np.abs(cross).sum(1))) == 120
    n = v["m_Normal"].reshape(7, 13, 3)
    assert float(n[4, 1, 1]) == 0.5 and n[5, 0, 1] == F(math.sqrt(0.75)) and float(n[3, 3, 0]) == 1.0
    assert np.array_equal(n[:, 12], n[:, 0]), "the seam column repeats column 0 exactly"
    assert not np.any(n[0, :, [0, 2]]) and not np.any(n[6, :, [0, 2]]), "the poles are points"
    assert np.array_equal(v["m_Position"], v["m_Normal"] * F(0.5))
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1.0).max() < 1e-7


def test_the_host_mirrors_table(pd):
    from toyrenderer_amd import host
    v, ix = PD.unit_sphere(pd)
    hv, hix = host.unit_sphere()
    assert hv.tobytes() == v.tobytes() and hix.tobytes() == ix.tobytes()


def test_every_triangle_with_area_faces_outward_under_the_stated_sign(pd):
    """In space: the right-handed area vector of (v0, v1, v2) points OUT of the sphere for all 120 (the winding as reversed).
    On the screen, through the project's camera (right-handed, looking down -Z, y flipped by the viewport): exactly those whose
    outward side faces the camera have edge(v0, v1, v2) < 0, the sign tests/ddgi_probe_draw_ref.c states."""
    v, ix = PD.unit_sphere(pd)
    cross, centre = _areas(v, ix)
    with_area = np.abs(cross).sum(1) > 0
    assert np.all((cross * centre).sum(1)[with_area] > 0)
    size = (96, 64)
    M = S.world_to_clip(size).astype(np.float64)
    world = np.array([0.0, 0.0, -3.0]) + 0.5 * v["m_Normal"].astype(np.float64)
    clip = np.c_[world, np.ones(len(world))] @ M
    sx, sy = (clip[:, 0] / clip[:, 3]) * 48 + 48, -(clip[:, 1] / clip[:, 3]) * 32 + 32
    t = ix.reshape(-1, 3)
    area = (sx[t[:, 1]] - sx[t[:, 0]]) * (sy[t[:, 2]] - sy[t[:, 0]]) - (sy[t[:, 1]] - sy[t[:, 0]]) * (sx[t[:, 2]] - sx[t[:, 0]])
    toward_camera = (cross * (np.zeros(3) - world[t].mean(1))).sum(1) > 0       # the camera is at the origin
    assert np.array_equal(area[with_area] < 0, toward_camera[with_area]) and 40 < int(np.count_nonzero(area[with_area] < 0)) < 60


# ---- by hand --------------------------------------------------------------------------------------------------------------------------------
def _hand(pd, depth):
    size = (96, 64)
    vol = S.constant_volume()
    pos, _ = PD.load_probes(pd, vol)
    assert pos.tolist() == [[0.0, 0.0, -3.0]]
    k = PD.consts(S.world_to_clip(size), 0.5, S.NEAR)
    return PD.draw(pd, k, vol, pos, [0], 1, depth, np.full((64, 96), 0x12345678, np.uint32))


def test_one_probe_of_one_colour(pd):
    """A probe straight ahead at distance 3 with radius 0.5 whose tile is one constant: every covered texel is the colour worked out
    here, the disc is the sphere's silhouette, and the depth it writes lies between the sphere's nearest point and its silhouette
    plane."""
    winners, color, depth, n = _hand(pd, np.zeros((64, 96), F))
    # the stored texel t = (rgb / (2 pi 1.0989)) ^ (1 / 5) to 10 bits; the screen shows ((t ^ 2.5) ^ 2 * 2 * 1.0989) = rgb / pi to 8
    want = 0xFF000000
    for ch, rgb in enumerate((0.5, 0.25, 0.125)):
        t = round((rgb / (2 * math.pi * 1.0989)) ** 0.2 * 1023) / 1023
        want |= int(min(max(t ** 5 * 2 * 1.0989, 0.0), 1.0) * 255 + 0.5) << (8 * ch)
    won = winners != 0
    assert n["won"] == int(won.sum()) > 400 and set(np.unique(color[won])) == {want} and want == 0xFF0A1429
    assert np.all(color[~won] == 0x12345678) and np.all(depth[~won] == 0.0)
    # the silhouette: a circle of radius r / sqrt(d^2 - r^2) in tangent units around the screen centre; P11 = 1 / tan(22.5 deg)
    radius_px = 0.5 / math.sqrt(9 - 0.25) / math.tan(math.radians(22.5)) * 32
    yy, xx = np.mgrid[0:64, 0:96]
    r = np.hypot(xx + 0.5 - 48, yy + 0.5 - 32)
    assert np.all(won[r < radius_px - 1.0]) and not np.any(won[r > radius_px + 0.5])     # the 12-gon lies inside the circle
    assert np.all(depth[won] <= F(S.NEAR / 2.5)) and np.all(depth[won] > F(S.NEAR / 3.0))
    assert n["near_dropped"] == 0 and n["back_culled"] + n["no_area"] + 56 == 156 and n["no_area"] == 36


def test_the_same_probe_behind_and_half_behind_a_plane(pd):
    free = _hand(pd, np.zeros((64, 96), F))
    plane = S.depth_plane((96, 64), 2.0)
    winners, color, depth, n = _hand(pd, plane)
    assert n["won"] == 0 and n["lost_to_scene"] == free[3]["won"] and not winners.any()
    assert np.all(color == 0x12345678) and np.array_equal(depth, plane)
    # a plane through the visible cap: the texels whose free depth is at least the plane's survive, bit for bit as before
    cut = S.depth_plane((96, 64), 2.7)
    winners, color, depth, n = _hand(pd, cut)
    keep = free[2] >= cut
    assert 0 < n["won"] == int(keep.sum()) < free[3]["won"] and n["won"] + n["lost_to_scene"] == free[3]["won"]
    assert np.array_equal(winners[keep], free[0][keep]) and not winners[~keep].any() and np.array_equal(depth[~keep], cut[~keep])


# ---- the scenes show what they are for -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(S.SCENES))
def test_a_scene_shows_its_point(pd, name, size):
    s = S.scene(name, size)
    k = PD.consts(s["world_to_clip"], s["radius"], s["near"])
    winners, color, depth, n = PD.draw(pd, k, s["vol"], s["positions"], s["to_probe"], s["count"], s["depth"], s["color"])
    missing = [c for c in s["shows"] if n[c] == 0]
    assert not missing, (name, size, missing, n)
    won = winners != 0
    assert np.array_equal(color[~won], s["color"][~won]) and np.array_equal(depth[~won], s["depth"][~won])
    assert np.all(depth[won] >= s["depth"][won]) and np.all((color[won] >> 24) == 255)
    if name == "two coincident":                                      # the later instance wins every tie
        assert n["tie"] == n["won"] and np.all(((winners[won] >> np.uint64(8)) & np.uint64(0xFFFFFF)) == 1)


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_sample_at_exactly_the_scene_depth_survives(pd, size):
    """GREATER_OR_EQUAL: over a depth buffer that already holds the sphere's own depth every winner ties the scene and survives (a
    sample that lost to another triangle through the same pixel centre before loses to the scene now)."""
    draw = lambda s: PD.draw(pd, PD.consts(s["world_to_clip"], s["radius"], s["near"]), s["vol"], s["positions"], s["to_probe"], s["count"], s["depth"], s["color"])
    free = draw(S.scene("one", size))
    winners, color, depth, n = draw(S.on_its_own_depth(draw, size))
    assert n["won"] == free[3]["won"] > 0
    assert np.array_equal(winners, free[0]) and np.array_equal(color, free[1]) and np.array_equal(depth, free[2])


def test_the_scenes_together_show_every_counter(pd):
    seen = set()
    for name in S.SCENES:
        s = S.scene(name, S.SIZES[0])
        n = PD.draw(pd, PD.consts(s["world_to_clip"], s["radius"], s["near"]), s["vol"], s["positions"], s["to_probe"], s["count"], s["depth"], s["color"])[3]
        seen |= {c for c in PD.COUNTERS if n[c]}
    assert seen == set(PD.COUNTERS)


# ---- LoadGIProbes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relocation", (False, True))
@pytest.mark.parametrize("classification", (False, True))
def test_loaded_probes(pd, relocation, classification):
    """Positions are Volume.probe_positions_and_states()'s word for word; the states are its states with classification on and all
    active with it off, where that helper goes on returning data.w."""
    vol = S.volume(counts=(3, 2, 4), relocation=relocation, classification=classification)
    pos, states = PD.load_probes(pd, vol)
    want_pos, want_states = vol.probe_positions_and_states()
    assert np.array_equal(pos.view(np.uint32), want_pos.view(np.uint32))
    assert np.any(want_states == 1.0) and np.array_equal(states, want_states if classification else np.zeros_like(want_states))


# ---- the constant block -----------------------------------------------------------------------------------------------------------------------
def test_layout_of_the_constant_block(tmp_path):
    t = "interop::GIProbeVisualizationConsts"
    got = layout_probe(tmp_path, [("size", f"sizeof({t})")] + [(f, f"offsetof({t}, {f})") for f in ("m_WorldToClip", "m_CameraDirection", "m_ProbeRadius", "m_NearPlane", "pad")]
                       + [("vertex", "sizeof(interop::UncompressedRawVertexFormat)"), ("normal", "offsetof(interop::UncompressedRawVertexFormat, m_Normal)")])
    d = I.GIProbeVisualizationConsts
    assert int(got["size"]) == d.itemsize == 96
    for f in ("m_WorldToClip", "m_CameraDirection", "m_ProbeRadius", "m_NearPlane", "pad"):
        assert int(got[f]) == d.fields[f][1], f
    assert int(got["m_ProbeRadius"]) == 76 and int(got["m_NearPlane"]) == 80, "the reference's 80 bytes come first, unchanged"
    assert int(got["vertex"]) == I.UncompressedRawVertexFormat.itemsize == 32 and int(got["normal"]) == I.UncompressedRawVertexFormat.fields["m_Normal"][1] == 12
