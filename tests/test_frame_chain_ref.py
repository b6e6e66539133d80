"""tests/frame_chain_ref.py on its own, no GPU: the conditions under which comparing a driver with the chain means something -- in some
frame behind the first no pass of the everything-on frame is vacuous, judged on the reference's outputs alone -- and the ties between
the chain and the per-pass chains the suite already trusts.  If a condition fails, the scene or the camera changes, not the number."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import alpha_test_ref as AT  # noqa: E402
import frame_chain_ref as FC  # noqa: E402
import taa_scenes as TS  # noqa: E402
from suite_support import gr, lr, same, vr  # noqa: E402, F401

W, H = FC.RENDER
MANY = 115                                           # 5 % of the 2304 texels
assert MANY == 5 * W * H // 100


@pytest.fixture(scope="module")
def libraries(tmp_path_factory):
    return FC.Libraries(tmp_path_factory.mktemp("frame_chain"))


@pytest.fixture(scope="module")
def frames(libraries, oracle):
    return FC.run(libraries, oracle)


@pytest.fixture(scope="module")
def unjittered(libraries, oracle):
    return FC.run(libraries, oracle, off=("taa",))


def _counters(frames):
    return [f["counters"] for f in frames[1:]]


def test_no_pass_is_vacuous(frames):
    """Every condition holds in some frame behind the first (most in all of them)."""
    later = _counters(frames)
    print([f["counters"] for f in frames])

    def some(condition, what):
        assert any(condition(n) for n in later), (what, later)
    some(lambda n: n["sky_filled"] >= MANY and n["sky_filled"] == n["sky"], "the sky fills many texels, all that nothing was drawn to")
    some(lambda n: n["covered"] >= MANY, "the lit scene covers many texels")
    some(lambda n: n["alpha_slot_ran"] and n["alpha_discarded"] >= MANY and n["alpha_kept"] >= MANY, "the alpha test discards many samples and keeps many")
    some(lambda n: all(t > 0 for t in n["taps_by_texture"].values()), "a covered texel sampled each BC format")
    some(lambda n: n["floor_lit"] >= MANY and n["floor_shadowed"] >= MANY, "many lit and many shadowed floor texels")
    some(lambda n: n["behind_kept"] > 0 and n["behind_discarded"] > 0, "floor texels behind the cut-out's kept and behind its discarded texels")
    some(lambda n: n["denoised_differs"] >= MANY and n["sigma_history_reads"] > 0 and n["sigma_history_texels"] > 0, "the denoiser changes many texels and reads its history")
    some(lambda n: n["ssao_below_255"] >= MANY, "SSAO darkens many texels")
    some(lambda n: n["irradiance_changed"] > 0, "the irradiance changes")
    some(lambda n: n["probes_moved"] > 0 or n["probes_switched"] > 0, "a probe moves or changes state")
    some(lambda n: not n["ddgi_skipped"] and n["reduction_passes"] >= 1, "the variability reduction runs")
    some(lambda n: n["taa_differs"] >= MANY and n["taa_valid"] >= MANY, "the resolve changes many texels, with valid history")
    some(lambda n: n["bloom_mip0_nonzero"] > 0, "bloom mip 0 is not black")
    some(lambda n: n["luminance"] != 1.0, "the luminance adapts")
    some(lambda n: n["probes_won"] > 0 and n["probes_lost_to_scene"] > 0, "probe spheres in front of and behind the scene")
    some(lambda n: n["box_motion"] > 0, "the moved box has motion")
    assert not any(f["counters"]["ddgi_skipped"] for f in frames), "the update does not stop within three frames"
    assert frames[0]["counters"]["sigma_history_reads"] == 0 and frames[0]["counters"]["taa_valid"] == 0, "the first frame resets both histories"
    assert frames[1]["counters"]["box_motion"] == frames[1]["counters"]["box_texels"] > 0, "frame 1: the box moved under every one of its texels"


def test_the_frames_differ_from_each_other(frames):
    """The camera moves, the box moves, the volume fills: nothing that is compared stays what it was, so a driver that replays a
    frame, or reads last frame's texture, shows."""
    for a, b in ((0, 1), (1, 2)):
        for name in ("depth", "vis", "gbuffer", "motion", "ssao", "penumbra", "shadow_mask", "shadow_history", "lighting_output", "anti_aliased_output", "taa_history",
                     "back_buffer", "hzb", "probe_winners"):
            assert np.count_nonzero(np.asarray(frames[a][name]) != np.asarray(frames[b][name])) > 0, (a, b, name)
        assert np.any(frames[a]["volume"].irradiance != frames[b]["volume"].irradiance) or np.any(frames[a]["volume"].data != frames[b]["volume"].data), (a, b, "the volume")
    assert frames[1]["prev_world_to_clip"].tobytes() == frames[0]["world_to_clip"].tobytes() and frames[2]["prev_world_to_clip"].tobytes() == frames[1]["world_to_clip"].tobytes()
    assert np.array_equal(frames[2]["instances"]["m_PrevWorldMatrix"], frames[1]["instances"]["m_WorldMatrix"])
    assert not np.array_equal(frames[1]["instances"]["m_PrevWorldMatrix"], frames[1]["instances"]["m_WorldMatrix"])


JITTERED_BLOCKS = ("basepass_consts", "shadow_consts", "sigma_consts", "lighting_consts", "sky_consts", "probe_cull_consts", "probe_draw_consts", "taa_consts")


def test_every_jittered_block_differs_from_its_unjittered_twin(frames, unjittered):
    """The same frames without TAA: every block that carries a matrix, or a constant derived from the projection, differs, so a
    driver that builds one of them from the unjittered view cannot equal the chain.  The one exception is a fact about the
    reference, pinned here: GTAOUpdateConstants (XeGTAO.h:164-198) reads m_ViewToClip's [0][0], [1][1], [2][2] and [3][2] only, and
    the pixel offset matrix (Scene.cpp:129-130) changes [2][0] and [2][1] only, so GTAOConstants is the same block with and without
    jitter; what the jitter changes for AO is its inputs, the depth and the normals."""
    for f in range(FC.FRAMES):
        assert frames[f]["gtao_consts"].tobytes() == unjittered[f]["gtao_consts"].tobytes(), f
        P, Q = frames[f]["view"].viewToClip, unjittered[f]["view"].viewToClip
        changed = {(int(r), int(c)) for r, c in zip(*np.nonzero(P != Q))}
        assert changed and changed <= {(2, 0), (2, 1)}, ("the jitter's two elements (frame 0's x offset is 0)", changed)
        assert np.count_nonzero(frames[f]["ssao"] != unjittered[f]["ssao"]) > 0, f
        for name in JITTERED_BLOCKS:
            if name == "taa_consts":
                assert name not in unjittered[f] and (f == 0 or np.any(frames[f][name]["m_JitterDelta"] != 0)), (f, name)
                continue
            assert frames[f][name].tobytes() != unjittered[f][name].tobytes(), (f, name)
        assert frames[f]["view"].worldToView.tobytes() == unjittered[f]["view"].worldToView.tobytes()
        assert tuple(map(float, frames[f]["jitter"][0])) == tuple(map(float, FC.TR.jitter_sequence(f + 1)[f]))
        assert np.count_nonzero(frames[f]["depth"] != unjittered[f]["depth"]) > 0, "the jitter moves the raster"


def test_without_the_options_the_chain_is_the_taa_tests_chain(libraries, oracle, vr, gr, lr):
    """Only TAA left on, texture-free materials: depth, motion and LightingOutput of every frame equal taa_scenes.frame_inputs, the
    chain tests/test_gpu_taa.py trusts (oracle -> visibility_ref -> gbuffer_ref -> lighting_ref), fed the same jittered view."""
    off = tuple(o for o in FC.OPTIONS if o != "taa")
    frames = FC.run(libraries, oracle, off=off)
    sc = FC.scene(textured=False)
    geo_v = (sc["vertices"], sc["vertexIds"], sc["triangles"])
    for f, got in enumerate(frames):
        scf = dict(sc, instances=FC.instances_at(sc, f))
        depth, motion, lit = TS.frame_inputs(oracle, vr, gr, lr, scf, geo_v, got["view"], got["prev_world_to_clip"], sc["materials"], got["lighting_consts"])
        same(got["depth"].view(np.uint32), depth.view(np.uint32), f"frame {f}: depth")
        same(got["motion"], motion, f"frame {f}: motion")
        same(got["lighting_output"], lit, f"frame {f}: LightingOutput")
        assert "ssao" not in got and "shadow_mask" not in got and "volume" not in got and "bloom" not in got and "probe_winners" not in got
        assert (got["depth"] > 0).sum() > FC.RENDER[0] and np.any(motion != 0)


def test_the_first_frame_s_rasters_are_the_alpha_test_chain(libraries, oracle, unjittered):
    """Frame 0 without TAA: visibility and depth equal alpha_test_ref.frames on the decoded twins, the chain tests/test_gpu_alpha_test.py
    and tests/test_gpu_bc_textures.py trust."""
    chain = FC.Chain(libraries, oracle, off=("taa",))
    view, _ = FC.view_at(0)
    (ref, vis, depth), = AT.frames(oracle, libraries.at, dict(chain.sc, textures=chain.twins), view, FC.FLAGS, True, 1)
    same(unjittered[0]["vis"], vis, "visibility")
    same(unjittered[0]["depth"].view(np.uint32), depth.view(np.uint32), "depth")
    solid = FC.Chain(libraries, oracle, off=("taa", "alpha_test")).frame(0)
    assert np.count_nonzero(solid["depth"] != depth) >= MANY, "the discard opens the card"
