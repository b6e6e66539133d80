"""What FrameDriver records, without a GPU: every configuration of tests/frame_stream.py through the stand-in device, against the
streams tests/golden/frame_streams.json holds (written from the commit before the driver's passes moved into classes of their own;
tests/frame_stream.py says how).  Between them the configurations turn every option on at least once and leave it off at least once,
over three consecutive frames (the history ping-pongs, the reset flags, rotation n); the variability configuration over 19, where
the stand-in's read-back gives zeros and the rule converges at call 18."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_stream as FS  # noqa: E402
from suite_support import sm  # noqa: E402, F401


@pytest.fixture(scope="module")
def run(sm, oracle):
    """(streams, the stand-in device) after every driver and both scenes were released."""
    return FS.streams(sm, oracle)


@pytest.fixture(scope="module")
def golden():
    return FS.golden()


def test_the_configurations_are_the_golden_ones(run, golden):
    got, _ = run
    assert list(got) == list(golden)
    assert {name: len(c["frames"]) for name, c in got.items()} == {name: len(c["frames"]) for name, c in golden.items()}


@pytest.mark.parametrize("name", list(FS.golden()))
def test_every_frame_records_the_golden_stream(run, golden, name):
    """Method, shader, group counts or indirect buffer, every binding, and length and CRC-32 of every constant block, in order."""
    got, want = run[0][name], golden[name]
    for n, (g, w) in enumerate(zip(got["frames"], want["frames"])):
        for at, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"{name}, frame {n + 1}, event {at}"
        assert len(g) == len(w), f"{name}, frame {n + 1}: {len(g)} events, the golden stream has {len(w)}"


@pytest.mark.parametrize("name", list(FS.golden()))
def test_construction_creates_and_uploads_the_same(run, golden, name):
    """The same resources (name, size, format, flags), uploads (checksums) and set-up commands.  Their order is not pinned: the
    order in which a driver creates its resources decides nothing."""
    got, want = run[0][name]["setup"], golden[name]["setup"]
    assert sorted(got) == sorted(want)


def test_a_converged_update_records_nothing(golden):
    """Calls 1 to 17 record the probe update; calls 18 and 19 record none of it, no refit and no copy."""
    frames = golden["ddgi_update, variability"]["frames"]
    update = [[e for e in f if e[0] == "copy_to_readback" or (e[0] == "dispatch" and e[1].split("_")[0] in ("raytracing", "giprobetrace", "ProbeBlendingCS", "ProbeRelocationCS",
                                                                                                         "ProbeClassificationCS", "ReductionCS"))] for f in frames]
    assert [len(u) for u in update] == [10] * 17 + [0, 0]
    assert all("deferredlighting_PS_Main" in FS.dispatch_names(f) for f in frames)


def test_every_option_is_on_once_and_off_once(golden):
    """By what only the option records or binds."""
    marks = dict(occlusion="minmaxdownsample_CS_Main", raster_depth="basepass_MS_Main_depth", visibility="basepass_PS_Main_motion", gbuffer="basepass_PS_Main_GBuffer",
                 lighting="deferredlighting_PS_Main", debug_mode="deferredlighting_PS_Main_Debug", ao="ambientocclusion_CS_XeGTAO_MainPass DEBUG_OUTPUT_MODE=0",
                 shadows="shadowmask_CS_ShadowMask", shadow_denoise="SIGMA_Shadow_Blur.cs", alpha_test="basepass_MS_Main_visibility ALPHA_MASK_MODE=1",
                 ddgi_update="giprobetrace_CS_ProbeTrace", relocate="ProbeRelocationCS_DDGIProbeRelocationCS", variability="ReductionCS_DDGIReductionCS REDUCTION=1",
                 sky="sky_PS_HosekWilkieSky", post="postprocess_PS_PostProcess", auto_exposure="adaptluminance_CS_AdaptExposure", bloom_mips="bloom_PS_Upsample",
                 taa="taa_CS_TemporalResolve", probes="giprobevisualization_PS_VisualizeGIProbes")
    names = {name: set(FS.dispatch_names(c["frames"][0])) for name, c in golden.items()}
    for option, shader in marks.items():
        on = [name for name, s in names.items() if shader in s]
        assert on and len(on) < len(names), (option, on)
    lighting = {name: [e[3] for e in c["frames"][0] if e[0] == "dispatch" and e[1] == "deferredlighting_PS_Main"] for name, c in golden.items()}
    for option, binding in (("ddgi", "T7=DDGI Probe Irradiance"), ("external ssao", "T3=External SSAO"), ("external shadow_mask", "T4=External Shadow Mask")):
        on = [name for name, b in lighting.items() if b and binding in b[0]]
        assert on and len(on) < len([b for b in lighting.values() if b]), (option, on)


def test_everything_handed_out_is_released_exactly_once(run):
    _, dev = run
    wrong = [(o.name, o.released) for o in dev.made if o.released != 1]
    assert not wrong, wrong
