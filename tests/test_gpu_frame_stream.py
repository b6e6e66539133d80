"""Every option of FrameDriver together on the device: the everything-on configuration of tests/frame_stream.py on the Cornell
fixture at 64 x 36, three frames.  tests/test_frame_stream.py pins what the driver records but cannot see what the back end's
record functions refuse, and no other test runs every option in one frame."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_stream as FS  # noqa: E402
from suite_support import dev, recorded, sm  # noqa: E402, F401
from toyrenderer_amd import ddgi  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_option_together_records_the_golden_dispatches_and_runs(dev, oracle, sm):
    """Frame by frame the dispatch names equal the golden stream's; every download_* of the enabled options returns an array of its
    documented shape; the third frame's back buffer has a texel with colour; release() raises nothing."""
    W, H = FS.RENDER
    sc, gs = FS.cornell(dev, sm, oracle)
    frames, kw = FS.configurations()[FS.EVERYTHING]
    golden = FS.golden()[FS.EVERYTHING]["frames"]
    drv = FS.make_driver(dev, sc, gs, **kw)
    try:
        for n in range(frames):
            drv.frame_counter = n
            names = [shader for _, shader in recorded(drv) if shader]      # records the frame through a proxy of the list
            assert names == FS.dispatch_names(golden[n]), f"frame {n + 1}"
            drv.run()
        drv.results()
        shapes = {name: (a.shape, a.dtype) for name, a in dict(
            ssao=drv.download_ssao(), shadow_mask=drv.download_shadow_mask(), shadow_penumbra=drv.download_shadow_penumbra(), shadow_tiles=drv.download_shadow_tiles(),
            shadow_history=drv.download_shadow_history(), ddgi_rays=drv.download_ddgi_rays(), ddgi_fixed_rays=drv.download_ddgi_fixed_rays(),
            ddgi_variability=drv.download_ddgi_variability(), bloom0=drv.download_bloom(0), bloom1=drv.download_bloom(1), bloom2=drv.download_bloom(2),
            anti_aliased_output=drv.download_anti_aliased_output(), taa_history=drv.download_taa_history(), probe_winners=drv.download_probe_winners()).items()}
        assert shapes == dict(
            ssao=((H, W), np.uint8), shadow_mask=((H, W), np.uint8), shadow_penumbra=((H, W), np.uint16), shadow_tiles=((3, 4), np.uint8), shadow_history=((H, W), np.uint16),
            ddgi_rays=((64, 256, 4), np.float32), ddgi_fixed_rays=((64, 32), np.float32), ddgi_variability=((4, 24, 24), np.float32), bloom0=((H, W), np.uint32),
            bloom1=((H // 2, W // 2), np.uint32), bloom2=((H // 4, W // 4), np.uint32), anti_aliased_output=((H, W), np.uint32), taa_history=((H, W, 4), np.float16),
            probe_winners=((H, W), np.uint64))
        vol = drv.download_ddgi()
        assert isinstance(vol, ddgi.Volume) and vol.irradiance.shape == (4, 32, 32) and vol.distance.shape == (4, 64, 64, 2) and vol.data.shape == (4, 4, 4, 4)
        count, positions, probes = drv.download_probes()
        assert 0 <= count <= 64 and positions.shape == (count, 3) and positions.dtype == np.float32 and probes.shape == (count,) and probes.dtype == np.uint32
        back = drv.back_buffer.download_mip(0)
        assert back.shape == (H, W) and (back & 0xFFFFFF).any(), "frame 3's back buffer is black"
    finally:
        drv.release()
        gs.release()
