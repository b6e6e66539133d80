"""The frame-level reference of probe variability: the tight Cornell volume of the placement tests (4 x 4 x 4 probes, relocation and
classification on) updated call by call on the CPU -- tests/ddgi_placement_ref.update for trace, blends and placement,
tests/ddgi_variability_ref.c for the variability buffer and its average, toyrenderer_amd.ddgi.VariabilityTracker for the rule -- as
FrameDriver(ddgi_update=dict(variability=True)) records it.  tests/test_gpu_ddgi_variability.py compares the drivers with it.

Run as a program it writes the sequence of averages and standard deviations (profiles/ddgi/variability_sequence.txt):
    python tests/ddgi_variability_frames.py 70 > profiles/ddgi/variability_sequence.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ddgi_placement_ref as DP  # noqa: E402
import ddgi_placement_scenes as PS  # noqa: E402
import ddgi_update_ref as DU  # noqa: E402
import ddgi_update_scenes as US  # noqa: E402
import ddgi_variability_ref as DV  # noqa: E402
from toyrenderer_amd import ddgi  # noqa: E402

F = np.float32
MIN_FRONT = 0.1                                   # GIRenderer.cpp:98: the fixture's bounding radius is below 3
# The threshold of the frame tests: the reference's own (GIRenderer.cpp:211).  The CPU run below has the ring's standard deviation
# fall under it at call 40 (9.4996e-04 after 1.2567e-03 at call 39: profiles/ddgi/variability_sequence.txt), between 18 and 60.
CONVERGES_AT = 40
THRESHOLD = 0.001


def driver_volume():
    """tests/test_gpu_ddgi_placement.py's: probe 22 pre-marked inactive."""
    vol = PS.tight_volume()
    vol.data[1, 1, 2, 3] = 1.0
    return vol


def settings(seed=13, threshold=THRESHOLD):
    return dict(seed=seed, relocate=True, classify=True, min_frontface_distance=MIN_FRONT, variability=True, variability_threshold=threshold)


def python_consts(seed, update):
    """The block FrameDriver's update number `update` runs with."""
    k = DU.consts(light=US.LIGHT, rotation=ddgi.random_rotation(np.random.default_rng([seed, update])))
    k["probeMinFrontfaceDistance"], k["probeFixedRayBackfaceThreshold"] = MIN_FRONT, 0.25
    return k


class Reference:
    """The volume's state call by call.  consts_of(update number) gives the block of a recorded update (the drivers differ in how
    they draw the rotation)."""

    def __init__(self, dv, dp, scene, threshold, consts_of):
        self.dv, self.dp, self.scene, self.consts_of = dv, dp, scene, consts_of
        self.state = driver_volume()
        self.state.variability = True
        self.rays = np.zeros((64, DU.RAYS, 4), F)
        self.var = np.zeros(DV.variability_shape(self.state), F)
        self.tracker = ddgi.VariabilityTracker(threshold)
        self.pending = [None, None]               # what the two read-back slots hold
        self.calls = self.updates = self.skipped = 0
        self.averages = []                        # per recorded update: the average its reductions wrote

    def reset(self):
        self.tracker.reset()
        self.var[...] = 0
        self.pending = [None, None]
        self.calls = self.skipped = 0

    def call(self):
        """One update call; True when it recorded nothing."""
        n = self.calls
        self.calls += 1
        if self.tracker.update():
            self.skipped += 1
            return True
        k = self.consts_of(self.updates)
        self.updates += 1
        before = self.state.copy()
        self.rays, _ = DP.update(self.dp, k, self.state, self.scene, rays_init=self.rays)
        irr, self.var, _ = DV.blend_radiance(self.dv, k, before, self.rays, self.var)
        assert np.array_equal(irr, self.state.irradiance)
        slot = n % 2
        self.tracker.set(F(0.0) if self.pending[slot] is None else self.pending[slot])
        avg, _, _ = DV.average(self.dv, self.state, self.var)        # behind placement: the data the reductions read
        self.pending[slot] = avg
        self.averages.append(avg)
        return False


def cornell_scene(sm, oracle):
    """(scene dict, reference scene) of the Cornell fixture as the frames have it."""
    import shadow_scenes as SS
    import shadowmask_ref as SR
    sc = SS.cornell()
    s = sc["loaded"]
    inst = sc["instances"].copy()
    oracle.update_instance_consts(s.nodes, s.primToNode, inst)
    inst["m_PrevWorldMatrix"] = inst["m_WorldMatrix"]
    sc["instances"] = inst
    s.meshData = sc["meshData"]
    return sc, DU.Scene(sm, SR.Accel(sc))


if __name__ == "__main__":
    import tempfile

    import shadowmask_ref as SR
    from oracle import pyoracle
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 70
    tmp = tempfile.mkdtemp()
    dv, dp, sm = DV.load(tmp), DP.load(tmp), SR.load(tmp)
    _, scene = cornell_scene(sm, pyoracle)
    ref = Reference(dv, dp, scene, 0.0, lambda u: python_consts(13, u))      # threshold 0: never converges, the whole sequence shows
    print("# tight Cornell volume (4 x 4 x 4), relocation and classification on, seed 13, FrameDriver's rotations; threshold 0 (never converges)")
    print("# python tests/ddgi_variability_frames.py %d" % calls)
    print("# call  average written    sample stored      ring stddev (at the call's Update)")
    for n in range(calls):
        ref.call()
        print("%4d  %.9e  %.9e  %.9e" % (n + 1, ref.averages[-1], ref.tracker.ring[ref.tracker.cursor], ref.tracker.stddev))
