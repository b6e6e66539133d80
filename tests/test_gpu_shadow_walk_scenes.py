"""The sun's any-hit walk (occluded() in csrc/k_shadowmask.hip) and the TLAS refit beside it on the GPU, on scenes that can tell a wrong
walk apart: the directed cases of tests/shadow_scenes.py WALK_CASES, every word against brute force over every triangle
(tests/shadowmask_ref.c, SR.BRUTE).  tests/test_gpu_shadowmask.py runs the same kernels on seeded random scenes, which do not sit on the
walk's rules; here a ladder of triangles stands on both sides of TMin in instances of scale 1, 0.25 and 4, rotated and mirrored, roofs
stand on both sides of TMax (one of them only because t is the world's, not the object space's), world matrices have no inverse, the
TLAS has levels of more than 256 inner nodes and is 26 levels deep and is refitted to moved instances, leaves name instances without
flags, material indices lie past the buffer and the light is the zero vector.  tests/test_shadowmask_ref.py holds the preconditions
(that each case sits on both sides of its rule, with the counts);
profiles/shadowmask/walk_mutations.txt the negative controls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shadow_scenes as SS  # noqa: E402
import shadowmask_ref as SR  # noqa: E402
from shadow_passes import Pass, unflagged_case, walk_case  # noqa: E402
from suite_support import bare_gpu_scene, dev, same, sm  # noqa: E402, F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(SS.WALK_CASES))
def test_walk_cases_match_brute_force(dev, sm, name):
    """Refit + trace in one command list over targets pre-filled with the sentinels; a moved case's instances are uploaded behind
    set_raytracing(), so the refit is what moves the boxes.  The TLAS nodes read back equal SR.refit byte for byte, and so do the
    instance records; the mask and the linear view depth equal brute force; far texels keep the mask's sentinel.

    NO EXCEPTION for the record of an instance whose world matrix has no inverse (the "singular" cases), whose reference holds
    infinities and NaNs: it is compared byte for byte like every other.  The device's NaN words could differ from the host's only
    where IEEE 754 leaves the choice open, in the sign and payload of a NaN that an operation creates or passes on.  Here they do not.
    cm::div_ is the compiler's IEEE division, whose last instruction (v_div_fixup_f32) gives 0xFFC00000 for 0 / 0, the same word
    x86 gives; x / 0 is an infinity with the quotient's sign on both; the fourth row's products and sums only ever meet
    that one NaN word (every NaN in a record is the same 0 / 0), finite numbers and infinities, so whichever operand a machine's
    propagation rule picks, it picks 0xFFC00000, and the negation flips its sign to 0x7FC00000 on both.  Read back from one MI355X,
    the twelve words of the instance scaled by (1, 0, 1), by 0 and by 1e-20 equalled the host's.  WHOEVER ADDS A
    SINGULAR CASE checks this again: a record that CREATES a NaN outside the division need not agree, because the sign of an
    invalid-operation NaN is each machine's own.  Two routes exist in objectFromWorld: 0 x infinity (a translation component of
    exactly 0 against an infinite row) and infinity - infinity (a column of the fourth row whose terms are infinities of opposite
    sign and no NaN).  In every case here each column of the fourth row holds at least one 0 / 0, so neither route decides a word."""
    c = walk_case(sm, name)
    gs = bare_gpu_scene(dev, c.sc)
    p = Pass(dev, gs, c.W, c.H, c.noise)
    try:
        if c.moved is not None:
            gs.instances.upload(c.moved)
        got_mask, got_lvd = p.run(c.k, c.depth, c.g)
        nodes, records = p.structure()
        want_nodes, want_records = SR.refit(sm, c.acc, c.inst)
        assert nodes.tobytes() == want_nodes.tobytes(), f"{name}: TLAS nodes after the refit"
        assert records.tobytes() == want_records.tobytes(), f"{name}: TLAS instances after the refit"
        same(got_mask, c.mask, f"{name}: mask")
        same(got_lvd, c.lvd, f"{name}: linear view depth")
        assert np.all(got_mask[c.far] == SR.SENTINEL8)
    finally:
        p.release(); gs.release()


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_a_leaf_whose_instance_has_no_flags_casts_nothing(dev, sm, soft):
    """suite_support.unflagged_leaves: 7 instances keep their leaves, boxes and object-from-world rows and lose only their flags
    (the builder gives such an instance no leaf, so on a structure it built the walk's `flags == 0` rule decides nothing).  The
    refitted arrays are uploaded over the ones set_raytracing() built and the trace runs alone, without a refit: the mask equals
    brute force, which skips them; entered, those leaves would occlude 130 (hard) and 140 (soft) more texels
    (tests/test_shadowmask_ref.py).  The structure read back is the one uploaded."""
    c = unflagged_case(sm, soft)
    gs = bare_gpu_scene(dev, c.sc)
    gs.rt["tlas_nodes"].upload(c.acc.tlas["nodes"])
    gs.rt["tlas_instances"].upload(c.acc.tlas["records"])
    p = Pass(dev, gs, c.W, c.H, c.noise)
    try:
        got_mask, got_lvd = p.run(c.k, c.depth, c.g, refit=False)
        nodes, records = p.structure()
        assert nodes.tobytes() == c.acc.tlas["nodes"].tobytes() and records.tobytes() == c.acc.tlas["records"].tobytes(), "the structure as uploaded"
        assert np.all(records["flags"][c.off] == 0)
        same(got_mask, c.mask, "unflagged leaves: mask")
        same(got_lvd, c.lvd, "unflagged leaves: linear view depth")
        assert np.all(got_mask[c.far] == SR.SENTINEL8)
    finally:
        p.release(); gs.release()
