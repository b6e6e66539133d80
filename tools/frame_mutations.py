"""Shows that tests/test_gpu_frame_chain.py can fail: mutants of the Python frame driver, each a swap of one binding or one matrix for
another of the same size and format, applied to a SCRATCH COPY of the toyrenderer_amd package (never to the tree) and run once
through pytest in a process that imports the copy.  No mutation touches an address, an extent, a loop bound or a dispatch size.

    python tools/frame_mutations.py --list
    python tools/frame_mutations.py MUTANT SCRATCH_DIR [pytest arguments ...]     # one mutant, one pytest run, in this process

A run of every mutant through the new file, tests/test_gpu_frame_stream.py and the per-pass file nearest to it (NEAREST) is recorded
in profiles/frame/mutations.txt.  The copy takes the package's Python files and links its lib/ directory, so the mutant runs the
product's own native libraries."""
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = "toyrenderer_amd"

# every mutant also gets this neutral edit: the driver keeps the frame's unjittered view where a mutation can reach it
PREPARE = [("frame.py", "        if self.taa is None:\n            return self._record_frame(query)\n", "        self._unjittered = self.view\n        if self.taa is None:\n            return self._record_frame(query)\n")]

# name: (what, [(file, old text (occurs exactly once), new text), ...])
MUTANTS = {
    "ao_unjittered": ("the AO constants from the unjittered projection (EQUIVALENT: GTAOUpdateConstants reads no element the jitter changes)",
                      [("gtao.py", "update_constants(W, H, self.ao, v.viewToClip,", "update_constants(W, H, self.ao, self._unjittered.viewToClip,")]),
    "ao_previous_view": ("the AO main pass's m_WorldToViewNoTranslate from the previous frame's world-to-view",
                         [("gtao.py", "push=main_pass_constants(v.worldToView,", "push=main_pass_constants(v.prevWorldToView,")]),
    "sky_unjittered": ("the sky's m_ClipToWorld unjittered",
                       [("sky.py", "pass_parameters(self.lighting_consts[\"m_ClipToWorld\"][0],",
                         "pass_parameters(I.clip_to_world(self._unjittered.worldToView, self._unjittered.viewToClip),")]),
    "probe_draw_unjittered": ("the probe draw's m_WorldToClip unjittered",
                              [("ddgi.py", "dk[\"m_WorldToClip\"] = I.world_to_clip(v.worldToView, v.viewToClip)",
                                "dk[\"m_WorldToClip\"] = I.world_to_clip(v.worldToView, self._unjittered.viewToClip)")]),
    "lighting_other_mask": ("lighting binds another R8_UNORM texture of the frame (the AO edges) as the shadow mask instead of the denoiser's; with the "
                            "denoiser on the trace writes the R16_FLOAT penumbra, so there is no raw mask of the mask's format to bind",
                            [("frame.py", "b.append(TEX_SRV(4, self.shadow_mask))", "b.append(TEX_SRV(4, self.ao_edges if self.ao_edges is not None else self.shadow_mask))")]),
    "bloom_before_sky": ("bloom recorded in front of the sky",
                         [("frame.py", "            self._sky(cl)\n        if self.bloom_mips:                                                              # Scene.cpp:503: between lighting and adapt luminance\n            self._bloom(cl)\n",
                           "            pass\n        if self.bloom_mips:\n            self._bloom(cl)\n        if self.sky is not None:\n            self._sky(cl)\n")]),
    "histogram_reads_aa": ("the histogram reads the anti-aliased output (the previous frame's: the resolve comes behind it)",
                           [("post.py", "[PUSH(0), TEX_SRV(0, self.lighting_output), UAV(0, self.histogram)]", "[PUSH(0), TEX_SRV(0, self.anti_aliased_output if self.taa is not None else self.lighting_output), UAV(0, self.histogram)]")]),
    "post_reads_lighting": ("post reads LightingOutput under TAA",
                            [("frame.py", "self._post_process(cl, self.anti_aliased_output if self.taa is not None else self.lighting_output)", "self._post_process(cl, self.lighting_output)")]),
    "sigma_history_swapped": ("the sigma history's two slots swapped: the stabilisation reads the slot written two frames ago and writes over the newest "
                              "(reading the very slot it writes is one texture bound twice, which the back end refuses)",
                              [("accel.py", "read, write = self.shadow_history[self.shadow_history_written], self.shadow_history[1 - self.shadow_history_written]",
                                "write, read = self.shadow_history[self.shadow_history_written], self.shadow_history[1 - self.shadow_history_written]")]),
    "taa_history_swapped": ("the TAA history's two slots swapped in the same way",
                            [("taa.py", "read, write = self.taa_history[self.taa_written], self.taa_history[1 - self.taa_written]",
                              "write, read = self.taa_history[self.taa_written], self.taa_history[1 - self.taa_written]")]),
}

# the per-pass GPU test file nearest to each mutation
NEAREST = {"ao_unjittered": "test_gpu_ao.py", "ao_previous_view": "test_gpu_ao.py", "sky_unjittered": "test_gpu_sky.py", "probe_draw_unjittered": "test_gpu_ddgi_probe_draw.py",
           "lighting_other_mask": "test_gpu_sigma.py", "bloom_before_sky": "test_gpu_bloom.py", "histogram_reads_aa": "test_gpu_postprocess.py",
           "post_reads_lighting": "test_gpu_taa.py", "sigma_history_swapped": "test_gpu_sigma.py", "taa_history_swapped": "test_gpu_taa.py"}


def make(name: str, scratch: str) -> str:
    """Writes the mutant's package under `scratch` and returns the directory to put in front of sys.path."""
    src, dst = os.path.join(ROOT, PACKAGE), os.path.join(scratch, PACKAGE)
    if os.path.exists(dst):
        shutil.rmtree(dst)
    os.makedirs(dst)
    for f in os.listdir(src):
        if f.endswith(".py"):
            shutil.copy(os.path.join(src, f), os.path.join(dst, f))
    os.symlink(os.path.join(src, "lib"), os.path.join(dst, "lib"))
    for file, old, new in PREPARE + MUTANTS[name][1]:
        path = os.path.join(dst, file)
        text = open(path).read()
        assert text.count(old) == 1, f"{name}: {file} holds the text to replace {text.count(old)} times: {old!r}"
        with open(path, "w") as out:
            out.write(text.replace(old, new))
    return scratch


def main(argv):
    if argv[:1] == ["--list"]:
        for name, (what, _) in MUTANTS.items():
            print(f"{name:24s} {NEAREST[name]:28s} {what}")
        return 0
    if len(argv) < 2 or argv[0] not in MUTANTS:
        sys.exit(__doc__)
    sys.path.insert(0, make(argv[0], os.path.abspath(argv[1])))
    import toyrenderer_amd
    assert os.path.dirname(toyrenderer_amd.__file__) == os.path.join(os.path.abspath(argv[1]), PACKAGE), toyrenderer_amd.__file__
    import pytest
    os.chdir(ROOT)
    return pytest.main(argv[2:])


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
