"""The scenes of the probe draw's tests (tests/test_ddgi_probe_draw_ref.py on the reference alone, tests/test_gpu_ddgi_probe_draw.py
on the GPU): what "giprobevisualization_PS_VisualizeGIProbes" is handed when it is dispatched alone.  Each scene names the counters of
tests/ddgi_probe_draw_ref.c it exists for (SHOWS); the CPU test asserts that the reference counts them, so a scene that cannot show
its point fails there and not silently on the GPU.

The camera sits at the origin and looks down -Z (synth.make_view, near 0.1).  The culled positions at t0 are the scene's own and
differ from the volume's probe positions: the shading must take the probe from the volume, through the instance -> probe map."""
import numpy as np

from toyrenderer_amd import ddgi, synth
from toyrenderer_amd import interop as I

F = np.float32
NEAR = 0.1
SIZES = ((96, 64), (67, 35))
GAMMAS = (5.0, 2.5)


def volume(seed=7, gamma=5.0, counts=(3, 2, 3), relocation=True, classification=True):
    """A seeded volume around (0, 0, -4): every irradiance texel random with borders filled, offsets within 0.3 of a cell, a third
    of the probes switched off."""
    rng = np.random.default_rng(seed)
    v = ddgi.Volume((0.0, 0.0, -4.0), (1.0, 0.75, 1.25), counts, 0.1, 0.3, gamma, relocation=relocation, classification=classification)
    v.irradiance[...] = ddgi.pack_unorm10(rng.uniform(0.02, 1.0, v.irradiance.shape + (3,)))
    ddgi.fill_borders(v.irradiance, I.kDDGIIrradianceInteriorTexels)
    v.data[..., :3] = rng.uniform(-0.3, 0.3, v.data.shape[:3] + (3,)).astype(np.float16)
    v.data[..., 3] = (rng.uniform(size=v.data.shape[:3]) < 0.34).astype(np.float16)
    return v


def constant_volume(rgb=(0.5, 0.25, 0.125)):
    """One probe at (0, 0, -3) whose every irradiance texel decodes to rgb / pi on the screen."""
    return ddgi.Volume.uniform((0.0, 0.0, -3.0), (1.0, 1.0, 1.0), (1, 1, 1), irradiance=rgb)


def world_to_clip(size):
    view = synth.make_view(render=size, near=NEAR)
    return I.world_to_clip(view.worldToView, view.viewToClip)


def depth_plane(size, z):
    """A depth buffer with everything at view distance z (reversed Z: near / z)."""
    return np.full((size[1], size[0]), F(NEAR) / F(z), F)


def depth_plane_and_step(size):
    """The left half at distance 2.8, which cuts the unit-depth range of a sphere at distance 3; the right half at 3.2 above a
    far step (0, nothing drawn) in the lowest quarter."""
    W, H = size
    d = np.zeros((H, W), F)
    d[:, :W // 2] = F(NEAR) / F(2.8)
    d[:, W // 2:] = F(NEAR) / F(3.2)
    d[H - H // 4:, W // 2:] = 0.0
    return d


def seeded_color(size, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, (size[1], size[0]), dtype=np.uint64).astype(np.uint32)


# name: (positions, instance -> probe, radius, depth: "none" | "plane" | "step", counters the scene exists for)
SCENES = {
    "one": ([(0.0, 0.0, -3.0)], [4], 0.5, "none", ("won", "back_culled", "no_area")),
    "one, plane and step": ([(0.1, -0.05, -3.0)], [9], 0.5, "step", ("won", "lost_to_scene")),
    "two overlapping": ([(0.0, 0.0, -3.0), (0.35, 0.1, -3.2)], [2, 11], 0.5, "none", ("won", "multi_instance")),
    "two coincident": ([(0.2, 0.1, -3.0), (0.2, 0.1, -3.0)], [5, 16], 0.4, "step", ("won", "multi_instance", "tie", "lost_to_scene")),
    "across each edge": ([(-1.95, 0.0, -3.0), (1.95, 0.1, -3.0), (0.0, 1.25, -3.0), (0.1, -1.25, -3.0), (1.9, 1.2, -3.0)], [0, 1, 2, 3, 17], 0.5, "none",
                         ("won", "clip_left", "clip_right", "clip_top", "clip_bottom")),
    "across the near plane": ([(0.45, 0.05, -0.3)], [6], 0.4, "none", ("won", "near_dropped")),
    "around the camera": ([(0.0, 0.0, 0.05)], [7], 1.0, "none", ("near_dropped", "back_culled")),
    "below half a pixel": ([(0.0, 0.0, -3.0)], [8], 0.008, "none", ("no_centre",)),
    "large": ([(0.05, 0.02, -1.3)], [10], 1.0, "plane", ("won", "lost_to_scene", "clip_top", "clip_bottom")),       # most of the screen
    "everything": ([(0.0, 0.0, -3.0), (0.35, 0.1, -3.2), (0.35, 0.1, -3.2), (-1.95, 0.0, -3.0), (1.95, 0.1, -3.0), (0.0, 1.25, -3.0), (0.1, -1.25, -3.0),
                    (0.45, 0.05, -0.3), (0.0, 0.0, 0.05), (0.5, 0.5, -3.0), (-0.6, -0.3, -2.5)], [4, 2, 11, 0, 1, 3, 17, 6, 7, 8, 13], 0.45, "step",
                   ("won", "lost_to_scene", "multi_instance", "tie", "near_dropped", "back_culled", "clip_left", "clip_right", "clip_top", "clip_bottom")),
}


def on_its_own_depth(draw, size, gamma=5.0):
    """"one" over a depth buffer that holds, where the sphere lies, exactly the depth the sphere itself has there (draw(scene) ->
    (winners, colour, depth, counters), the reference's draw): every winning sample ties the scene, which GREATER_OR_EQUAL lets
    through and GREATER would not.  Elsewhere the buffer is 0."""
    s = scene("one", size, gamma)
    s["depth"] = draw(s)[2]
    return s


def scene(name, size, gamma=5.0):
    """dict(vol, positions, to_probe, count, radius, near, world_to_clip, depth, color, shows)."""
    positions, to_probe, radius, depth, shows = SCENES[name]
    d = {"none": lambda: np.zeros((size[1], size[0]), F), "plane": lambda: depth_plane(size, 0.38), "step": lambda: depth_plane_and_step(size)}[depth]()
    positions = np.asarray(positions, F)
    if name == "below half a pixel":                                  # its centre on the corner of four pixels, whatever the size
        m = world_to_clip(size)
        cx, cy = size[0] // 2, size[1] // 2
        positions = np.asarray([[(2.0 * cx / size[0] - 1.0) * 3.0 / m[0, 0], (1.0 - 2.0 * cy / size[1]) * 3.0 / m[1, 1], -3.0]], F)
    return dict(vol=volume(gamma=gamma), positions=positions, to_probe=np.asarray(to_probe, np.uint32), count=len(positions), radius=radius, near=NEAR,
                world_to_clip=world_to_clip(size), depth=d, color=seeded_color(size), shows=shows)
