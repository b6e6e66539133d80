"""What FrameDriver records, configuration by configuration, without a GPU: a stand-in of rhi.Device that notes every command in
order, the configurations of tests/test_frame_stream.py, and the golden file tests/golden/frame_streams.json.

The stand-in implements exactly the calls GpuScene, ddgi.Volume.upload and FrameDriver make.  It hands out objects with a handle
(`h`) as rhi's have, so rhi.CB / SRV / TEX_UAV ... build their ctypes bindings from them unchanged, and notes per event one list of
strings:
    dispatch            shader, "gx,gy,gz", the bindings, "length:crc32" of the push constants ("" without)
    dispatch_indirect   shader, the debug name of the arguments buffer, the bindings, the push constants
    constant_buffer     debug name, "length:crc32"
    write_buffer        buffer, offset, "length:crc32";  clear_*: resource, value;  copy_to_readback: slot, source, offset, bytes
    create, upload, execute, open, close: what the driver does around the lists
A binding reads kind + slot = debug name (@mip when not 0): b CB, push, t / u structured SRV / UAV, T / U texture SRV / UAV,
s sampler, table.  No payload is kept, only lengths and checksums.  The stand-in also counts release() per object.

The golden file is written from the commit BEFORE a change to the driver, with this file copied in, and committed as it is:
    python tests/frame_stream.py --write tests/golden/frame_streams.json
It holds every distinct event once ("events") and per configuration the indices of its set-up (construction) and of each frame."""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from toyrenderer_amd import rhi  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "frame_streams.json")
RENDER = (64, 36)
KINDS = ("b", "push", "t", "u", "T", "U", "s", "table")         # rhi.BIND_* in order


def _sum(data) -> str:
    raw = np.ascontiguousarray(data).tobytes()
    return f"{len(raw)}:{zlib.crc32(raw):08x}"


class _Object:
    """Anything the device hands out: a handle, a debug name and a count of release()."""

    def __init__(self, dev, name, tracked=True):
        self.dev, self.name, self.released = dev, name, 0
        dev.handles += 1
        self.h = dev.handles
        dev.by_handle[self.h] = self
        if tracked:
            dev.made.append(self)

    def release(self):
        self.released += 1


class Buffer(_Object, rhi.Buffer):
    """An rhi.Buffer by type (GpuScene.release_raytracing tells its buffers from its host arrays by it), none of its methods."""
    ptr = 0

    def __init__(self, dev, nbytes, name, tracked=True):
        _Object.__init__(self, dev, name, tracked)
        self.size, self.data = int(nbytes), None

    def upload(self, arr, offset=0):
        raw = np.ascontiguousarray(arr).tobytes()
        if self.data is None:
            self.data = bytearray(self.size)
        assert offset + len(raw) <= self.size, (self.name, offset, len(raw), self.size)
        self.data[offset:offset + len(raw)] = raw
        self.dev.note("upload", self.name, str(offset), _sum(arr))
        return self

    def download(self, dtype=np.uint32, count=None, offset=0):
        dtype = np.dtype(dtype)
        n = (self.size - offset) // dtype.itemsize if count is None else count
        raw = bytes(self.data or bytearray(self.size))[offset:offset + n * dtype.itemsize]
        return np.frombuffer(raw, dtype).copy()


class Texture(_Object):
    def __init__(self, dev, w, h, mips, fmt, name, array_size=0):
        super().__init__(dev, name)
        self.w, self.hgt, self.mips, self.format, self.array_size = w, h, mips, fmt, array_size

    def upload_mip(self, k, arr):
        self.dev.note("upload", self.name, f"mip {k}", _sum(arr))

    def upload_slice(self, k, arr):
        self.dev.note("upload", self.name, f"slice {k}", _sum(arr))


class TextureTable(_Object):
    def set(self, index, tex):
        self.dev.note("table_set", str(index), tex.name)


class Readback(_Object):
    def read(self, slot, dtype=np.uint8, count=None):
        return np.zeros(1 if count is None else int(count), np.dtype(dtype)), 0

    def reset(self):
        self.dev.note("readback_reset", self.name)


class CommandList(_Object):
    def _bindings(self, bindings) -> str:
        out = []
        for b in bindings:
            res = self.dev.by_handle[b.resource].name if b.resource else None
            out.append(KINDS[b.type] + str(b.slot) + ("" if res is None else "=" + res) + (f"@{b.baseMip}" if b.baseMip else ""))
        return " ".join(out)

    def open(self):
        self.dev.note("open")
        return self

    def close(self):
        self.dev.note("close")
        return self

    def write_buffer(self, buf, arr, offset=0):
        self.dev.note("write_buffer", buf.name, str(offset), _sum(arr))

    def clear_buffer_u32(self, buf, value=0):
        self.dev.note("clear_buffer_u32", buf.name, str(int(value)))

    def clear_texture_f32(self, tex, value):
        self.dev.note("clear_texture_f32", tex.name, repr(float(value)))

    def clear_texture_u32(self, tex, value):
        self.dev.note("clear_texture_u32", tex.name, str(int(value)))

    def constant_buffer(self, data, name="cb"):
        self.dev.note("constant_buffer", name, _sum(data))
        return Buffer(self.dev, np.ascontiguousarray(data).nbytes, name, tracked=False)   # the list's own, as rhi.CommandList keeps them

    def dispatch(self, shader, bindings, groups, push=None):
        self.dev.note("dispatch", shader, ",".join(str(int(g)) for g in groups), self._bindings(bindings), "" if push is None else _sum(push))

    def dispatch_indirect(self, shader, bindings, args, offset=0, push=None):
        self.dev.note("dispatch_indirect", shader, args.name + (f"+{offset}" if offset else ""), self._bindings(bindings), "" if push is None else _sum(push))

    def copy_to_readback(self, rb, slot, src, offset, nbytes):
        self.dev.note("copy_to_readback", str(int(slot)), src.name, str(int(offset)), str(int(nbytes)))


class Device:
    """The stand-in of rhi.Device.  log: every event since the last take(); made: every object handed out."""

    def __init__(self):
        self.handles, self.by_handle, self.made, self.log = 0, {}, [], []

    def note(self, *event):
        self.log.append(list(event))

    def take(self):
        out, self.log = self.log, []
        return out

    def wait_idle(self):
        pass

    def execute(self, *lists):
        self.note("execute", str(len(lists)))

    def create_buffer(self, nbytes, name="", stride=4, uav=True, indirect=False, virtual=False, volatile_constant=False):
        self.note("create", "buffer", name, f"{int(nbytes)} bytes, stride {stride}" + ("" if uav else ", no uav") + (", indirect" if indirect else ""))
        return Buffer(self, nbytes, name)

    def buffer_from(self, arr, name="", uav=True, min_bytes=4):
        arr = np.ascontiguousarray(arr)
        b = self.create_buffer(max(arr.nbytes, min_bytes), name=name, stride=max(arr.dtype.itemsize, 1), uav=uav)
        if arr.nbytes:
            b.upload(arr)
        return b

    def create_texture(self, w, h, mips, fmt, name="", uav=True, render_target=False):
        self.note("create", "texture", name, f"{w} x {h}, {mips} mips, format {fmt}" + ("" if uav else ", no uav") + (", render target" if render_target else ""))
        return Texture(self, w, h, mips, fmt, name)

    def create_texture_array(self, w, h, slices, fmt, name="", uav=False):
        self.note("create", "texture array", name, f"{w} x {h} x {slices}, format {fmt}" + (", uav" if uav else ""))
        return Texture(self, w, h, 1, fmt, name, array_size=slices)

    def create_sampled_texture(self, mips, fmt, name=""):
        t = self.create_texture(mips[0].shape[1], mips[0].shape[0], len(mips), fmt, name, uav=False)
        for k, m in enumerate(mips):
            t.upload_mip(k, m)
        return t

    def create_texture_table(self, capacity):
        self.note("create", "texture table", str(capacity))
        return TextureTable(self, "texture table")

    def create_readback(self, bytes_per_slot, slots):
        self.note("create", "readback", f"{slots} slots of {bytes_per_slot} bytes")
        return Readback(self, "readback")

    def create_command_list(self):
        self.note("create", "command list")
        return CommandList(self, "command list")


# ---- the scene and the configurations -----------------------------------------------------------------------------------------------------
def cornell(dev, sm, oracle):
    """(scene dict, GpuScene with its acceleration structure) of the Cornell fixture as tests/ddgi_variability_frames.py builds it."""
    import ddgi_variability_frames as VF
    from suite_support import gpu_scene
    sc, _ = VF.cornell_scene(sm, oracle)
    s = sc["loaded"]
    gs = gpu_scene(dev, s, sc["instances"], s.vertices, sc["materials"])
    gs.set_raytracing(sc["indices"], sc["cached"].meshSpecific)
    return sc, gs


def cornell_with_alpha_mask(dev, sc):
    """The fixture has no alpha-mask instance, so pass slots 2 and 3 never run on it: the same scene with its last opaque instance
    moved to the alpha-mask list."""
    from toyrenderer_amd.frame import GpuScene
    s = sc["loaded"]
    gs = GpuScene(dev, sc["instances"], s.meshData, s.meshlets, s.opaqueIds[:-1], s.opaqueIds[-1:])
    gs.set_geometry(s.vertices, s.meshletVertexIds, s.meshletTriangles)
    gs.set_materials(sc["materials"])
    gs.set_raytracing(sc["indices"], sc["cached"].meshSpecific)
    return gs


EVERYTHING = "everything"


def configurations():
    """{name: (frames, FrameDriver keywords)}: between them every option is on at least once and off at least once."""
    import ddgi_variability_frames as VF
    import shadow_scenes as SS
    import sky_ref as SK
    shadows, dataset = dict(noise=SS.noise_image()), SK.dataset()
    volume = VF.driver_volume

    def lit(**kw):
        return dict(lighting=True, **kw)
    c = {
        "flags 7": dict(culling_flags=7),
        "flags 5": dict(culling_flags=5),
        "raster_depth": dict(raster_depth=True),
        "visibility": dict(visibility=True),
        "visibility, flags 5": dict(visibility=True, culling_flags=5),
        "gbuffer": dict(gbuffer=True),
        "lighting": lit(),
        "lighting, debug_mode 2": lit(debug_mode=2),
        "ao": lit(ao=dict()),
        "ao, 2 denoise passes, gbuffer only": dict(gbuffer=True, ao=dict(denoise_passes=2, quality=1)),
        "shadows": lit(shadows=shadows),
        "shadows, shadow_denoise": lit(shadows=shadows, shadow_denoise=dict()),
        "alpha_test": lit(alpha_test=True, shadows=shadows),
        "alpha_test" + ALPHA_MASK: lit(alpha_test=True, shadows=shadows),
        "raster_depth, alpha_test" + ALPHA_MASK: dict(raster_depth=True, alpha_test=True),
        "lighting, flags 5" + ALPHA_MASK: lit(culling_flags=5),
        "ddgi": lit(ddgi=volume()),
        "ddgi_update": lit(ddgi=volume(), ddgi_update=dict(seed=4)),
        "ddgi_update, relocate and classify": lit(ddgi=volume(), ddgi_update=dict(seed=4, relocate=True, classify=True, min_frontface_distance=VF.MIN_FRONT)),
        "ddgi_update, variability": lit(ddgi=volume(), ddgi_update=VF.settings()),
        "sky": lit(sky=(dataset,)),
        "post, manual exposure": dict(post=True, exposure=(1.5, 0.18)),
        "post, auto exposure": dict(post=True),
        "bloom_mips 3": dict(post=True, bloom_mips=3, bloom_strength=0.2),
        "taa": dict(post=True, taa=dict()),
        "probes": dict(post=True, ddgi=volume(), probes=dict()),
        EVERYTHING: dict(post=True, ao=dict(), shadows=shadows, shadow_denoise=dict(), alpha_test=True, ddgi=volume(), ddgi_update=VF.settings(),
                         sky=(dataset, 3.0, (0.2, 0.2, 0.2)), bloom_mips=3, taa=dict(), probes=dict(hide_inactive=True)),
    }
    return {name: (19 if name == "ddgi_update, variability" else 3, kw) for name, kw in c.items()}


ALPHA_MASK = " (an alpha-mask instance)"          # configurations of this suffix run on cornell_with_alpha_mask


def make_driver(dev, sc, gs, **kw):
    import ddgi_update_scenes as US
    from toyrenderer_amd import gltf_lite
    from toyrenderer_amd.frame import FrameDriver
    cam = sc["camera"]
    return FrameDriver(dev, gs, gltf_lite.view_of(cam, RENDER), record_capacity=4096, dir_light=US.LIGHT, camera_origin=tuple(float(x) for x in cam.position), **kw)


def frames(drv, count):
    """Records and runs `count` consecutive frames; yields after each."""
    for n in range(count):
        drv.frame_counter = n
        drv.record()
        drv.run()
        yield n


def streams(sm, oracle):
    """({name: dict(setup=events, frames=[events, ...])}, the device) of every configuration, each driver released, then the scene."""
    dev = Device()
    sc, gs = cornell(dev, sm, oracle)
    masked = cornell_with_alpha_mask(dev, sc)
    out = {}
    configs = configurations()
    external = [dev.create_texture(*RENDER, 1, fmt, name) for fmt, name in ((rhi.FORMAT_R8_UNORM, "External Shadow Mask"), (rhi.FORMAT_R8_UINT, "External SSAO"),
                                                                          (rhi.FORMAT_R11G11B10_FLOAT, "External Bloom"))]
    configs["external shadow_mask, ssao and bloom"] = (3, dict(post=True, shadow_mask=external[0], ssao=external[1], bloom=(external[2], 0.3)))
    dev.take()
    for name, (count, kw) in configs.items():
        drv = make_driver(dev, sc, masked if name.endswith(ALPHA_MASK) else gs, **kw)
        out[name] = dict(setup=dev.take(), frames=[])
        for _ in frames(drv, count):
            out[name]["frames"].append(dev.take())
        drv.release()
    for t in external:
        t.release()
    gs.release()
    masked.release()
    return out, dev


def pack(s) -> dict:
    """The golden file's form: every distinct event once, the streams as indices into them."""
    events, index = [], {}

    def ids(stream):
        out = []
        for e in stream:
            key = tuple(e)
            if key not in index:
                index[key] = len(events)
                events.append(list(e))
            out.append(index[key])
        return out
    return dict(events=events, configurations={name: dict(setup=ids(c["setup"]), frames=[ids(f) for f in c["frames"]]) for name, c in s.items()})


def unpack(packed) -> dict:
    ev = packed["events"]
    return {name: dict(setup=[ev[i] for i in c["setup"]], frames=[[ev[i] for i in f] for f in c["frames"]]) for name, c in packed["configurations"].items()}


def golden() -> dict:
    with open(GOLDEN) as f:
        return unpack(json.load(f))


def dispatch_names(stream):
    return [e[1] for e in stream if e[0].startswith("dispatch")]


if __name__ == "__main__":
    import tempfile

    import shadowmask_ref as SR
    from oracle import pyoracle
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/frame_stream.py --write PATH")
    got, _ = streams(SR.load(tempfile.mkdtemp()), pyoracle)
    with open(sys.argv[2], "w") as f:
        json.dump(pack(got), f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(got)} configurations, {sum(len(c['frames']) for c in got.values())} frames -> {sys.argv[2]}")
