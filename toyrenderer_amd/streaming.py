"""Texture streaming from Python: the streamable textures of a GpuScene and the per-frame loop of FrameDriver(streaming=...).

The loop has the frame shape of the reference's TextureFeedbackManager, recorded into the frame's own command list:
  PrepareTexturesToProcessThisFrame : round-robin over the streamable textures, textures_per_frame at a time;
  BeginFrame : for every earlier frame whose read-back slot has arrived (rhi.Readback.ready: a poll, NEVER a wait for the device;
               a slot still in flight is looked at again by the next frame), apply THE RESIDENCY RULE (host.residency_round:
               csrc/host/TextureResidency.h, compiled host code without a GPU) to each texture that frame decoded, write
               the mapped tiles (write_texture_region, from the mips the scene kept on the host), poison the unmapped ones when asked,
               rewrite the min-mip maps that changed, and clear the feedback of this frame's textures;
  EndFrame   : decode this frame's textures' feedback into a buffer and copy it to the read-back slot of this frame (skipped while all
               READBACK_SLOTS slots are in flight).
The read-back LATENCY is one frame when each frame has completed before the next is recorded (frame f applies what frame f - 1 asked
for), and grows by the frames in flight otherwise, because nothing here waits.  With T streamable textures a static camera's image
therefore equals the fully resident one, and the maps have stopped changing, within ceil(T / textures_per_frame) + LATENCY + 1
frames (twentieth amendment).  The loop runs in record(): a frame that is run again without being recorded streams
nothing.  Textures keep their full device allocation: this saves upload traffic, not memory."""
from __future__ import annotations

import numpy as np

from . import host
from . import interop as I
from . import rhi

LATENCY = 1            # frames between a feedback's decode and its use, when each frame completes before the next is recorded
READBACK_SLOTS = 3     # read-back slots: frames whose feedback may be in flight
NONE = 0xFFFFFFFF
SLOTS = ("m_AlbedoTexture", "m_NormalTexture", "m_MetallicRoughnessTexture", "m_EmissiveTexture")


def default_region(fmt: int):
    """D3D's 64 KB tile shapes: 128 x 128 (RGBA8), 512 x 256 (BC1, BC4), 256 x 256 (BC2, BC3, BC5)."""
    if fmt not in rhi.BC_FORMATS:
        return 128, 128
    return (512, 256) if rhi.format_block_bytes(fmt) == 8 else (256, 256)


class StreamedTexture:
    """One streamable texture of a GpuScene: the device texture with its region, its two maps, the host mips and the residency."""

    def __init__(self, dev, index, mips, fmt, region, poison, name):
        self.index, self.format, self.region, self.poison = index, fmt, region, poison
        self.block_bytes = rhi.format_block_bytes(fmt) if fmt in rhi.BC_FORMATS else 0
        if self.block_bytes:
            self.w, self.h = int(mips.width), int(mips.height)
            self.host = [np.frombuffer(bytes(m), np.uint8).reshape((max(self.h >> k, 1) + 3) // 4, (max(self.w >> k, 1) + 3) // 4, self.block_bytes).copy()
                         for k, m in enumerate(mips)]
        else:
            self.host = [np.ascontiguousarray(m, np.uint8) for m in mips]
            self.h, self.w = self.host[0].shape[:2]
        self.levels = len(self.host)
        self.S, self.tiles = host.residency_tiles((self.w, self.h, self.levels), region)
        self.tile_bytes = region[0] * region[1] // 16 * self.block_bytes if self.block_bytes else region[0] * region[1] * 4
        self.regions = (self.w // region[0], self.h // region[1])
        self.resident, self.idle = np.zeros(max(self.tiles, 1), np.uint8), np.zeros(max(self.tiles, 1), np.uint32)
        self.min_mip = np.full((self.regions[1], self.regions[0]), self.S, np.uint8)
        self.texture = dev.create_texture(self.w, self.h, self.levels, fmt, name, uav=False)
        self.texture.set_streaming_region(*region)
        for k in range(self.levels):                                     # the packed tail is resident; the rest is poison or as allocated
            if k >= self.S:
                self.texture.upload_mip(k, self.host[k])
            elif poison is not None:
                self.texture.upload_mip(k, self._poison_like(self.host[k]))
        self.min_mip_map = dev.create_texture(self.regions[0], self.regions[1], 1, rhi.FORMAT_R8_UINT, f"{name} min-mip", uav=False)
        self.min_mip_map.upload_mip(0, self.min_mip)
        self.feedback = dev.create_sampler_feedback(self.texture, f"{name} feedback")
        self.min_mip_index = self.feedback_index = NONE                  # set by GpuScene.set_textures

    def _poison_like(self, a):
        return np.frombuffer((np.uint32(self.poison).tobytes() * (a.nbytes // 4 + 1))[:a.nbytes], np.uint8).reshape(a.shape)

    def tile(self, number):
        """(level, x, y, w, h in texels, the host bytes) of a tile number."""
        k = 0
        while number >= (tx := (self.w >> k) // self.region[0]) * ((self.h >> k) // self.region[1]):
            number -= tx * ((self.h >> k) // self.region[1])
            k += 1
        x, y = (number % tx) * self.region[0], (number // tx) * self.region[1]
        rw, rh = self.region
        data = self.host[k][y // 4:(y + rh) // 4, x // 4:(x + rw) // 4] if self.block_bytes else self.host[k][y:y + rh, x:x + rw]
        return k, x, y, rw, rh, np.ascontiguousarray(data)

    def release(self):
        for t in (self.texture, self.min_mip_map, self.feedback):
            t.release()


def create_streamed(dev, index, mips, fmt, streaming, name):
    """A StreamedTexture, or None for a texture that is not tiled (its size is no multiple of the DEFAULT region: it stays fully
    resident).  A size that is no multiple of a region GIVEN in streaming['region'] is refused by name."""
    w, h = (mips.width, mips.height) if hasattr(mips, "width") else (np.asarray(mips[0]).shape[1], np.asarray(mips[0]).shape[0])
    region = streaming.get("region")
    given = region is not None
    region = tuple(int(r) for r in region) if given else default_region(fmt)
    if w % region[0] or h % region[1]:
        if given:
            raise ValueError(f"set_textures: texture {index} of {w} x {h} texels is no multiple of the streaming region {region[0]} x {region[1]}")
        return None
    poison = streaming.get("poison")
    return StreamedTexture(dev, index, mips, fmt, region, None if poison is None or poison is False else int(poison) & 0xFFFFFFFF, name)


def check_materials(materials, streams, num_textures):
    """GpuScene.set_materials' rule for the two map indices, applied in place: a flagged slot of a streamable texture gets that texture's
    map indices when it names none; an index that names anything but the map of that very texture is refused."""
    by_index = {s.index: s for s in streams}
    for bit, slot in enumerate(SLOTS):
        t = materials[slot]
        for m in np.nonzero((materials["m_MaterialFlags"] >> bit) & 1)[0]:
            d, mm, fb = int(t["m_DescriptorIndex"][m]), int(t["m_MinMapTextureDescriptorIndex"][m]), int(t["m_FeedbackTextureDescriptorIndex"][m])
            s = by_index.get(d)
            if s is None:
                if mm != NONE or fb != NONE:
                    raise ValueError(f"set_materials: a material's texture ({slot}) names a sampler-feedback or min-mip texture, and its texture {d} is not "
                                     "streamable: texture streaming is on for textures loaded with set_textures(streaming=...) only")
                continue
            if (mm not in (NONE, s.min_mip_index)) or (fb not in (NONE, s.feedback_index)):
                raise ValueError(f"set_materials: a material's texture ({slot}) names a min-mip or feedback index ({mm:#x}, {fb:#x}) that is not the map of its own texture {d} "
                                 f"({s.min_mip_index}, {s.feedback_index})")
            t["m_MinMapTextureDescriptorIndex"][m], t["m_FeedbackTextureDescriptorIndex"][m] = s.min_mip_index, s.feedback_index


class TextureStreamingPass:
    """FrameDriver(gbuffer=True, streaming=dict(textures_per_frame=1, evict_after=4, poison=False, visualize=False)): the host loop of
    texture streaming over the scene's streamable textures (GpuScene.set_textures(..., streaming=dict(region=..., poison=...))).
    poison=True: a tile that is unmapped is overwritten with the scene's poison word, so that a read of it shows.  visualize:
    m_bVisualizeMinMipTilesOnAlbedoOutput.  streaming_stats holds the last recorded frame's numbers (tiles total, resident, uploaded
    this frame, bytes uploaded this frame, textures processed); download_min_mip(i) and download_feedback(i) read texture i's maps."""
    streaming = None
    streaming_stats = None

    def _check_streaming(self, streaming, gbuffer):
        if streaming is None:
            return
        if not gbuffer:
            raise ValueError("streaming= needs gbuffer=True (or lighting, post): the G-buffer resolve is what reads the maps and writes the feedback")
        if self.alpha_test:
            raise ValueError("streaming= with alpha_test=True: the alpha-tested rasters and the sun rays do not honour the min-mip map yet")
        if not self.scene.streams:
            raise ValueError("streaming= needs streamable textures: GpuScene.set_textures(..., streaming=dict(region=...))")
        unknown = set(streaming) - {"textures_per_frame", "evict_after", "poison", "visualize"}
        if unknown:
            raise ValueError(f"streaming=: unknown keys {sorted(unknown)}")
        s = dict(textures_per_frame=int(streaming.get("textures_per_frame", 1)), evict_after=int(streaming.get("evict_after", 4)),
                 poison=bool(streaming.get("poison", False)), visualize=bool(streaming.get("visualize", False)))
        if s["textures_per_frame"] < 1 or s["evict_after"] < 1:
            raise ValueError("streaming=: textures_per_frame and evict_after are at least 1")
        if s["poison"] and any(t.poison is None for t in self.scene.streams):
            raise ValueError("streaming=dict(poison=True) needs the scene's poison word: GpuScene.set_textures(..., streaming=dict(poison=0x...))")
        self.streaming = s

    def _create_streaming(self):
        if self.streaming is None:
            return
        streams = self.scene.streams
        self._stream_offsets = np.cumsum([0] + [t.regions[0] * t.regions[1] for t in streams])
        total = (int(self._stream_offsets[-1]) + 3) // 4 * 4
        self._stream_decoded = self._own(self.dev.create_buffer(total, "Decoded Sampler Feedback"))
        self._stream_readback = self._own(self.dev.create_readback(total, READBACK_SLOTS))
        self._stream_frame, self._stream_next, self._stream_pending = 0, 0, []
        self.streaming_history = []                                      # per recorded frame: {texture index: the feedback bytes the rule saw}

    def _streaming_begin_frame(self, cl):
        s, streams = self.streaming, self.scene.streams
        stats = dict(tilesTotal=sum(t.tiles for t in streams), tilesResident=0, tilesUploaded=0, bytesUploaded=0, texturesProcessed=0)
        seen = {}
        while self._stream_pending and self._stream_readback.ready(self._stream_pending[0][0]):   # oldest first; a poll, never a wait
            slot, earlier = self._stream_pending.pop(0)
            data, written = self._stream_readback.read(slot)
            if written != self._stream_readback.bytes_per_slot:          # that frame was recorded and never run: it decoded nothing
                continue
            for j in earlier:
                t = streams[j]
                fb = data[self._stream_offsets[j]:self._stream_offsets[j + 1]].reshape(t.regions[1], t.regions[0])
                seen[t.index] = fb.copy()
                got = host.residency_round((t.w, t.h, t.levels), t.region, t.tile_bytes, fb, s["evict_after"], t.resident, t.idle)
                t.resident, t.idle = got["resident"], got["idle"]
                for n in np.nonzero(got["mapped"][:t.tiles])[0]:
                    k, x, y, w, h, texels = t.tile(int(n))
                    cl.write_texture_region(t.texture, k, x, y, w, h, texels)
                if s["poison"]:
                    for n in np.nonzero(got["unmapped"][:t.tiles])[0]:
                        k, x, y, w, h, texels = t.tile(int(n))
                        cl.write_texture_region(t.texture, k, x, y, w, h, t._poison_like(texels))
                if not np.array_equal(got["min_mip"], t.min_mip):
                    t.min_mip = got["min_mip"]
                    cl.write_texture_region(t.min_mip_map, 0, 0, 0, t.regions[0], t.regions[1], t.min_mip)
                stats["tilesUploaded"] += got["stats"]["tilesMapped"]
                stats["bytesUploaded"] += got["stats"]["bytesUploaded"]
                stats["texturesProcessed"] += 1
        stats["tilesResident"] = int(sum(t.resident[:t.tiles].sum() for t in streams))
        n = min(s["textures_per_frame"], len(streams))                   # PrepareTexturesToProcessThisFrame
        self._stream_now = [(self._stream_next + i) % len(streams) for i in range(n)]
        self._stream_next = (self._stream_next + n) % len(streams)
        for j in self._stream_now:
            cl.clear_sampler_feedback(streams[j].feedback)
        self.streaming_stats = stats
        self.streaming_history.append(seen)

    def _streaming_end_frame(self, cl):
        streams, f = self.scene.streams, self._stream_frame
        if len(self._stream_pending) >= READBACK_SLOTS:                           # every slot is in flight: this frame's feedback is dropped
            return
        for j in self._stream_now:
            cl.decode_sampler_feedback(self._stream_decoded, streams[j].feedback, int(self._stream_offsets[j]))
        cl.copy_to_readback(self._stream_readback, f % READBACK_SLOTS, self._stream_decoded, 0, self._stream_decoded.size)
        self._stream_pending.append((f % READBACK_SLOTS, list(self._stream_now)))
        self._stream_frame = f + 1

    def _stream_of(self, i):
        for t in self.scene.streams:
            if t.index == i:
                return t
        raise ValueError(f"texture {i} is not streamable")

    def download_min_mip(self, i: int):
        """uint8 [regions y, regions x]: the min-mip map of texture i on the device."""
        return self._download("download_min_mip", self.streaming, "streaming= is off", lambda: self._stream_of(i).min_mip_map.download_mip(0))

    def download_feedback(self, i: int):
        """uint8 [regions y, regions x]: the feedback map of texture i on the device, decoded on the host (0xFF = never sampled)."""
        return self._download("download_feedback", self.streaming, "streaming= is off",
                              lambda: np.minimum(self._stream_of(i).feedback.download_mip(0), 0xFF).astype(np.uint8))
