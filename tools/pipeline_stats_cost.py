"""Cost of the base pass's pipeline statistics queries on the flagship frame (bench.py's drop-in path, one GPU).

Prints one JSON line: the frame time with statistics off and on (wall time of K frames each, after a warm-up), the stats
commands' own device time per frame (device profile filtered to one op name at a time), and the first stats command after
switching on, which also builds the byte array of triangle counts from the meshlet buffer.  For kernel times without the
profile's events: rocprofv3 --kernel-trace --stats -- python tools/pipeline_stats_cost.py --only-on.

    python tools/pipeline_stats_cost.py [--config C3] [--steps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only-on", action="store_true", help="statistics on for every frame, no profile (for rocprofv3)")
    args = ap.parse_args()

    from bench import build_shard, host_threads
    from toyrenderer_amd import host, rhi, synth

    spec = synth.config_spec(args.config)
    view = synth.make_view(eye=(0.0, 0.0, 0.0), prev_eye=(0.05, 0.0, 0.1), prev_yaw=0.002)
    depth = synth.gen_depth(view, 200)
    record_cap = spec.num_instances * ((spec.meshlets_lod0 + 31) // 32) + 1
    r = host.Renderer(render=(view.renderW, view.renderH), max_groups=record_cap, max_transient_bytes=8 << 30)
    try:
        dev = rhi.Device(handle=r.device())
        build_shard(spec, 0, 1, r, threads=min(8, host_threads()))
        r.set_culling(7)
        r.set_gpu_timers(False)
        r.upload_depth(depth)

        def frames(n):
            for _ in range(n):
                r.set_camera(view)
                r.frame()
            r.wait_idle()

        def timed(n):
            frames(args.warmup)
            t0 = time.perf_counter()
            frames(n)
            return (time.perf_counter() - t0) * 1e3 / n

        out = {"config": args.config, "steps": args.steps}
        if args.only_on:
            r.set_pipeline_statistics(True)
            out["frame_ms_on"] = timed(args.steps)
            out["stats"] = r.pipeline_statistics()[1]
            print(json.dumps(out))
            return
        frames(64)
        out["frame_ms_off"] = timed(args.steps)
        # first frame with statistics on: its early stats command builds the triangle-count bytes
        early, late = "basepass_AS_Main LATE_CULL=0#stats", "basepass_AS_Main LATE_CULL=1#stats"
        dev.profile_reset(); dev.profile_filter(early); dev.profile_enable(True)
        r.set_pipeline_statistics(True)
        frames(1)
        dev.profile_enable(False)
        out["first_early_stats_ms_with_byte_build"] = dev.profile().get(early, (0, 0.0))[1]
        out["frame_ms_on"] = timed(args.steps)
        for name in (early, late):
            dev.profile_reset(); dev.profile_filter(name); dev.profile_enable(True)
            frames(args.steps)
            dev.profile_enable(False)
            n, ms = dev.profile().get(name, (0, 0.0))
            out[name.split()[1].replace("#", "_") + "_ms_per_frame"] = ms / max(n, 1)
        dev.profile_filter(None)
        r.set_pipeline_statistics(False)
        out["frame_ms_off_again"] = timed(args.steps)
        out["stats"] = r.pipeline_statistics()[1]
        print(json.dumps(out))
    finally:
        r.shutdown()


if __name__ == "__main__":
    main()
