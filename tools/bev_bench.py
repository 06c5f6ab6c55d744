"""Bird's-eye camera views (okenv_render_views): views per second and kernel time for a population.

Default: C2's population (4096 agents, Silverstone, bench initial state), RGBA 96x96 at 1 and 2 samples per axis, RGBA 128x128
and CLASS8 64x64.  Each configuration is warmed up, then `--iters` back-to-back okenv_render_views calls are bracketed by one
pair of HIP events (torch.cuda.Event on the handle's stream): the time per call is kernel time plus launch gaps between
identical launches.  Output bytes per second are reported beside the ~6 TB/s plain-store rate of MI355X_MICROARCH (HBM
streaming stores).  Prints one JSON line per configuration.

  python tools/bev_bench.py [--agents 4096] [--track Silverstone] [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STORE_TBPS = 6.0  # plain-store rate quoted by the microarchitecture notes

CONFIGS = [  # (label, width, height, samples, format)
    ("rgba96_s1", 96, 96, 1, "rgba"),
    ("rgba96_s2", 96, 96, 2, "rgba"),
    ("rgba128_s1", 128, 128, 1, "rgba"),
    ("class64_s1", 64, 64, 1, "class"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--heading-up", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated labels")
    a = ap.parse_args()

    import torch

    import openkitchen_amd as ok
    capi = ok.capi
    if not torch.cuda.is_available():
        raise SystemExit("bev_bench needs a GPU")
    track = ok.Track(a.track)
    env = ok.BatchedEnvironment.from_track(track, a.agents, num_rays=15)
    env.init_bench_state()
    stream = torch.cuda.current_stream()
    env.set_stream(stream.cuda_stream)
    env.rollout_random(20, seed=1)  # spread the population a little (some crashed, some re-placed)
    torch.cuda.synchronize()
    flags = capi.VIEW_DRAW_AGENT | capi.VIEW_DRAW_HEADING | (capi.VIEW_HEADING_UP if a.heading_up else 0)
    only = set(a.only.split(",")) if a.only else None
    for label, w, h, s, fmt in CONFIGS:
        if only and label not in only:
            continue
        code = capi.VIEW_RGBA8 if fmt == "rgba" else capi.VIEW_CLASS8
        env.render_create(track, w, h, s, code, flags)
        info = env.render_info()
        out = torch.empty(env.render_shape, dtype=torch.uint8, device="cuda")
        for _ in range(a.warmup):
            env.render_views(out)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(a.iters):
            env.render_views(out)
        t1.record(stream)
        t1.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / a.iters
        nbytes = info["bytes_per_call"]
        print(json.dumps({
            "config": label, "track": a.track, "agents": a.agents, "width": w, "height": h, "samples": s, "format": fmt,
            "heading_up": a.heading_up, "us_per_call": round(us, 2), "views_per_s": round(a.agents / (us * 1e-6)),
            "out_bytes": nbytes, "out_TBps": round(nbytes / (us * 1e-6) / 1e12, 3), "store_floor_us": round(nbytes / (STORE_TBPS * 1e12) * 1e6, 2),
            "triangles": info["triangles"], "registrations": info["registrations"], "grid": [info["grid_nx"], info["grid_ny"]],
            "grid_cell": info["grid_cell"]}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
