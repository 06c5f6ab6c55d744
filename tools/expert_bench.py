#!/usr/bin/env python3
"""Cost of the expert drivers on the device, next to the launches they sit beside (docs/HISTORY.md section 16).

4096 agents on Silverstone; the 7-ray potential field (the collectors' settings) and the 19-ray VFH.  HIP events around
`--iters` back-to-back okenv_expert_act calls without and with recording, around `expert_act + step(1)` pairs, and -- the
yardsticks, on the same handle in the same run -- around okenv_controller_act and okenv_step(1).  Then samples/s of
collect_demonstrations without and with 96 x 96 RGBA frames.  Prints one JSON document; --out writes it to a file too.

  python tools/expert_bench.py --out profiles/expert/expert_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import openkitchen_amd as ok  # noqa: E402
from openkitchen_amd.demonstrations import collect_demonstrations  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

COLLECTOR = dict(lookahead=2, goal_wrap=False, clamp_deg=10.0)


def timed(venv, fn, iters, repeats=5):
    """Median over `repeats` of the mean microseconds per call of `fn`, `iters` calls between two events."""
    out = []
    for _ in range(repeats):
        venv.reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / iters)
    return float(np.median(out)), [round(v, 3) for v in out]


def bench_kind(kind, fan, N, iters, track):
    v = VectorEnvironment(track, N, ray_angles_deg=fan, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=3)
    v.enable_expert(kind, **(COLLECTOR if kind == "potfield" else dict(goal_wrap=True)))
    R = fan.size
    rec = {"action": torch.empty((N, 2), device="cuda"), "dist": torch.empty((N, R), device="cuda"),
           "rel_xy": torch.empty((N, R, 2), device="cuda"), "alive": torch.empty((N,), dtype=torch.uint8, device="cuda")}
    n_params = v.env.controller_create(16)
    v.env.controller_set_params(np.random.default_rng(0).normal(0, 0.5, (N, n_params)).astype(np.float32))
    res = {"kind": kind, "rays": int(R), "agents": N, "iters": iters}

    def pair():
        v.env.expert_act()
        v.env.step(1)

    for name, fn in (("expert_act_us", lambda: v.env.expert_act()), ("expert_act_recording_us", lambda: v.env.expert_act(rec)),
                     ("expert_act_plus_step_us", pair), ("controller_act_us", lambda: v.env.controller_act(100.0, 5.0)),
                     ("step_us", lambda: v.env.step(1))):
        timed(v, fn, 20, repeats=1)  # warm-up
        res[name], res[name + "_runs"] = timed(v, fn, iters)
    v.close()
    return res


def bench_collect(N, steps, track, images):
    v = VectorEnvironment(track, N, ray_angles_deg=np.linspace(-90, 90, 7).astype(np.float32), auto_reset=True, randomize_lane=True,
                          randomize_heading=True, seed=3)
    v.enable_expert("potfield", **COLLECTOR)
    if images:
        v.enable_camera(96, 96)
    collect_demonstrations(v, 8, images=images, seed=1)
    torch.cuda.synchronize()
    runs = []
    for r in range(3):
        t0 = time.perf_counter()
        out = collect_demonstrations(v, steps, images=images, seed=2 + r)
        torch.cuda.synchronize()
        runs.append(N * steps / (time.perf_counter() - t0))
        del out
    v.close()
    return {"agents": N, "steps": steps, "images": bool(images), "samples_per_s": float(np.median(runs)), "runs": [round(x) for x in runs]}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--agents", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--collect-steps", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ok.build()
    doc = {"device": torch.cuda.get_device_name(0), "track": a.track,
           "kernels": [bench_kind("potfield", np.linspace(-90, 90, 7).astype(np.float32), a.agents, a.iters, a.track),
                       bench_kind("vfh", np.linspace(-90, 90, 19).astype(np.float32), a.agents, a.iters, a.track)],
           "collect": [bench_collect(a.agents, a.collect_steps, a.track, False), bench_collect(a.agents, a.collect_steps, a.track, True)]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
