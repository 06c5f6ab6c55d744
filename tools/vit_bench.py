"""The image transformer driver: okenv_vit_act per call at the reference shape (224 x 224 frames, patch 8, width
384, 6 heads, 12 blocks, feed-forward 1536, head 128 / 64) at 16 and 64 agents, against dino.ViT behind frames_to_input in fp32 with the
same weights, eager and as one replayed torch.cuda.graph, and one iteration of dino.drive (step + camera + act).

    python tools/vit_bench.py [--out profiles/vit/vit_bench.json] [--reps 5] [--agents 16 64] [--kernel-stats results.db]
    python tools/vit_bench.py --act-only 16        # three acts and nothing else: the run to put under a kernel trace

Every figure is the time between two HIP events on the environment's stream around one call, median / min / max of --reps repetitions
after one warm-up call.  --kernel-stats merges the per-kernel totals of a kernel trace of the --act-only run (the trace's SQLite results database: its
`top_kernels` view of name, calls and total duration in microseconds) into the result.  FLOPs per agent are counted from the shape (2 per multiply-add: the linear layers, the
scores and the context); the floor is FLOPs / 157 TFLOP/s, the f32 matrix peak."""
import argparse
import json
import os
import sqlite3
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import dino  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

PEAK_TFLOPS = 157.0


def flop_per_agent(cfg):
    T, D, F = (cfg.image_size // cfg.patch) ** 2 + 1, cfg.dim, cfg.dim_feedforward
    block = T * (3 * D * D + D * D + 2 * D * F) + 2 * T * T * D
    return 2.0 * ((T - 1) * D * 3 * cfg.patch ** 2 + cfg.depth * block + D * cfg.head_hidden1 + cfg.head_hidden1 * cfg.head_hidden2 + cfg.head_hidden2)


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_ms(fn, reps):
    fn()
    return stats([event_ms(fn) for _ in range(reps)])


def attach(N):
    venv = VectorEnvironment("Austin", N, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=0)
    torch.manual_seed(0)
    model = dino.ViT().to(venv.device).eval()
    sd = model.state_dict()
    cfg = dino.vit_config_from_state_dict(sd)
    venv.enable_camera(width=cfg.image_size, height=cfg.image_size, fmt="rgba")
    venv.enable_vit_policy(cfg, dino.vit_params_from_state_dict(sd))
    venv.reset()
    venv.step(n_steps=8)
    return venv, model, cfg


def population(N, reps):
    venv, model, cfg = attach(N)
    frames = venv.camera()
    out = torch.empty(N, device=venv.device)
    flop = flop_per_agent(cfg) * N
    mean, std = (torch.tensor(list(v), device=venv.device) for v in (cfg.mean, cfg.std))  # (nothing is copied from the host inside the capture)

    def torch_act():
        with torch.no_grad():
            y = model(dino.frames_to_input(frames, mean, std))[:, 0]
        venv.throttle.fill_(dino.THROTTLE)
        torch.clamp(y * dino.STEER_SCALE, -dino.STEER_SCALE, dino.STEER_SCALE, out=venv.steering)
        return y

    res = {"vit_act_ms": timed_ms(lambda: venv.vit_act({"output": out}, frames=frames), reps), "torch_eager_fp32_ms": timed_ms(torch_act, reps)}
    want = torch_act()
    torch.cuda.synchronize()
    res["max_abs_output_difference"] = float((out - want).abs().max())
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch_act()
        with torch.cuda.graph(graph, stream=side):
            torch_act()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    res["torch_graph_fp32_ms"] = timed_ms(graph.replay, reps)

    def iteration():
        venv.step()
        venv.camera(out=frames)
        venv.vit_act(frames=frames)

    res["drive_iteration_ms"] = timed_ms(iteration, reps)
    res["flop_per_act"] = flop
    res["floor_ms"] = flop / (PEAK_TFLOPS * 1e12) * 1e3
    res["vit_act_tflops"] = flop / (res["vit_act_ms"]["median"] * 1e-3) / 1e12
    res["agents_per_pass"] = min(N, (1 << 30) // (4 * ((cfg.image_size // cfg.patch) ** 2 + 1) * (6 * cfg.dim + cfg.dim_feedforward)))
    venv.close()
    return res


def kernel_stats(path):
    rows = {}
    for name, calls, total_us in sqlite3.connect(path).execute("select name, total_calls, total_duration from top_kernels"):
        if "okVit" in name:
            rows[name.replace("void ", "").split("(")[0]] = {"calls": int(calls), "total_us": round(float(total_us), 1)}
    whole = sum(r["total_us"] for r in rows.values())
    for r in rows.values():
        r["share_of_the_act"] = round(r["total_us"] / whole, 4)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "vit", "vit_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--agents", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--act-only", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.act_only:
        venv, model, cfg = attach(a.act_only)
        frames = venv.camera()
        for _ in range(3):
            venv.vit_act(frames=frames)
        torch.cuda.synchronize()
        venv.close()
        return
    res = {"device": torch.cuda.get_device_name(0), "track": "Austin",
           "network": "224 x 224 frames, patch 8 (785 tokens), width 384, 6 heads, 12 blocks, feed-forward 1536, head 384-128-64-1", "reps": a.reps,
           "peak_tflops_f32_matrix": PEAK_TFLOPS, "populations": {str(N): population(N, a.reps) for N in a.agents}}
    if a.kernel_stats:
        res["kernels_of_three_acts_at_16_agents"] = kernel_stats(a.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
