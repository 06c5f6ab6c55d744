"""Shared-network actors on the device: what okenv_actor_act costs next to the calls around it, and what an
episode iteration costs in the four forms of the policy-gradient loop.

    python tools/actor_bench.py [--out profiles/actor/actor_bench.json]

Device events around back-to-back calls; every figure is the median of --reps repetitions with the smallest and the largest beside
it.  The PyTorch-actor forms (1, 2) are the baseline and are measured from that code path in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.rollout import PPO_ACTIONS, collect_episode, collect_episode_device  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.array([-70, -30, 0, 30, 70], dtype=np.float32)


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def time_calls(fn, calls, reps):
    """us per call of `calls` back-to-back calls between two device events."""
    out = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / calls)
    return stats(out[1:])  # the first repetition warms up


def networks(seed):
    torch.manual_seed(seed)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3), torch.nn.Softmax(dim=1)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    return actor, critic


def kernel_figures(N, reps):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=True, seed=0, reward="step")
    actor, critic = networks(0)
    venv.enable_actor(actor, critic)
    venv.reset()
    rec = {"state": torch.empty((N, 5), device="cuda"), "action": torch.empty(N, dtype=torch.int64, device="cuda"),
           "prob": torch.empty(N, device="cuda"), "value": torch.empty(N, device="cuda"), "alive": torch.empty(N, dtype=torch.bool, device="cuda")}
    env = venv.env
    out = {"actor_act_us": time_calls(lambda: env.actor_act(), 200, reps), "actor_act_record_us": time_calls(lambda: env.actor_act(rec), 200, reps)}
    env.expert_create("potfield")
    out["expert_act_us"] = time_calls(lambda: env.expert_act(), 200, reps)
    n = env.controller_create(16)
    env.controller_set_params(np.zeros((N, n), dtype=np.float32))
    out["controller_act_us"] = time_calls(lambda: env.controller_act(30.0, 5.0), 200, reps)
    env.actor_act()
    out["step_us"] = time_calls(lambda: env.step(1), 200, reps)
    venv.close()
    return out


def loop_figures(N, reps, steps):
    """us per iteration of a fixed number of iterations (auto-reset on, so that every form runs `steps` iterations)."""
    out = {}
    for form in ("1_torch_eager", "2_torch_graph", "3_device_eager", "4_device_graph32"):
        venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=True, seed=0, reward="step")
        actor, critic = networks(0)
        venv.enable_actor(actor, critic)
        table = torch.tensor(PPO_ACTIONS, dtype=torch.float32, device="cuda")
        times = []
        if form == "2_torch_graph":
            venv.reset()
            slot = {"a": torch.zeros(N, dtype=torch.int64, device="cuda"), "p": torch.zeros(N, device="cuda")}

            def body():
                with torch.no_grad():
                    probs = torch.clamp(actor(venv.observation()), 1e-8, 1.0 - 1e-8)
                    action = torch.multinomial(probs, 1).squeeze(1)
                    slot["p"].copy_(torch.log(probs.gather(1, action.unsqueeze(1))).squeeze(1))
                    slot["a"].copy_(action)
                venv.step(table[action])
            graph = venv.capture(body)
            run = lambda: [graph.replay() for _ in range(steps)]  # noqa: E731
        elif form == "1_torch_eager":
            run = lambda: collect_episode(venv, actor, max_steps=steps, check_every=32)  # noqa: E731
        elif form == "3_device_eager":
            run = lambda: collect_episode_device(venv, max_steps=steps, check_every=32)  # noqa: E731
        else:
            run = lambda: collect_episode_device(venv, max_steps=steps, graph_chunk=32)  # noqa: E731
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6 / steps)
        out[form] = stats(times[1:])
        venv.close()
    base_spread = max(out["1_torch_eager"]["max"] - out["1_torch_eager"]["min"], out["2_torch_graph"]["max"] - out["2_torch_graph"]["min"])
    out["ratio_form1_over_form3"] = out["1_torch_eager"]["median"] / out["3_device_eager"]["median"]
    out["ratio_form2_over_form4"] = out["2_torch_graph"]["median"] / out["4_device_graph32"]["median"]
    out["baseline_spread_us"] = base_spread
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "actor", "actor_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=512)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "networks": "5-128-3 + 5-128-1", "track": "Silverstone", "rays": 5,
           "kernel_4096": kernel_figures(4096, args.reps),
           "loop_us_per_iteration": {str(N): loop_figures(N, args.reps, args.steps) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
