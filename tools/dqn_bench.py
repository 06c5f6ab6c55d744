"""Deep-Q learning on the device: rollout.dqn_update against the example's PyTorch loop on the same ring
contents, okenv_replay_push against the step launch it follows, the device time of the update's two kernels, and the example's own
printed times and losses on both paths.

    python tools/dqn_bench.py [--out profiles/dqn/dqn_bench.json] [--reps 9] [--skip-example]

(1) One episode per population fills the device's ring (collect_episode_dqn on Silverstone, epsilon 0.99); its fields are copied
    into the example's TorchRing.  (a) is examples/dqn_racer.py's update_torch as it is, (b) rollout.dqn_update, both 200 iterations
    on one batch of B samples.  Wall-clock times between two device synchronisations, alternated, median / min / max of --reps
    repetitions after one warm-up of each; both keep stepping their own parameters.
(2) 200 x okenv_replay_push and 200 x okenv_step(1) at 4096 agents on the same handle, each between two device events.
(3) The events okenv_dqn_update records around its kernels while okenv_set_timing is on.
(4, 5) examples/dqn_racer.py for five episodes at 1024 agents on both paths: its printed lines."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import dqn_racer  # noqa: E402
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd.rollout import DQN_ACTIONS, collect_episode_dqn, dqn_update  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
ITERATIONS, CAPACITY = 200, 1 << 20


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def population(N, reps):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=False, seed=0)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 5)).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=dqn_racer.LR)
    venv.enable_actor(net, mode="eps_greedy", actions=DQN_ACTIONS, epsilon=0.99)
    venv.enable_learner(lr=dqn_racer.LR)
    venv.enable_replay(CAPACITY, gamma=dqn_racer.GAMMA)
    ep = collect_episode_dqn(venv, max_steps=3000, graph_chunk=32)
    size, pushed = venv.env.replay_size()
    ring = dqn_racer.TorchRing(CAPACITY, 5, venv.device)
    venv.env.replay_get({"state": ring.state, "next_state": ring.next_state, "action": ring.action, "reward": ring.reward, "done": ring.done})
    ring.pushed = pushed
    gen = torch.Generator(device=venv.device)
    gen.manual_seed(0)
    res = {"steps": ep["steps"], "transitions": size, "batches": {}}
    for B in (100, 4096):
        parent = lambda: dqn_racer.update_torch(net, opt, ring, B, ITERATIONS, False, gen)  # noqa: E731
        device = lambda: dqn_update(venv, batch=B, iterations=ITERATIONS)  # noqa: E731
        parent()
        device()
        a_ms, b_ms = [], []
        for _ in range(reps):  # alternated: both see the same machine
            a_ms.append(wall(parent))
            b_ms.append(wall(device))
        venv.env.set_timing(True)
        per_kernel = {k: [] for k in capi.UPDATE_KERNELS}
        for _ in range(reps):
            device()
            for k, v in venv.env.dqn_timing().items():
                per_kernel[k].append(v)
        venv.env.set_timing(False)
        kernels = {k: {"us_per_update": stats(per_kernel[k]), "us_per_iteration": stats(per_kernel[k])["median"] / ITERATIONS} for k in capi.UPDATE_KERNELS}
        a, b = stats(a_ms), stats(b_ms)
        res["batches"][str(B)] = {"torch_loop_ms": a, "dqn_update_ms": b, "ratio_of_medians": a["median"] / b["median"],
                                  "torch_spread_ms": a["max"] - a["min"], "gain_ms": a["median"] - b["median"],
                                  "faster_by_more_than_the_torch_spread": (a["median"] - b["median"]) > (a["max"] - a["min"]), "kernels": kernels,
                                  "kernel_sum_us": sum(kernels[k]["us_per_update"]["median"] for k in kernels)}
    venv.close()
    return res


def push_against_step(reps, calls=200, N=4096):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=True, seed=0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 5)).cuda()
    venv.enable_actor(net, mode="eps_greedy", actions=DQN_ACTIONS, epsilon=0.99)
    venv.enable_replay(CAPACITY)
    rec = {"state": torch.empty((N, 5), device=venv.device), "action": torch.empty(N, dtype=torch.int64, device=venv.device),
           "alive": torch.empty(N, dtype=torch.uint8, device=venv.device)}
    venv.actor_act(rec)
    venv.env.step(1)
    venv.replay_push(rec)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / calls

    push_us, step_us = [], []
    for _ in range(reps):
        push_us.append(timed(lambda: venv.replay_push(rec)))
        step_us.append(timed(lambda: venv.env.step(1)))
    venv.close()
    p, s = stats(push_us), stats(step_us)
    return {"agents": N, "calls": calls, "push_us_per_call": p, "step_us_per_call": s, "push_costs_less_than_the_step": p["median"] < s["median"]}


def example(path, episodes=5, agents=1024):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dqn_racer.py"), "--agents", str(agents), "--episodes", str(episodes),
                          "--max-steps", "1000", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, cwd=ROOT)
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.startswith("episode")]
    return {"returncode": out.returncode, "lines": lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dqn", "dqn_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-example", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Silverstone", "rays": 5, "iterations": ITERATIONS, "reps": args.reps,
           "populations": {str(N): population(N, args.reps) for N in (1024, 4096)}, "push": push_against_step(args.reps)}
    if not args.skip_example:
        res["example"] = {path: example(path) for path in ("--device-update", "--torch-update")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
