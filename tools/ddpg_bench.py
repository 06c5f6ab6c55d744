"""DDPG on the device: rollout.ddpg_update against the example's PyTorch loop on the same ring contents,
okenv_ddpg_act and okenv_ddpg_replay_push against the step launch they surround, the device time of the update's four kernels, and
the example's own printed times and losses on both paths.

    python tools/ddpg_bench.py [--out profiles/ddpg/ddpg_bench.json] [--reps 9] [--skip-example]

(1) One episode at 1024 agents fills the device's ring (collect_episode_ddpg on Silverstone, uniform exploration (20, 2)); its fields
    are copied into the example's TorchRing.  (a) is examples/ddpg_racer.py's TorchDdpg.update as it is, (b) rollout.ddpg_update, both
    50 iterations on batches of B samples.  Wall-clock times between two device synchronisations, alternated, median / min / max of
    --reps repetitions after one warm-up of each; both keep stepping their own parameters.
(2) 200 x okenv_ddpg_act, 200 x okenv_ddpg_replay_push and 200 x okenv_step(1) at 4096 agents on one handle, each between two events.
(3) The events okenv_ddpg_update records around its kernels while okenv_set_timing is on.
(4, 5) examples/ddpg_racer.py for five episodes at 1024 agents on both paths: its printed lines."""
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
import ddpg_racer  # noqa: E402
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd.rollout import collect_episode_ddpg, ddpg_update  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
ITERATIONS, CAPACITY = 50, 1 << 20


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def networks():
    torch.manual_seed(0)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 2)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(7, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    return actor, critic


def update(reps, N=1024):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=False, seed=0)
    actor, critic = networks()
    venv.enable_ddpg(actor, critic, noise=(20.0, 2.0))
    venv.enable_ddpg_replay(CAPACITY)
    ep = collect_episode_ddpg(venv, max_steps=3000, graph_chunk=32)
    size, pushed = venv.env.ddpg_replay_size()
    ring = ddpg_racer.TorchRing(CAPACITY, 5, venv.device)
    venv.env.ddpg_replay_get({"state": ring.state, "next_state": ring.next_state, "action": ring.action, "reward": ring.reward, "done": ring.done})
    ring.pushed = pushed
    agent = ddpg_racer.TorchDdpg(actor, critic, venv.device)
    gen = torch.Generator(device=venv.device)
    gen.manual_seed(0)
    res = {"agents": N, "steps": ep["steps"], "transitions": size, "batches": {}}
    for B in (250, 4096):
        parent = lambda: agent.update(ring, B, ITERATIONS, gen)  # noqa: E731
        device = lambda: ddpg_update(venv, batch=B, iterations=ITERATIONS)  # noqa: E731
        parent()
        device()
        a_ms, b_ms = [], []
        for _ in range(reps):  # alternated: both see the same machine
            a_ms.append(wall(parent))
            b_ms.append(wall(device))
        venv.env.set_timing(True)
        per_kernel = {k: [] for k in capi.DDPG_KERNELS}
        for _ in range(reps):
            device()
            for k, v in venv.env.ddpg_timing().items():
                per_kernel[k].append(v)
        venv.env.set_timing(False)
        kernels = {k: {"us_per_update": stats(per_kernel[k]), "us_per_iteration": stats(per_kernel[k])["median"] / ITERATIONS} for k in capi.DDPG_KERNELS}
        a, b = stats(a_ms), stats(b_ms)
        res["batches"][str(B)] = {"torch_loop_ms": a, "ddpg_update_ms": b, "ratio_of_medians": a["median"] / b["median"],
                                  "torch_spread_ms": a["max"] - a["min"], "gain_ms": a["median"] - b["median"],
                                  "faster_by_more_than_the_torch_spread": (a["median"] - b["median"]) > (a["max"] - a["min"]), "kernels": kernels,
                                  "kernel_sum_us": sum(kernels[k]["us_per_update"]["median"] for k in kernels)}
    venv.close()
    return res


def act_and_push_against_step(reps, calls=200, N=4096):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=True, seed=0)
    actor, critic = networks()
    venv.enable_ddpg(actor, critic, noise=(20.0, 2.0))
    venv.enable_ddpg_replay(CAPACITY)
    rec = {"state": torch.empty((N, 5), device=venv.device), "action": torch.empty((N, 2), device=venv.device),
           "alive": torch.empty(N, dtype=torch.uint8, device=venv.device)}
    venv.ddpg_act(rec)
    venv.env.step(1)
    venv.ddpg_replay_push(rec)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / calls

    act_us, push_us, step_us = [], [], []
    for _ in range(reps):
        act_us.append(timed(lambda: venv.ddpg_act(rec)))
        push_us.append(timed(lambda: venv.ddpg_replay_push(rec)))
        step_us.append(timed(lambda: venv.env.step(1)))
    venv.close()
    return {"agents": N, "calls": calls, "act_us_per_call": stats(act_us), "push_us_per_call": stats(push_us), "step_us_per_call": stats(step_us)}


def example(path, episodes=5, agents=1024):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ddpg_racer.py"), "--agents", str(agents), "--episodes", str(episodes),
                          "--max-steps", "1000", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, cwd=ROOT)
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.startswith(("episode", "largest"))]
    return {"returncode": out.returncode, "lines": lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "ddpg", "ddpg_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-example", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Silverstone", "rays": 5, "iterations": ITERATIONS, "reps": args.reps,
           "update": update(args.reps), "act_push": act_and_push_against_step(args.reps)}
    if not args.skip_example:
        res["example"] = {path: example(path) for path in ("--device-update", "--torch-update")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
