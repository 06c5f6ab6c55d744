"""The continuous REINFORCE learner: okenv_gauss_act beside a step launch, the PyTorch update of
examples/reinforce_continuous_racer.py's module against rollout.reinforce_continuous_update on the same batch, and the device time of
the update's kernels.

    python tools/gauss_bench.py [--out profiles/gauss/gauss_bench.json] [--reps 9] [--max-steps 1000]

One episode per population (1024 and 4096 agents) is recorded once by collect_episode_gauss on Silverstone with the reference's
5-128-128-2 network (log_std 2.5), turned into the batch by prepare_gauss_batch and reused.  (a) okenv_gauss_act, recording, and
okenv_step: wall-clock time of 200 calls each between two device synchronisations, per call.  (b) one batched PyTorch update of the
same module on that batch -- ONE forward over all M states with the recorded eps, the reference's log_prob with pre left in the graph,
the loss sum of -(log_prob * return), one backward pass and one Adam step -- against rollout.reinforce_continuous_update with the
reference's choices (accumulate, sum, grad "reference") and the default slice: wall-clock times between two device synchronisations,
alternated, median / min / max of --reps repetitions after one warm-up of each; both keep stepping their own parameters.  (c) comes
from the events okenv_gauss_update records around its kernels while okenv_set_timing is on, in repetitions of their own."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd.rollout import collect_episode_gauss, prepare_gauss_batch, reinforce_continuous_update  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
LR, SLICE, CALLS = 1e-3, 16384, 200


class Policy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log_std = torch.nn.Parameter(torch.full((2,), 2.5))
        self.fc1, self.fc2, self.mean = torch.nn.Linear(5, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 2)

    def forward(self, x):
        return self.mean(torch.relu(self.fc2(torch.relu(self.fc1(x)))))


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def per_call_us(fn, reps):
    fn()
    return stats([wall(lambda: [fn() for _ in range(CALLS)]) * 1e3 / CALLS for _ in range(reps)])


def population(N, reps, max_steps):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=False, seed=0)
    torch.manual_seed(0)
    policy = Policy().cuda()
    opt = torch.optim.Adam(policy.parameters(), lr=LR)
    venv.enable_gauss_actor(policy)
    venv.enable_gauss_learner(lr=LR)
    ep = collect_episode_gauss(venv, max_steps=max_steps, graph_chunk=32)
    data = prepare_gauss_batch(venv, ep, gamma=0.99, normalize="returns")
    M = data["count"]
    states, eps, ret = data["states"], data["eps"], data["returns"]

    def torch_update():
        mu = policy(states)
        std = torch.exp(policy.log_std)
        pre = mu + std * eps
        logp = (-0.5 * ((pre - mu) / std) ** 2 - torch.log(std) - 0.5 * math.log(2.0 * math.pi)).sum(1) - torch.log(1.0 - torch.tanh(pre) ** 2 + 1e-6).sum(1)
        loss = (-(logp * ret)).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()

    device = lambda: reinforce_continuous_update(venv, data, slice=SLICE)  # noqa: E731
    torch_update()
    device()
    a_ms, b_ms = [], []
    for _ in range(reps):  # alternated: both see the same machine
        a_ms.append(wall(torch_update))
        b_ms.append(wall(device))
    venv.env.set_timing(True)
    per_kernel = {k: [] for k in capi.GAUSS_KERNELS}
    for _ in range(reps):
        device()
        for k, v in venv.env.gauss_timing().items():
            per_kernel[k].append(v)
    venv.env.set_timing(False)
    rec = {"state": torch.empty((N, 5), device="cuda"), "eps": torch.empty((N, 2), device="cuda"), "pre": torch.empty((N, 2), device="cuda"),
           "action": torch.empty((N, 2), device="cuda"), "logp": torch.empty(N, device="cuda"), "alive": torch.empty(N, dtype=torch.uint8, device="cuda")}
    venv.reset()
    calls = {"gauss_act_us": per_call_us(lambda: venv.gauss_act(None), reps), "gauss_act_recording_us": per_call_us(lambda: venv.gauss_act(rec), reps),
             "step_us": per_call_us(lambda: venv.env.step(1), reps)}
    slices = (M + SLICE - 1) // SLICE
    kernels = {k: {"us_per_update": stats(per_kernel[k]), "us_per_slice": stats(per_kernel[k])["median"] / slices} for k in capi.GAUSS_KERNELS}
    a, b = stats(a_ms), stats(b_ms)
    venv.close()
    return {"T": int(ep["alive"].shape[0]), "M": M, "slices": slices, "calls": calls, "torch_ms": a, "reinforce_continuous_update_ms": b,
            "ratio_of_medians": a["median"] / b["median"], "device_path_is_faster": b["median"] < a["median"], "kernels": kernels,
            "kernel_sum_us": sum(kernels[k]["us_per_update"]["median"] for k in kernels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gauss", "gauss_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-steps", type=int, default=1000)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Silverstone", "rays": 5, "network": "5-128-128-2", "log_std": 2.5, "slice": SLICE,
           "reps": args.reps, "max_steps": args.max_steps, "calls_per_region": CALLS,
           "populations": {str(N): population(N, args.reps, args.max_steps) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
