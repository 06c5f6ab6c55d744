"""REINFORCE's update: the PyTorch update of examples/reinforce_racer.py against rollout.reinforce_update on the
same batch, and the device time of the kernels.

    python tools/reinforce_bench.py [--out profiles/reinforce/reinforce_bench.json] [--reps 9]

One episode per population is recorded once by collect_episode_device (dropout 0.6) on Silverstone, turned into the batch by
prepare_batch and reused.  (a) is the example's PyTorch update on that batch: ONE forward of the module with nn.Dropout over all M
states, the loss sum of -log p(a) * return, one backward pass and one Adam step (the example itself keeps the graphs of its T per-step
forwards instead, which costs more).  (b) is rollout.reinforce_update with the reference's choices (accumulate, sum) and the default
slice.  Both are wall-clock times between two device synchronisations, alternated, median / min / max of --reps repetitions after one
warm-up of each; both keep stepping their own parameters.  (c) comes from the events okenv_reinforce_update records around its
kernels while okenv_set_timing is on, in repetitions of their own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd.rollout import collect_episode_device, prepare_batch, reinforce_update  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
LR, DROPOUT, SLICE = 0.01, 0.6, 16384


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
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=False, seed=0, reward="step")
    torch.manual_seed(0)
    affine1, affine2 = torch.nn.Linear(5, 128).cuda(), torch.nn.Linear(128, 3).cuda()
    policy = torch.nn.Sequential(affine1, torch.nn.Dropout(DROPOUT), torch.nn.ReLU(), affine2, torch.nn.Softmax(dim=1)).train()
    opt = torch.optim.Adam(policy.parameters(), lr=LR)
    venv.enable_actor([affine1.weight, affine1.bias, affine2.weight, affine2.bias])
    venv.enable_learner(lr=LR)
    venv.set_actor_dropout(DROPOUT)
    ep = collect_episode_device(venv, max_steps=3000, graph_chunk=32)
    data = prepare_batch(venv, ep, gamma=0.99, normalize="returns")
    M = data["count"]
    states, actions, ret = data["states"], data["actions"].unsqueeze(1), data["returns"]

    def torch_update():
        loss = (-torch.log(policy(states).gather(1, actions)).squeeze(1) * ret).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()

    device = lambda: reinforce_update(venv, data, slice=SLICE)  # noqa: E731
    torch_update()
    device()
    a_ms, b_ms = [], []
    for _ in range(reps):  # alternated: both see the same machine
        a_ms.append(wall(torch_update))
        b_ms.append(wall(device))
    venv.env.set_timing(True)
    per_kernel = {k: [] for k in capi.REINFORCE_KERNELS}
    for _ in range(reps):
        device()
        for k, v in venv.env.reinforce_timing().items():
            per_kernel[k].append(v)
    venv.env.set_timing(False)
    slices = (M + SLICE - 1) // SLICE
    kernels = {k: {"us_per_update": stats(per_kernel[k]), "us_per_slice": stats(per_kernel[k])["median"] / slices} for k in capi.REINFORCE_KERNELS}
    a, b = stats(a_ms), stats(b_ms)
    venv.close()
    return {"T": int(ep["alive"].shape[0]), "M": M, "slices": slices, "torch_ms": a, "reinforce_update_ms": b, "ratio_of_medians": a["median"] / b["median"],
            "device_path_is_faster": b["median"] < a["median"], "kernels": kernels,
            "kernel_sum_us": sum(kernels[k]["us_per_update"]["median"] for k in kernels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "reinforce", "reinforce_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Silverstone", "rays": 5, "dropout": DROPOUT, "slice": SLICE, "reps": args.reps,
           "populations": {str(N): population(N, args.reps) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
