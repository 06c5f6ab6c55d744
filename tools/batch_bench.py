"""From a recorded episode to the learner's batch: the parent's torch path against rollout.prepare_batch on
the same episode, and the device time and traffic of each of the five kernels.

    python tools/batch_bench.py [--out profiles/batch/batch_bench.json] [--reps 9]

One episode per population is recorded once by collect_episode_device on Silverstone and reused.  (a) and (b) are wall-clock times
between two device synchronisations, alternated, median / min / max of --reps repetitions after one warm-up of each; (c) comes from
the events okenv_batch_prepare records between its kernels while okenv_set_timing is on, in repetitions of their own.  The bytes are
what the algorithm has to move, computed from T, N, R and M."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd.rollout import collect_episode_device, discounted_returns, prepare_batch  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def parent_path(ep):
    """examples/ppo_racer.py without --device-batch, as it is."""
    alive = ep["alive"]
    returns = discounted_returns(ep["rewards"] * alive)
    mask = alive.reshape(-1)
    states = ep["states"].reshape(-1, 5)[mask]
    actions = ep["actions"].reshape(-1, 1)[mask]
    old_logp = ep["log_probs"].reshape(-1, 1)[mask]
    ret = returns.reshape(-1, 1)[mask]
    return states, actions, old_logp, ret


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_bytes(T, N, R, M):
    """Bytes each kernel has to move (reads + writes) for the outputs prepare_batch asks for without a value plane."""
    chunks = T * ((N + 63) // 64)
    groups = (chunks + 15) // 16
    return {"walk": T * N * (4 + 1 + 4) + N * 36, "tree": N * 36 * 2, "count": T * N + groups * 4, "scan": groups * 8,
            "gather": T * N + groups * 4 + M * (4 + 2 * 8 + 2 * 4 + 2 * 4 + 2 * 4 * R)}


def population(N, reps):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=False, seed=0, reward="step")
    torch.manual_seed(0)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3), torch.nn.Softmax(dim=1)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    venv.enable_actor(actor, critic)
    ep = collect_episode_device(venv, max_steps=3000, graph_chunk=32)
    T = int(ep["alive"].shape[0])
    device = lambda: prepare_batch(venv, ep, gamma=0.99, normalize="returns")  # noqa: E731
    M = device()["count"]
    parent_path(ep)
    a_ms, b_ms = [], []
    for _ in range(reps):  # alternated: both see the same machine
        a_ms.append(wall(lambda: parent_path(ep)))
        b_ms.append(wall(device))
    venv.env.set_timing(True)
    per_kernel = {k: [] for k in capi.BATCH_KERNELS}
    for _ in range(reps):
        device()
        for k, v in venv.env.batch_timing().items():
            per_kernel[k].append(v)
    venv.env.set_timing(False)
    nbytes = kernel_bytes(T, N, 5, M)
    kernels = {}
    for k in capi.BATCH_KERNELS:
        s = stats(per_kernel[k])
        gbs = nbytes[k] / (s["median"] * 1e-6) / 1e9
        kernels[k] = {"us": s, "bytes": nbytes[k], "GB_per_s": gbs, "share_of_hbm_peak": gbs / HBM_PEAK_GBS}
    a, b = stats(a_ms), stats(b_ms)
    venv.close()
    return {"T": T, "M": M, "parent_ms": a, "prepare_batch_ms": b, "ratio_of_medians": a["median"] / b["median"],
            "parent_spread_ms": a["max"] - a["min"], "gain_ms": a["median"] - b["median"],
            "faster_by_more_than_the_parent_spread": (a["median"] - b["median"]) > (a["max"] - a["min"]), "kernels": kernels,
            "kernel_sum_us": sum(kernels[k]["us"]["median"] for k in kernels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "batch", "batch_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Silverstone", "rays": 5, "gamma": 0.99, "reps": args.reps,
           "hbm_peak_GB_per_s": HBM_PEAK_GBS, "populations": {str(N): population(N, args.reps) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
