"""PPO's update: the parent's PyTorch minibatch loop against rollout.ppo_update on the same batch, and the
device time of the two kernels.

    python tools/update_bench.py [--out profiles/update/update_bench.json] [--reps 9]

One episode per population is recorded once by collect_episode_device on Silverstone, turned into the batch by prepare_batch and
reused.  (a) is the update loop of examples/ppo_racer.py as the parent has it (five epochs of 4096-sample minibatches, two forwards,
two backward passes and two Adam steps each), (b) rollout.ppo_update with the same epochs and minibatch size.  Both are wall-clock
times between two device synchronisations, alternated, median / min / max of --reps repetitions after one warm-up of each; both keep
stepping their own parameters from repetition to repetition, as successive episodes do.  (c) comes from the events okenv_ppo_update
records around its kernels while okenv_set_timing is on, in repetitions of their own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd.rollout import collect_episode_device, ppo_update, prepare_batch  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
CLIP, EPOCHS, BATCH = 0.2, 5, 4096


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def parent_update(actor, critic, opt_a, opt_c, states, actions, old_logp, ret):
    """examples/ppo_racer.py without --device-update, as it is."""
    for _ in range(EPOCHS):
        perm = torch.randperm(states.shape[0], device=states.device)
        for i in range(0, states.shape[0], BATCH):
            j = perm[i:i + BATCH]
            values = critic(states[j])
            adv = ret[j] - values.detach()
            probs = torch.clamp(actor(states[j]), 1e-8, 1 - 1e-8)
            ratio = torch.exp(torch.log(probs.gather(1, actions[j])) - old_logp[j])
            actor_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()
            critic_loss = torch.nn.functional.mse_loss(values, ret[j])
            opt_a.zero_grad()
            actor_loss.backward()
            opt_a.step()
            opt_c.zero_grad()
            critic_loss.backward()
            opt_c.step()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def population(N, reps):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=False, seed=0, reward="step")
    torch.manual_seed(0)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3), torch.nn.Softmax(dim=1)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    opt_a = torch.optim.Adam(actor.parameters(), lr=3e-4)
    opt_c = torch.optim.Adam(critic.parameters(), lr=3e-4)
    venv.enable_actor(actor, critic)
    venv.enable_learner(lr=3e-4, clip=CLIP)
    ep = collect_episode_device(venv, max_steps=3000, graph_chunk=32)
    data = prepare_batch(venv, ep, gamma=0.99, normalize="returns")
    M = data["count"]
    states, actions, old_logp, ret = data["states"], data["actions"].unsqueeze(1), data["log_probs"].unsqueeze(1), data["returns"].unsqueeze(1)
    parent = lambda: parent_update(actor, critic, opt_a, opt_c, states, actions, old_logp, ret)  # noqa: E731
    device = lambda: ppo_update(venv, data, epochs=EPOCHS, minibatch=BATCH, shuffle=True)  # noqa: E731
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
        for k, v in venv.env.update_timing().items():
            per_kernel[k].append(v)
    venv.env.set_timing(False)
    minibatches = EPOCHS * ((M + BATCH - 1) // BATCH)
    kernels = {k: {"us_per_update": stats(per_kernel[k]), "us_per_minibatch": stats(per_kernel[k])["median"] / minibatches} for k in capi.UPDATE_KERNELS}
    a, b = stats(a_ms), stats(b_ms)
    venv.close()
    return {"T": int(ep["alive"].shape[0]), "M": M, "minibatches": minibatches, "parent_ms": a, "ppo_update_ms": b,
            "ratio_of_medians": a["median"] / b["median"], "parent_spread_ms": a["max"] - a["min"], "gain_ms": a["median"] - b["median"],
            "faster_by_more_than_the_parent_spread": (a["median"] - b["median"]) > (a["max"] - a["min"]), "kernels": kernels,
            "kernel_sum_us": sum(kernels[k]["us_per_update"]["median"] for k in kernels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "update", "update_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Silverstone", "rays": 5, "epochs": EPOCHS, "minibatch": BATCH, "reps": args.reps,
           "populations": {str(N): population(N, args.reps) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
