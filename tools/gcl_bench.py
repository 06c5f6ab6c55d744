"""Guided cost learning: okenv_gcl_act beside a step launch, and the cost update and the policy / value update
on the device against one batched PyTorch forward / backward / Adam step of the same modules on the same data.

    python tools/gcl_bench.py [--out profiles/gcl/gcl_bench.json] [--reps 5] [--steps 32]

Per population (1024 and 4096 agents) one rollout of --steps steps is recorded once by collect_episode_gcl on Silverstone with the
reference's 7-64-64 networks and reused.  Every figure is the time between two HIP events on the environment's stream around the
region, median / min / max of --reps repetitions after one warm-up: (a) 200 calls of okenv_gcl_act, recording, and of okenv_step, per
call; (b) rollout.gcl_cost_update against BCEWithLogits on the same rows (the expert rows drawn with torch.randint); (c)
rollout.gcl_policy_update with the reference's choices (one step on the mean) against updatePolicy written in PyTorch; both sides keep
stepping their own parameters.  The per-kernel times come from okenv_debug_gcl_timing in repetitions of their own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
from gcl_racer import CostNet, PolicyNet, ValueNet, log_prob  # noqa: E402
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd.demonstrations import collect_demonstrations  # noqa: E402
from openkitchen_amd.rollout import collect_episode_gcl, gcl_cost_update, gcl_policy_update, gcl_rewards, prepare_gcl_batch  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.linspace(-90, 90, 7).astype(np.float32)
LR, CLIP, CALLS = 3e-4, 0.2, 200


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


def timed(fn, reps):
    fn()
    return stats([event_ms(fn) for _ in range(reps)])


def population(N, reps, steps):
    venv = VectorEnvironment("Silverstone", N, ray_angles_deg=RAYS, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=0)
    torch.manual_seed(0)
    policy, value, cost = PolicyNet().cuda(), ValueNet().cuda(), CostNet().cuda()
    opts = {k: torch.optim.Adam(m.parameters(), lr=LR) for k, m in (("policy", policy), ("value", value), ("cost", cost))}
    venv.enable_gcl(policy, value, cost)
    venv.enable_gcl_learner(lr=LR, clip=CLIP, cost_lr=LR)
    venv.enable_expert("potfield", lookahead=2, goal_wrap=False, clamp_deg=10.0)
    E = venv.set_gcl_expert(collect_demonstrations(venv, 32, seed=0))
    bank_state, bank_action = venv._gcl_bank
    ep = collect_episode_gcl(venv, steps, graph_chunk=8)
    keep = ep["alive"].reshape(-1)
    xs, acts = ep["states"].reshape(keep.numel(), -1)[keep].contiguous(), ep["squashed"].reshape(-1, 2)[keep].contiguous()
    batch = prepare_gcl_batch(venv, ep, gcl_rewards(venv, ep))
    M = batch["count"]
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def torch_cost():
        rows = torch.randint(E, (xs.shape[0],), device=xs.device)
        c_e, c_p = cost(bank_state[rows], bank_action[rows]), cost(xs, acts)
        loss = bce(c_e, torch.zeros_like(c_e)) + bce(c_p, torch.ones_like(c_p))
        opts["cost"].zero_grad()
        loss.backward()
        opts["cost"].step()

    def torch_policy():
        G, x = batch["returns"], batch["states"]
        v = value(x)
        adv = G - v.detach()
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(log_prob(policy, policy(x), batch["pre"]) - batch["log_probs"])
        loss_pi = -torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()
        loss_v = torch.nn.functional.mse_loss(v, G)
        for name, loss in (("policy", loss_pi), ("value", loss_v)):
            opts[name].zero_grad()
            loss.backward()
            opts[name].step()

    res = {"T": steps, "expert_rows": E, "policy_rows": int(xs.shape[0]), "M": M}
    pairs = {"cost_update": (torch_cost, lambda: gcl_cost_update(venv, ep)), "policy_value_update": (torch_policy, lambda: gcl_policy_update(venv, batch))}
    for name, (in_torch, on_device) in pairs.items():
        a, b = timed(in_torch, reps), timed(on_device, reps)
        res[name] = {"torch_ms": a, "device_ms": b, "ratio_of_medians": a["median"] / b["median"], "device_path_is_faster": b["median"] < a["median"]}
    venv.env.set_timing(True)
    kernels = {}
    for which, fn in (("cost", pairs["cost_update"][1]), ("policy", pairs["policy_value_update"][1]), ("value", pairs["policy_value_update"][1])):
        per = {k: [] for k in capi.GCL_KERNELS}
        for _ in range(reps):
            fn()
            for k, v in venv.env.gcl_timing(which).items():
                per[k].append(v)
        kernels[which] = {k: stats(v) for k, v in per.items()}
    venv.env.set_timing(False)
    res["kernels_us"] = kernels
    rec = {k: torch.empty((N, 2), device="cuda") for k in ("eps", "pre", "squashed", "action")}
    rec.update(state=torch.empty((N, 7), device="cuda"), logp=torch.empty(N, device="cuda"), alive=torch.empty(N, dtype=torch.uint8, device="cuda"))
    venv.reset()
    per_call = lambda fn: {k: v * 1e3 / CALLS for k, v in timed(lambda: [fn() for _ in range(CALLS)], reps).items()}  # noqa: E731
    res["calls_us"] = {"gcl_act": per_call(lambda: venv.gcl_act(None)), "gcl_act_recording": per_call(lambda: venv.gcl_act(rec)),
                       "step": per_call(lambda: venv.env.step(1))}
    venv.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gcl", "gcl_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Silverstone", "rays": 7, "networks": "policy 7-64-64-2, value 7-64-64-1, cost 9-64-64-1",
           "reps": args.reps, "steps": args.steps, "calls_per_region": CALLS,
           "populations": {str(N): population(N, args.reps, args.steps) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
