"""Guided cost learning racers on the device environment: the reference's RLRacers/GuidedCostLearning app (main.cpp:114-187, GCLAgent.hpp,
Networks.hpp, ReadExpertData.hpp) for N agents that share the 7-64-64-2 policy, the 7-64-64-1 value and the 9-64-64-1 cost network.

    python examples/gcl_racer.py [--agents 1024] [--episodes 20] [--track Silverstone] [--steps 32] [--expert-steps 64]
                                 [--device-update [--graph-chunk 8]] [--bc-init] [--greedy-eval]

The expert is recorded once with the potential-field collector on the device (7 rays, lookahead 2, 10 degree clamp: what the reference's
loader reads from disk).  Per episode (main.cpp:150-187): a rollout of --steps steps; one Adam step of the cost network on
BCEWithLogits(c_expert, 0) + BCEWithLogits(c_policy, 1) with as many uniform expert draws as policy samples; a second rollout whose
reward is -cost under the network just stepped; discounted returns (gamma 0.99; a crashed agent is re-placed and its episode ends
there); updatePolicy: normalised advantages G - V(x), the clipped surrogate on the recorded pre-squash sample, the value network's
squared error, one Adam step each, lr 3e-4 throughout.

--device-update: everything stays on the device: okenv_gcl_act acts and records, rollout.gcl_cost_update,
rollout.gcl_rewards, rollout.prepare_gcl_batch and rollout.gcl_policy_update do the rest in place in the parameters the device acts
with; the modules receive them at the end.  Without it the same loop runs in PyTorch with the same modules.
--bc-init: the reference's commented-out warm start, in PyTorch: the policy's mean regressed on the expert's actions for a few epochs.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.demonstrations import collect_demonstrations  # noqa: E402
from openkitchen_amd.rollout import (collect_episode_gcl, gcl_cost_update, gcl_expert_rows, gcl_policy_update, gcl_rewards,  # noqa: E402
                                     prepare_gcl_batch)
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

SCALE, BIAS = (50.0, 10.0), (50.0, 0.0)  # (a_0 + 1) / 2 * 100 and a_1 * 10 (GCLAgent.hpp:64-72)


class PolicyNet(torch.nn.Module):
    def __init__(self, rays=7, hidden=64):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(rays, hidden), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, 2)
        self.log_std = torch.nn.Parameter(torch.zeros(2))

    def forward(self, x):
        return torch.tanh(self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x))))))


class ValueNet(torch.nn.Module):
    def __init__(self, rays=7, hidden=64):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(rays, hidden), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, 1)

    def forward(self, x):
        return self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x))))).squeeze(1)


class CostNet(torch.nn.Module):
    def __init__(self, rays=7, hidden=64):
        super().__init__()
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(rays + 2, hidden), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, 1)
        self.fc3.weight.data.mul_(0.1)
        self.fc3.bias.data.mul_(0.0)

    def forward(self, s, a):
        return self.fc3(torch.tanh(self.fc2(torch.tanh(self.fc1(torch.cat([s, a], 1)))))).squeeze(1)


def log_prob(policy, mu, pre):
    z = (pre - mu) / torch.exp(policy.log_std)
    return -0.5 * ((z * z).sum(1) + 2.0 * policy.log_std.sum() + 2.0 * math.log(2.0 * math.pi))


def torch_rollout(venv, policy, steps, greedy=False):
    """GCLAgent.hpp:102-135 with the module acting, auto-reset re-placing crashed agents."""
    scale, bias = (torch.tensor(v, dtype=torch.float32, device=venv.device) for v in (SCALE, BIAS))
    venv.reset()
    rows = {k: [] for k in ("states", "pre", "squashed", "log_probs", "alive")}
    with torch.no_grad():
        for _ in range(steps):
            x = (venv.rel_x * venv.rel_x + venv.rel_y * venv.rel_y) / 40000.0
            mu = policy(x)
            pre = mu if greedy else mu + torch.exp(policy.log_std) * torch.randn_like(mu)
            a = torch.tanh(pre)
            for k, v in (("states", x), ("pre", pre), ("squashed", a), ("log_probs", log_prob(policy, mu, pre)), ("alive", ~venv.done.clone())):
                rows[k].append(v)
            venv.step(a * scale + bias)
    return {k: torch.stack(v) for k, v in rows.items()}


def torch_returns(rewards, alive, gamma):
    out, c = torch.zeros_like(rewards), torch.zeros_like(rewards[0])
    for t in range(rewards.shape[0] - 1, -1, -1):
        c = torch.where(alive[t], rewards[t] + gamma * c, torch.zeros_like(c))
        out[t] = c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--steps", type=int, default=32, help="steps per rollout (the reference: 2048 samples of one agent)")
    ap.add_argument("--expert-steps", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-update", action="store_true", help="act, cost update, rewards, batch and policy / value update on the device")
    ap.add_argument("--graph-chunk", type=int, default=8, help="with --device-update: iterations per replayed HIP graph (0: eager)")
    ap.add_argument("--bc-init", action="store_true", help="behavioural-cloning warm start of the policy's mean, in PyTorch")
    ap.add_argument("--greedy-eval", action="store_true", help="one more rollout at the end with pre = mu")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    rays = np.linspace(-90, 90, 7).astype(np.float32)
    venv = VectorEnvironment(args.track, args.agents, ray_angles_deg=rays, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=args.seed)
    lr, gamma, clip = 3e-4, 0.99, 0.2
    policy, value, cost = PolicyNet().cuda(), ValueNet().cuda(), CostNet().cuda()
    # the expert, once (ReadExpertData.hpp reads what this collector writes)
    venv.enable_expert("potfield", lookahead=2, goal_wrap=False, clamp_deg=10.0)
    demos = collect_demonstrations(venv, args.expert_steps, seed=args.seed)
    bank_state, bank_action = gcl_expert_rows(demos)
    print("expert bank: %d rows" % bank_state.shape[0], flush=True)
    if args.bc_init:
        bc = torch.optim.Adam(policy.parameters(), lr=1e-3)
        for epoch in range(20):
            loss = torch.nn.functional.mse_loss(policy(bank_state), bank_action)
            bc.zero_grad()
            loss.backward()
            bc.step()
        print("bc-init: mse %.5f" % float(loss), flush=True)
    opts = {"policy": torch.optim.Adam(policy.parameters(), lr=lr), "value": torch.optim.Adam(value.parameters(), lr=lr),
            "cost": torch.optim.Adam(cost.parameters(), lr=lr)}
    if args.device_update:
        venv.enable_gcl(policy, value, cost, scale=SCALE, bias=BIAS)
        venv.enable_gcl_learner(lr=lr, clip=clip, cost_lr=lr)
        venv.set_gcl_expert(demos)
    for episode in range(args.episodes):
        t0 = time.perf_counter()
        if args.device_update:
            ep = collect_episode_gcl(venv, args.steps, graph_chunk=args.graph_chunk)
            cost_loss = gcl_cost_update(venv, ep)["loss"]
            ep = collect_episode_gcl(venv, args.steps, graph_chunk=args.graph_chunk)
            batch = prepare_gcl_batch(venv, ep, gcl_rewards(venv, ep), gamma=gamma)
            out = gcl_policy_update(venv, batch)
            policy_loss, value_loss, samples = out["policy_loss"], out["value_loss"], batch["count"]
        else:
            ep = torch_rollout(venv, policy, args.steps)
            keep = ep["alive"].reshape(-1)
            xs, acts = ep["states"].reshape(keep.numel(), -1)[keep], ep["squashed"].reshape(-1, 2)[keep]
            rows = torch.randint(bank_state.shape[0], (xs.shape[0],), device=xs.device)
            bce = torch.nn.functional.binary_cross_entropy_with_logits
            c_e, c_p = cost(bank_state[rows], bank_action[rows]), cost(xs, acts)
            cost_loss = (bce(c_e, torch.zeros_like(c_e)) + bce(c_p, torch.ones_like(c_p))).reshape(1)
            opts["cost"].zero_grad()
            cost_loss.backward()
            opts["cost"].step()
            ep = torch_rollout(venv, policy, args.steps)
            T, N = ep["alive"].shape
            with torch.no_grad():
                rewards = -cost(ep["states"].reshape(T * N, -1), ep["squashed"].reshape(T * N, 2)).reshape(T, N)
            keep = ep["alive"].reshape(-1)
            G = torch_returns(rewards, ep["alive"], gamma).reshape(-1)[keep]
            xs, pre, old = ep["states"].reshape(T * N, -1)[keep], ep["pre"].reshape(-1, 2)[keep], ep["log_probs"].reshape(-1)[keep]
            v = value(xs)
            adv = G - v.detach()
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            ratio = torch.exp(log_prob(policy, policy(xs), pre) - old)
            policy_loss = (-torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()).reshape(1)
            value_loss = torch.nn.functional.mse_loss(v, G).reshape(1)
            for name, loss in (("policy", policy_loss), ("value", value_loss)):
                opts[name].zero_grad()
                loss.backward()
                opts[name].step()
            samples = int(keep.sum())
        torch.cuda.synchronize()
        print("episode %3d: %7d samples, cost loss %9.5f, policy loss %10.6f, value loss %10.5f, alive %5.1f %%, %.3f s" % (
            episode, samples, float(cost_loss.detach()[0]), float(policy_loss.detach()[0]), float(value_loss.detach()[0]), 100.0 * float(ep["alive"].float().mean()),
            time.perf_counter() - t0), flush=True)
    if args.device_update:
        venv.pull_gcl()
    if args.greedy_eval:
        if args.device_update:
            venv.set_gcl_greedy(True)
            ep = collect_episode_gcl(venv, args.steps, graph_chunk=0)
        else:
            ep = torch_rollout(venv, policy, args.steps, greedy=True)
        print("greedy: alive %5.1f %%" % (100.0 * float(ep["alive"].float().mean())), flush=True)
    finite = all(bool(torch.isfinite(p).all()) for m in (policy, value, cost) for p in m.parameters())
    print("mean std %.4f, parameters finite %s" % (float(torch.exp(policy.log_std.detach()).mean()), finite), flush=True)
    venv.close()
    return 0 if finite else 1


if __name__ == "__main__":
    sys.exit(main())
