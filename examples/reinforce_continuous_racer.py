"""Continuous REINFORCE racers on the device environment: the reference's RLRacers/ReinforceContinuous app (reinforce_sim.cpp:46-108,
ReinforceAgent.hpp, Policy.hpp) for N agents that share the 5-128-128-2 network with its Gaussian head and learned log_std.

    python examples/reinforce_continuous_racer.py [--agents 1024] [--episodes 20] [--track Silverstone] [--grad reference|score]
                                                  [--device-update [--graph-chunk 32]] [--greedy-eval]

Per episode (reinforce_sim.cpp:52-105): resetAgent to random centre-line points, one observation step, then act / step until every
agent has crashed; the action is tanh(mu + exp(log_std) * eps) scaled to throttle in [0, 100] and steering in [-10, 10]; the reward is
the distance moved in the step (prev_pos refreshed every step) and -5 on the crashing step.  Then
ReinforceAgent::updatePolicy (ReinforceAgent.hpp:96-135): discounted returns (gamma 0.99, normalised), the loss sum of
-log_prob * return, one Adam step with lr 1e-3.

--grad reference keeps the pre-tanh sample in the graph, as the reference does: every gradient then flows through the tanh correction
and the Gaussian term gives the mean none.  --grad score detaches it: the score-function estimator.

--device-update: the whole episode stays on the device (DESIGN.md sections 15 and 20): okenv_gauss_act acts and records,
rollout.prepare_gauss_batch builds the training set, rollout.reinforce_continuous_update computes loss and gradient and takes the
Adam step in place in the parameters the device actor acts with; the torch module receives them after every episode only to print
exp(log_std).  Without it the plain PyTorch loop runs with the same module.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.rollout import (collect_episode_gauss, discounted_returns, prepare_gauss_batch,  # noqa: E402
                                     reinforce_continuous_update)
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402


class Policy(torch.nn.Module):
    """Policy.hpp:17-53: fc1 -> relu -> fc2 -> relu -> mean, and the free parameter log_std (2.5; kEnableLogStdHead is false)."""

    def __init__(self, rays=5, hidden=128, log_std=2.5):
        super().__init__()
        self.log_std = torch.nn.Parameter(torch.full((2,), float(log_std)))
        self.fc1 = torch.nn.Linear(rays, hidden)
        self.fc2 = torch.nn.Linear(hidden, hidden)
        self.mean = torch.nn.Linear(hidden, 2)

    def forward(self, x):
        return self.mean(torch.relu(self.fc2(torch.relu(self.fc1(x)))))


SCALE, BIAS = (50.0, 10.0), (50.0, 0.0)  # ((t_0 + 1) * 0.5) * 100 and t_1 * 10 (ReinforceAgent.hpp:85-88)


def log_prob(policy, mu, pre, detach):
    """ReinforceAgent.hpp:76-83; detach=False leaves pre in the graph, as the reference does."""
    std = torch.exp(policy.log_std)
    z = ((pre.detach() if detach else pre) - mu) / std
    t = torch.tanh(pre.detach() if detach else pre)
    return (-0.5 * z * z - torch.log(std) - 0.5 * math.log(2.0 * math.pi)).sum(1) - torch.log(1.0 - t * t + 1e-6).sum(1)


def torch_episode(venv, policy, max_steps, detach, greedy=False, check_every=8, crash_reward=-5.0):
    """reinforce_sim.cpp:52-105 with the module acting: the log-probabilities keep their graphs, as saved_log_probs do."""
    scale, bias = (torch.tensor(v, dtype=torch.float32, device=venv.device) for v in (SCALE, BIAS))
    venv.reset()
    logps, rewards, alive = [], [], []
    steps = 0
    while True:
        mu = policy(venv.observation())
        pre = mu if greedy else mu + torch.exp(policy.log_std) * torch.randn_like(mu)
        logps.append(log_prob(policy, mu, pre, detach))
        alive.append(~venv.done.clone())
        px, py = venv.pos_x.clone(), venv.pos_y.clone()
        venv.step(torch.tanh(pre.detach()) * scale + bias)
        moved = torch.sqrt((venv.pos_x - px) ** 2 + (venv.pos_y - py) ** 2)
        rewards.append(moved.masked_fill(venv.done, crash_reward))
        steps += 1
        if steps % check_every == 0 and venv.env.alive_count() == 0:
            break
        if steps >= max_steps:
            break
    alive = torch.stack(alive)
    T = max(1, int(alive.any(dim=1).sum()))
    return {"log_probs": torch.stack(logps)[:T], "rewards": torch.stack(rewards)[:T], "alive": alive[:T]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--max-steps", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-std", type=float, default=2.5)               # Policy.hpp: log_std's initial value
    ap.add_argument("--grad", choices=("reference", "score"), default="reference")
    ap.add_argument("--device-update", action="store_true", help="act, batch and update on the device (rollout.reinforce_continuous_update)")
    ap.add_argument("--graph-chunk", type=int, default=32, help="with --device-update: iterations per replayed HIP graph (0: eager)")
    ap.add_argument("--greedy-eval", action="store_true", help="one more episode at the end with tanh(mu) (ReinforceAgent.hpp:137-146)")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    rays = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
    venv = VectorEnvironment(args.track, args.agents, ray_angles_deg=rays, auto_reset=False, seed=args.seed)
    lr, gamma = 1e-3, 0.99                                              # ReinforceAgent.hpp: kLearningRate, kGamma
    policy = Policy(log_std=args.log_std).cuda()
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    if args.device_update:
        venv.enable_gauss_actor(policy, scale=SCALE, bias=BIAS)
        venv.enable_gauss_learner(lr=lr)
    lengths = torch.zeros(1)
    for episode in range(args.episodes + (1 if args.greedy_eval else 0)):
        evaluate = episode == args.episodes
        t0 = time.perf_counter()
        if args.device_update:
            venv.set_gauss_greedy(evaluate)
            ep = collect_episode_gauss(venv, max_steps=args.max_steps, graph_chunk=args.graph_chunk)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            loss, samples = torch.zeros(1), int(ep["alive"].sum())
            if not evaluate:
                data = prepare_gauss_batch(venv, ep, gamma=gamma, normalize="returns")
                loss = reinforce_continuous_update(venv, data, grad=args.grad)["loss"]
                venv.pull_gauss()
        else:
            ep = torch_episode(venv, policy, args.max_steps, args.grad == "score", greedy=evaluate)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            mask = ep["alive"].reshape(-1)
            loss, samples = torch.zeros(1), int(mask.sum())
            if not evaluate:
                returns = discounted_returns(ep["rewards"].detach() * ep["alive"], gamma, normalize=False).reshape(-1)[mask]
                returns = (returns - returns.mean()) / (returns.std() + torch.finfo(torch.float32).eps)
                loss = (-ep["log_probs"].reshape(-1)[mask] * returns).sum().reshape(1)   # loss += -(log_prob * G)
                opt.zero_grad()
                loss.backward()
                opt.step()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        lengths = ep["alive"].sum(dim=0).float()
        std = torch.exp(policy.log_std.detach()).mean()
        print("%s %3d: %5d steps, mean episode length %7.1f (max %5d), %7d samples, loss %12.4f, mean std %8.4f, rollout %.2f s, update %.4f s" % (
            "greedy " if evaluate else "episode", episode, ep["alive"].shape[0], float(lengths.mean()), int(lengths.max()), samples, float(loss[0]),
            float(std), t1 - t0, t2 - t1), flush=True)
    print("parameters finite %s" % all(bool(torch.isfinite(p).all()) for p in policy.parameters()), flush=True)
    return float(lengths.mean())


if __name__ == "__main__":
    main()
