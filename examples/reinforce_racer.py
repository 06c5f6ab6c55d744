"""REINFORCE racers on the device environment: the reference's RLRacers/Reinforce app (reinforce_sim.cpp:46-90, ReinforceAgent.hpp,
Policy.hpp) for N agents that share the 5-128-3 policy network with its Dropout(0.6).

    python examples/reinforce_racer.py [--agents 1024] [--episodes 20] [--track Silverstone] [--device-update [--graph-chunk 32]]

Per episode (reinforce_sim.cpp:52-88): resetAgent to random centre-line points, one observation step, then act / step until every
agent has crashed; then ReinforceAgent::updatePolicy (ReinforceAgent.hpp:91-123): discounted returns (gamma 0.99, normalised), the
loss sum of -log p(a) * return over the episode's samples, one Adam step with lr 0.01.  The returns are discounted per agent along
time and normalised over the alive samples, as everywhere in this project.

--device-update: the whole episode stays on the device (DESIGN.md sections 14, 15 and 19): okenv_actor_act with the dropout mask on
the hidden layer acts and records, rollout.prepare_batch builds the training set, rollout.reinforce_update regenerates every
sample's mask, computes loss and gradient and takes the Adam step in place in the parameters the device actor acts with; the torch
module receives them once, at the end (venv.pull_actor()).

Without it the plain PyTorch loop runs: the module with torch.nn.Dropout in training mode acts, and the update is the reference's
one backward pass over the log-probabilities that were saved while acting.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.rollout import PPO_ACTIONS, collect_episode_device, discounted_returns, prepare_batch, reinforce_update  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402


def torch_episode(venv, policy, max_steps, check_every=8):
    """reinforce_sim.cpp:52-88 with the module acting in training mode: the log-probabilities keep their graphs, as saved_log_probs do."""
    table = torch.tensor(PPO_ACTIONS, dtype=torch.float32, device=venv.device)  # (ReinforceAgent::kActionMap is PPOAgent's)
    venv.reset()
    logps, rewards, alive = [], [], []
    steps = 0
    while True:
        probs = policy(venv.observation())
        action = torch.multinomial(probs.detach(), 1)
        logps.append(torch.log(probs.gather(1, action)).squeeze(1))
        alive.append(~venv.done.clone())
        venv.step(table[action.squeeze(1)])
        rewards.append(venv.reward.clone())
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
    ap.add_argument("--dropout", type=float, default=0.6)               # Policy.hpp:18
    ap.add_argument("--device-update", action="store_true", help="act, batch and update on the device (rollout.reinforce_update)")
    ap.add_argument("--graph-chunk", type=int, default=32, help="with --device-update: iterations per replayed HIP graph (0: eager)")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    rays = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
    venv = VectorEnvironment(args.track, args.agents, ray_angles_deg=rays, auto_reset=False, seed=args.seed, reward="step")
    lr, gamma = 0.01, 0.99                                              # ReinforceAgent.hpp: kLearningRate, kGamma
    affine1, affine2 = torch.nn.Linear(5, 128).cuda(), torch.nn.Linear(128, 3).cuda()
    # Policy::forward: affine1 -> dropout -> relu -> affine2 -> softmax
    policy = torch.nn.Sequential(affine1, torch.nn.Dropout(args.dropout), torch.nn.ReLU(), affine2, torch.nn.Softmax(dim=1)).train()
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    if args.device_update:
        venv.enable_actor([affine1.weight, affine1.bias, affine2.weight, affine2.bias])
        venv.enable_learner(lr=lr)
        venv.set_actor_dropout(args.dropout)
    for episode in range(args.episodes):
        t0 = time.perf_counter()
        if args.device_update:
            ep = collect_episode_device(venv, max_steps=args.max_steps, graph_chunk=args.graph_chunk)
            data = prepare_batch(venv, ep, gamma=gamma, normalize="returns")
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            loss = reinforce_update(venv, data)["loss"]
            samples = data["count"]
        else:
            ep = torch_episode(venv, policy, args.max_steps)
            mask = ep["alive"].reshape(-1)
            returns = discounted_returns(ep["rewards"] * ep["alive"], gamma, normalize=False).reshape(-1)[mask]
            returns = (returns - returns.mean()) / (returns.std() + torch.finfo(torch.float32).eps)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            loss = (-ep["log_probs"].reshape(-1)[mask] * returns).sum().reshape(1)   # loss += -log_prob * return
            opt.zero_grad()
            loss.backward()
            opt.step()
            samples = int(mask.sum())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        lengths = ep["alive"].sum(dim=0).float()
        print("episode %3d: %5d steps, mean episode length %7.1f (max %5d), %7d samples, loss %12.4f, rollout %.2f s, update %.4f s" % (
            episode, ep["alive"].shape[0], float(lengths.mean()), int(lengths.max()), samples, float(loss[0]), t1 - t0, t2 - t1), flush=True)
    if args.device_update:
        venv.pull_actor()
    print("parameters finite %s" % all(bool(torch.isfinite(p).all()) for p in policy.parameters()), flush=True)
    return float(lengths.mean())


if __name__ == "__main__":
    main()
