"""PPO racers on the device environment: the reference's RLRacers/PPO app (ppo_sim.cpp + PPOAgent.hpp) for thousands of
agents, with the environment, resets and reward bookkeeping on the GPU and the learner in PyTorch-ROCm.

    python examples/ppo_racer.py [--agents 1024] [--episodes 20] [--track Silverstone] [--device-actor [--graph-chunk 32]] [--device-batch]
                                 [--device-update]

--device-actor: the agents act on the device too (okenv_actor_act): one kernel per step evaluates actor and
critic, samples and records the step, and --graph-chunk K replays K such iterations as one HIP graph.

--device-batch: the episode becomes the training set on the device (rollout.prepare_batch): returns, their
normalisation over the alive samples and the packing of those samples in five kernels instead of a Python loop over the rows and
five masked selections; the time of that stage is printed on its own.

--device-update (needs --device-actor --device-batch): the update runs on the device as well (rollout.ppo_update, DESIGN.md section
16): per minibatch two kernels compute both losses, their gradients and the Adam steps in place in the parameters the device actor
acts with, so the whole episode -- act, step, record, batch, update -- stays on the device and the torch modules receive the
parameters once, at the end (venv.pull_actor()).

Per episode (ppo_sim.cpp:49-89): resetAgent to random centre-line points, one observation step, then act / step until
every agent has crashed; then PPOAgent::updatePolicy (PPOAgent.hpp:106-160): discounted returns (gamma 0.99,
normalised), 5 epochs of clipped-surrogate actor updates and MSE critic updates, Adam 3e-4.  Differences from the
reference, both forced by scale: returns are discounted per agent along time (the reference discounts across its
interleaved 15-agent buffer) and minibatches are 4096 samples (the reference uses 64).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.rollout import collect_episode, collect_episode_device, discounted_returns, ppo_update, prepare_batch  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--max-steps", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-actor", action="store_true", help="act with the device actor kernel instead of the PyTorch forward")
    ap.add_argument("--graph-chunk", type=int, default=32, help="with --device-actor: iterations per replayed HIP graph (0: eager)")
    ap.add_argument("--device-batch", action="store_true", help="build the training set with the device kernels (rollout.prepare_batch)")
    ap.add_argument("--device-update", action="store_true", help="run the minibatch loop on the device too (rollout.ppo_update)")
    args = ap.parse_args()
    if args.device_update and not (args.device_actor and args.device_batch):
        ap.error("--device-update requires --device-actor --device-batch")
    torch.manual_seed(args.seed)
    rays = np.array([-70, -30, 0, 30, 70], dtype=np.float32)          # PPOAgent.hpp:56-61
    venv = VectorEnvironment(args.track, args.agents, ray_angles_deg=rays, auto_reset=False, seed=args.seed, reward="step")
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3), torch.nn.Softmax(dim=1)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    opt_a = torch.optim.Adam(actor.parameters(), lr=3e-4)             # kLearningRate
    opt_c = torch.optim.Adam(critic.parameters(), lr=3e-4)
    clip, epochs, batch = 0.2, 5, 4096
    if args.device_actor:
        venv.enable_actor(actor, critic)
    if args.device_update:
        venv.enable_learner(lr=3e-4, clip=clip)
        before = [p.detach().clone() for net in (actor, critic) for p in net.parameters()]
    for episode in range(args.episodes):
        t0 = time.perf_counter()
        if args.device_actor:
            if not args.device_update:  # (the device update steps the parameters the device actor reads)
                venv.sync_actor()  # the parameters the last update left
            ep = collect_episode_device(venv, max_steps=args.max_steps, graph_chunk=args.graph_chunk)
        else:
            ep = collect_episode(venv, actor, max_steps=args.max_steps)
        alive = ep["alive"]
        lengths = alive.sum(dim=0).float()
        if args.device_batch:
            torch.cuda.synchronize()
            tb = time.perf_counter()
            data = prepare_batch(venv, ep, gamma=0.99, normalize="returns")  # returns normalised over the alive samples
            states, actions, old_logp, ret = data["states"], data["actions"].unsqueeze(1), data["log_probs"].unsqueeze(1), data["returns"].unsqueeze(1)
            torch.cuda.synchronize()
            t_batch = time.perf_counter() - tb
        else:
            returns = discounted_returns(ep["rewards"] * alive)          # reward only while the agent is driving
            mask = alive.reshape(-1)
            states = ep["states"].reshape(-1, 5)[mask]
            actions = ep["actions"].reshape(-1, 1)[mask]
            old_logp = ep["log_probs"].reshape(-1, 1)[mask]
            ret = returns.reshape(-1, 1)[mask]
        t1 = time.perf_counter()
        for _ in range(0 if args.device_update else epochs):
            perm = torch.randperm(states.shape[0], device=states.device)
            for i in range(0, states.shape[0], batch):
                j = perm[i:i + batch]
                values = critic(states[j])
                adv = ret[j] - values.detach()
                probs = torch.clamp(actor(states[j]), 1e-8, 1 - 1e-8)
                ratio = torch.exp(torch.log(probs.gather(1, actions[j])) - old_logp[j])
                actor_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
                critic_loss = torch.nn.functional.mse_loss(values, ret[j])
                opt_a.zero_grad()
                actor_loss.backward()
                opt_a.step()
                opt_c.zero_grad()
                critic_loss.backward()
                opt_c.step()
        if args.device_update:
            ppo_update(venv, data, epochs=epochs, minibatch=batch, shuffle=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print("episode %3d: %5d steps, mean episode length %7.1f (max %5d), %7d samples, rollout %.2f s, update %.2f s%s" % (
            episode, ep["states"].shape[0], float(lengths.mean()), int(lengths.max()), states.shape[0], t1 - t0, t2 - t1,
            ", of the rollout the batch %.4f s" % t_batch if args.device_batch else ""), flush=True)
    if args.device_update:
        venv.pull_actor()
        after = [p.detach() for net in (actor, critic) for p in net.parameters()]
        changed = torch.cat([(a != b).reshape(-1) for a, b in zip(after, before)]).cpu()
        moments = venv.env.learner_state()  # a parameter has had a gradient exactly when its second moment is not 0
        stepped = torch.from_numpy(np.concatenate([moments["policy_v"], moments["value_v"]]) != 0)
        print("device update: parameters finite %s, changed %d of the %d that had a gradient (%d parameters, %d optimiser steps)" % (
            all(bool(torch.isfinite(p).all()) for p in after), int((changed & stepped).sum()), int(stepped.sum()), changed.numel(), moments["t"]),
            flush=True)
    return float(lengths.mean())


if __name__ == "__main__":
    main()
