"""Deep-Q racers on the device environment: the reference's RLRacers/Deep_Q_Learning app (dq_racer_sim.cpp + DQAgent.hpp) for
thousands of agents that share one Q network.

    python examples/dqn_racer.py [--agents 1024] [--episodes 20] [--track Silverstone] [--device-update | --torch-update]
                                 [--graph-chunk 32] [--capacity 1000000] [--batch 100] [--iterations 200] [--resample]

Per episode (dq_racer_sim.cpp:61-133): resetAgent to random centre-line points, one observation step, then act epsilon-greedily /
step / store (state, action, next state, reward, done) until every agent has crashed; then DQLearnAgent::updateDQN
(DQAgent.hpp:106-150): one batch of 100 uniform samples of the replay buffer, 200 iterations of the mean squared
temporal-difference error against r + 0.99 max q'(s') with Adam 1e-4, no target network; epsilon starts at 0.99 and falls by 0.01
per episode.  The agents always act on the device (okenv_actor_act in its eps-greedy mode).

--device-update (the default): the transitions go into the device's replay ring (rollout.collect_episode_dqn) and the update runs
there too (rollout.dqn_update), in place in the parameters the device actor acts with: an episode crosses to
the host with the one integer that ends it, and the torch module receives the parameters once, at the end (venv.pull_actor()).

--torch-update: the baseline to measure against -- a replay ring of torch tensors filled by per-step copies, and updateDQN as a
PyTorch loop.

Differences from the reference, as in DESIGN.md section 14: the Q network is 5 -> 128 -> 5 with one hidden layer (the reference's
400-300 stack is a GEMM's business), the buffer is a ring that forgets the oldest transitions, and only agents that entered a step
alive are stored (--push-all stores crashed agents' frozen observations too, as the reference's loop does).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.rollout import DQN_ACTIONS, collect_episode_dqn, dqn_update  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

GAMMA, LR, SENSOR_RANGE = 0.99, 1e-4, 200.0


class TorchRing:
    """The replay ring as torch tensors: the same slots and order as the device's (transition p lives in slot p mod C)."""

    def __init__(self, capacity, num_rays, device):
        self.capacity, self.pushed = capacity, 0
        self.state = torch.zeros((capacity, num_rays), device=device)
        self.next_state = torch.zeros((capacity, num_rays), device=device)
        self.action = torch.zeros(capacity, dtype=torch.int64, device=device)
        self.reward = torch.zeros(capacity, device=device)
        self.done = torch.zeros(capacity, device=device)

    def push(self, state, action, next_state, reward, done, selected):
        idx = selected.nonzero().flatten()
        n = idx.numel()
        keep = idx[max(0, n - self.capacity):]
        slots = (self.pushed + max(0, n - self.capacity) + torch.arange(keep.numel(), device=idx.device)) % self.capacity
        self.state[slots], self.next_state[slots], self.action[slots] = state[keep], next_state[keep], action[keep]
        self.reward[slots], self.done[slots] = reward[keep], done[keep]
        self.pushed += n

    def size(self):
        return min(self.pushed, self.capacity)


def collect_episode_torch(venv, ring, rec, max_steps, check_every=8, push_all=False):
    """The same loop with the store in Python: per step the record, the next observation, the reward and the flags are copied."""
    venv.reset()
    steps = 0
    while True:
        venv.actor_act(rec)
        venv.step()
        crashed = venv.done
        clearance = torch.clamp(venv.distances.min(dim=1).values, max=SENSOR_RANGE)
        reward = torch.where(crashed, torch.full_like(clearance, -200.0), clearance)  # DQAgent.hpp:162-181
        ring.push(rec["state"], rec["action"], venv.observation(), reward, crashed.float(), torch.ones_like(crashed) if push_all else rec["alive"] != 0)
        steps += 1
        if steps % check_every == 0 and venv.env.alive_count() == 0:
            break
        if steps >= max_steps:
            break
    return {"steps": steps}


def update_torch(net, opt, ring, batch, iterations, resample, generator):
    """updateDQN (DQAgent.hpp:106-150)."""
    losses = []
    if ring.size() == 0:
        return torch.zeros(iterations, device=ring.state.device)
    idx = torch.randint(ring.size(), (batch,), device=ring.state.device, generator=generator)
    for _ in range(iterations):
        if resample:
            idx = torch.randint(ring.size(), (batch,), device=ring.state.device, generator=generator)
        q = net(ring.state[idx])
        with torch.no_grad():
            y = ring.reward[idx] + GAMMA * net(ring.next_state[idx]).amax(dim=1)
        target = q.detach().clone()
        target[torch.arange(batch, device=idx.device), ring.action[idx]] = y
        loss = torch.nn.functional.mse_loss(q, target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--max-steps", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--capacity", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=100)          # kBatchSize
    ap.add_argument("--iterations", type=int, default=200)     # kIterationSteps
    ap.add_argument("--resample", action="store_true", help="a fresh batch per iteration (the reference's commented alternative)")
    ap.add_argument("--push-all", action="store_true", help="store crashed agents' frozen observations too, as the reference's loop does")
    ap.add_argument("--graph-chunk", type=int, default=32, help="with --device-update: iterations per replayed HIP graph (0: eager)")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--device-update", action="store_true", help="replay ring and update on the device (the default)")
    mode.add_argument("--torch-update", action="store_true", help="replay ring in torch tensors, update as a PyTorch loop (the baseline)")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    rays = np.array([-70, -30, 0, 30, 70], dtype=np.float32)   # DQAgent.hpp:59-65
    venv = VectorEnvironment(args.track, args.agents, ray_angles_deg=rays, auto_reset=False, seed=args.seed)
    net = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, len(DQN_ACTIONS))).cuda()
    epsilon = 0.99                                               # kEpsilon
    venv.enable_actor(net, mode="eps_greedy", actions=DQN_ACTIONS, epsilon=epsilon)
    if args.torch_update:
        opt = torch.optim.Adam(net.parameters(), lr=LR)          # kLearningRate
        ring = TorchRing(args.capacity, 5, venv.device)
        rec = {"state": torch.empty((args.agents, 5), device=venv.device), "action": torch.empty(args.agents, dtype=torch.int64, device=venv.device),
               "alive": torch.empty(args.agents, dtype=torch.uint8, device=venv.device)}
        gen = torch.Generator(device=venv.device)
        gen.manual_seed(args.seed)
    else:
        venv.enable_learner(lr=LR)
        venv.enable_replay(args.capacity, push_all=args.push_all, gamma=GAMMA)
        before = [p.detach().clone() for p in net.parameters()]
    for episode in range(args.episodes):
        venv.set_actor_epsilon(epsilon)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.torch_update:
            ep = collect_episode_torch(venv, ring, rec, args.max_steps, push_all=args.push_all)
        else:
            ep = collect_episode_dqn(venv, max_steps=args.max_steps, graph_chunk=args.graph_chunk)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if args.torch_update:
            losses = update_torch(net, opt, ring, args.batch, args.iterations, args.resample, gen)
            venv.sync_actor()
            stored = ring.size()
        else:
            losses = dqn_update(venv, batch=args.batch, iterations=args.iterations, resample=args.resample)
            stored = venv.env.replay_size()[0]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        first, last = float(losses[0]), float(losses[-1])
        print("episode %3d  epsilon %.2f  steps %5d  stored %8d  loss %.4g -> %.4g  rollout %.3f s  update %.3f s" % (
            episode, epsilon, ep["steps"], stored, first, last, t1 - t0, t2 - t1), flush=True)
        assert np.isfinite(first) and np.isfinite(last)
        epsilon = epsilon - 0.01 if epsilon > 0.01 else 0.0     # dq_racer_sim.cpp:117-128
    if not args.torch_update:
        venv.pull_actor()
        moved = max(float((p.detach() - b).abs().max()) for p, b in zip(net.parameters(), before))
        print("largest parameter movement: %.3g" % moved)
        assert moved > 0 and all(torch.isfinite(p).all() for p in net.parameters())
    venv.close()


if __name__ == "__main__":
    main()
