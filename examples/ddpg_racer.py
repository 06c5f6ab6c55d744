"""DDPG racers on the device environment: the reference's RLRacers/DDPG app (ddpg_sim.cpp + DDPGAgent.hpp) for thousands of agents
that share the four networks.

    python examples/ddpg_racer.py [--agents 1024] [--episodes 20] [--track Silverstone] [--device-update | --torch-update]
                                  [--graph-chunk 32] [--capacity 1000000] [--batch 250] [--iterations 50] [--noise 0 0]

Per episode (ddpg_sim.cpp:55-95): resetAgent to random centre-line points, one observation step, then act / step / store (state,
action, next state, +1, done) until every agent has crashed; then DDPGAgent::update (DDPGAgent.hpp:127-170) 50 times: a batch of 250
uniform samples, the critic's step on mse(critic(s, a), r + 0.99 (1 - done) critic'(s', actor'(s'))) with Adam 1e-3, the actor's step
on -critic(s, actor(s)).mean() with Adam 1e-4, and the soft updates with tau = 0.005.  The agents always act on the device
(okenv_ddpg_act): throttle_delta = tanh * 50 + 50, steering_delta = tanh * 5.

--device-update (the default): the transitions go into the device's ring (rollout.collect_episode_ddpg) and the update runs there too
(rollout.ddpg_update), in place in the parameters the device actor acts with; the torch modules receive them once, at the end.

--torch-update: the baseline to measure against -- a ring of torch tensors filled by per-step copies, and the update as a PyTorch loop.

Differences from the reference, as in DESIGN.md section 18: the networks are 5 -> 128 -> 2 and 7 -> 128 -> 1 with one hidden layer, the
buffer is a ring that forgets the oldest transitions, and only agents that entered a step alive are stored (--push-all stores
crashed agents' frozen observations too).  --noise adds the optional uniform exploration; the reference has none.
"""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.rollout import collect_episode_ddpg, ddpg_update  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

GAMMA, TAU, LR_ACTOR, LR_CRITIC = 0.99, 0.005, 1e-4, 1e-3
SCALE, BIAS = (50.0, 5.0), (50.0, 0.0)


class TorchRing:
    """The replay ring as torch tensors: the same slots and order as the device's (transition p lives in slot p mod C)."""

    def __init__(self, capacity, num_rays, device):
        self.capacity, self.pushed = capacity, 0
        self.state = torch.zeros((capacity, num_rays), device=device)
        self.next_state = torch.zeros((capacity, num_rays), device=device)
        self.action = torch.zeros((capacity, 2), device=device)
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
        venv.ddpg_act(rec)
        venv.step()
        crashed = venv.done
        ring.push(rec["state"], rec["action"], venv.observation(), torch.ones_like(rec["state"][:, 0]), crashed.float(),
                  torch.ones_like(crashed) if push_all else rec["alive"] != 0)
        steps += 1
        if steps % check_every == 0 and venv.env.alive_count() == 0:
            break
        if steps >= max_steps:
            break
    return {"steps": steps}


class TorchDdpg:
    """DDPGAgent's four networks and two optimisers in PyTorch."""

    def __init__(self, actor, critic, device):
        self.actor, self.critic = actor, critic
        self.actor_target, self.critic_target = copy.deepcopy(actor), copy.deepcopy(critic)
        self.opt_actor = torch.optim.Adam(actor.parameters(), lr=LR_ACTOR)
        self.opt_critic = torch.optim.Adam(critic.parameters(), lr=LR_CRITIC)
        self.scale, self.bias = torch.tensor(SCALE, device=device), torch.tensor(BIAS, device=device)

    def act(self, net, state):
        return torch.tanh(net(state)) * self.scale + self.bias

    def update(self, ring, batch, iterations, generator):
        """DDPGAgent::update (DDPGAgent.hpp:127-170), `iterations` times."""
        device = ring.state.device
        if ring.size() == 0:
            return torch.zeros(iterations, device=device), torch.zeros(iterations, device=device)
        critic_losses, actor_losses = [], []
        for _ in range(iterations):
            idx = torch.randint(ring.size(), (batch,), device=device, generator=generator)
            s, a, s2 = ring.state[idx], ring.action[idx], ring.next_state[idx]
            with torch.no_grad():
                q2 = self.critic_target(torch.cat([s2, self.act(self.actor_target, s2)], 1))
                y = ring.reward[idx, None] + (1.0 - ring.done[idx, None]) * GAMMA * q2
            critic_loss = torch.nn.functional.mse_loss(self.critic(torch.cat([s, a], 1)), y)
            self.opt_critic.zero_grad()
            critic_loss.backward()
            self.opt_critic.step()
            actor_loss = -self.critic(torch.cat([s, self.act(self.actor, s)], 1)).mean()
            self.opt_actor.zero_grad()
            actor_loss.backward()
            self.opt_actor.step()
            with torch.no_grad():
                for net, target in ((self.actor, self.actor_target), (self.critic, self.critic_target)):
                    for p, q in zip(net.parameters(), target.parameters()):
                        q.copy_(TAU * p + (1.0 - TAU) * q)
            critic_losses.append(critic_loss.detach())
            actor_losses.append(actor_loss.detach())
        return torch.stack(critic_losses), torch.stack(actor_losses)


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=20)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--max-steps", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--capacity", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=250)           # kBatchSize
    ap.add_argument("--iterations", type=int, default=50)       # ddpg_sim.cpp:88
    ap.add_argument("--noise", type=float, nargs=2, default=(0.0, 0.0), help="uniform exploration half-widths (the reference: none)")
    ap.add_argument("--push-all", action="store_true", help="store crashed agents' frozen observations too, as the reference's loop does")
    ap.add_argument("--graph-chunk", type=int, default=32, help="with --device-update: iterations per replayed HIP graph (0: eager)")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--device-update", action="store_true", help="replay ring and update on the device (the default)")
    mode.add_argument("--torch-update", action="store_true", help="replay ring in torch tensors, update as a PyTorch loop (the baseline)")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    rays = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
    venv = VectorEnvironment(args.track, args.agents, ray_angles_deg=rays, auto_reset=False, seed=args.seed)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 2)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(7, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    venv.enable_ddpg(actor, critic, scale=SCALE, bias=BIAS, noise=tuple(args.noise), gamma=GAMMA, tau=TAU, lr_actor=LR_ACTOR, lr_critic=LR_CRITIC)
    before = [p.detach().clone() for p in list(actor.parameters()) + list(critic.parameters())]
    if args.torch_update:
        agent = TorchDdpg(actor, critic, venv.device)
        ring = TorchRing(args.capacity, 5, venv.device)
        rec = {"state": torch.empty((args.agents, 5), device=venv.device), "action": torch.empty((args.agents, 2), device=venv.device),
               "alive": torch.empty(args.agents, dtype=torch.uint8, device=venv.device)}
        gen = torch.Generator(device=venv.device)
        gen.manual_seed(args.seed)
    else:
        venv.enable_ddpg_replay(args.capacity, push_all=args.push_all)
    for episode in range(args.episodes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.torch_update:
            ep = collect_episode_torch(venv, ring, rec, args.max_steps, push_all=args.push_all)
        else:
            ep = collect_episode_ddpg(venv, max_steps=args.max_steps, graph_chunk=args.graph_chunk)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if args.torch_update:
            critic_loss, actor_loss = agent.update(ring, args.batch, args.iterations, gen)
            keep = flat(actor)
            venv.env.ddpg_set_params(keep, None)  # the device actor acts with the module's new parameters
            stored = ring.size()
        else:
            critic_loss, actor_loss = ddpg_update(venv, batch=args.batch, iterations=args.iterations)
            stored = venv.env.ddpg_replay_size()[0]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        values = [float(critic_loss[0]), float(critic_loss[-1]), float(actor_loss[0]), float(actor_loss[-1])]
        print("episode %3d  steps %5d  stored %8d  critic loss %.4g -> %.4g  actor loss %.4g -> %.4g  rollout %.3f s  update %.3f s" % (
            episode, ep["steps"], stored, *values, t1 - t0, t2 - t1), flush=True)
        assert np.isfinite(values).all()
    if args.torch_update:
        targets = [flat(agent.actor_target), flat(agent.critic_target)]
    else:
        venv.pull_ddpg()
        st = venv.env.ddpg_state()
        targets = [torch.from_numpy(st["actor_target"]).cuda(), torch.from_numpy(st["critic_target"]).cuda()]
    now = list(actor.parameters()) + list(critic.parameters())
    moved = max(float((p.detach() - b).abs().max()) for p, b in zip(now, before))
    apart = max(float((flat(actor) - targets[0]).abs().max()), float((flat(critic) - targets[1]).abs().max()))
    print("largest parameter movement: %.3g  largest distance online - target: %.3g" % (moved, apart))
    assert moved > 0 and apart > 0 and all(torch.isfinite(p).all() for p in now)
    venv.close()


if __name__ == "__main__":
    main()
