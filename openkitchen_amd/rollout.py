"""Episode collection for the policy-gradient callers (RLRacers/PPO/ppo_sim.cpp:46-92, RLRacers/Reinforce) on the
device environment.

The reference runs 15 agents until ALL have crashed, pushing (state, action, log-prob, +1 reward) per agent and step
into one shared buffer -- crashed agents keep contributing their frozen observation.  `collect_episode` is that loop
for N agents with everything kept on the GPU as [T, N, ...] tensors; `alive[t, i]` marks the entries an agent produced
before it crashed, so a learner can mask the frozen tail (or keep it, as the reference does).
"""
import torch

from . import _capi as capi

# PPOAgent::kActionMap (RLRacers/PPO/PPOAgent.hpp:41-43): action index -> (throttle, steering)
PPO_ACTIONS = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0))


def collect_episode(venv, policy, max_steps=None, check_every=8, actions=PPO_ACTIONS):
    """One pass of the episode loop (ppo_sim.cpp:49-89).

    policy(states [N, R]) -> action probabilities [N, len(actions)] (an Actor::forward, RLRacers/PPO/Actor.hpp:20-27).
    Returns a dict of stacked device tensors: states [T, N, R] (sensor_hits_.norm() / kSensorRange), actions [T, N] i64,
    log_probs [T, N], rewards [T, N] (= 1), alive [T, N] bool.
    """
    assert venv.reward_kind == capi.REWARD_STEP, 'create the VectorEnvironment with reward="step"'
    assert not venv.auto_reset or max_steps is not None, "with auto-reset on the episode never ends: pass max_steps"
    table = torch.tensor(actions, dtype=torch.float32, device=venv.device)
    # resetAgent for every agent + the initial-observation step (ppo_sim.cpp:53-60)
    venv.reset()
    states, acts, logps, rewards, alive = [], [], [], [], []
    steps = 0
    while True:
        state = venv.observation()
        with torch.no_grad():
            probs = torch.clamp(policy(state), 1e-8, 1.0 - 1e-8)        # kProbClamp (PPOAgent.hpp:27,83)
            action = torch.multinomial(probs, 1).squeeze(1)             # :86
            logp = torch.log(probs.gather(1, action.unsqueeze(1))).squeeze(1)
        alive.append(~venv.done.clone())
        states.append(state)
        acts.append(action)
        logps.append(logp)
        venv.step(table[action])
        rewards.append(venv.reward.clone())
        steps += 1
        if steps % check_every == 0 and venv.env.alive_count() == 0:
            break
        if max_steps is not None and steps >= max_steps:
            break
    return {"states": torch.stack(states), "actions": torch.stack(acts), "log_probs": torch.stack(logps),
            "rewards": torch.stack(rewards), "alive": torch.stack(alive)}


class _EpisodeBuffers:
    """[T, N, ...] tensors of an episode, preallocated in blocks of `block` steps; slot(t) gives step t's record pointers."""

    def __init__(self, venv, block, with_value):
        self.venv, self.block, self.blocks = venv, block, []
        self.fields = {"state": ((venv.num_rays,), torch.float32), "action": ((), torch.int64), "prob": ((), torch.float32),
                       "alive": ((), torch.bool), "reward": ((), torch.float32)}
        if with_value:
            self.fields["value"] = ((), torch.float32)

    def _block(self, t):
        while t // self.block >= len(self.blocks):
            self.blocks.append({k: torch.empty((self.block, self.venv.num_envs) + shape, dtype=dt, device=self.venv.device)
                                for k, (shape, dt) in self.fields.items()})
        return self.blocks[t // self.block], t % self.block

    def slot(self, t):
        b, i = self._block(t)
        return {k: v[i] for k, v in b.items()}

    def rows(self, t, n):
        b, i = self._block(t)
        assert i + n <= self.block
        return {k: v[i:i + n] for k, v in b.items()}

    def finish(self, steps):
        """The first `steps` rows of every field: a view when one block holds them, else one concatenation per field."""
        if not self.blocks:
            self._block(0)
        if len(self.blocks) == 1:
            return {k: v[:steps] for k, v in self.blocks[0].items()}
        return {k: torch.cat([b[k] for b in self.blocks])[:steps] for k in self.fields}


def _record_of(slot):
    return {k: v for k, v in slot.items() if k != "reward"}


def collect_episode_device(venv, max_steps=None, check_every=8, graph_chunk=0):
    """collect_episode with the acting on the device: the loop of ppo_sim.cpp:49-89 as `actor_act -> step -> tracker_update`, the
    actor being the one given to venv.enable_actor (call venv.sync_actor() after optimiser steps).  Returns the same dict as
    collect_episode -- states [T, N, R], actions [T, N] i64, log_probs [T, N] (= torch.log of the recorded probabilities),
    rewards [T, N], alive [T, N] bool -- plus values [T, N] when a critic is attached.  The tensors are preallocated in blocks and
    the kernel writes row t directly.

    graph_chunk = K > 0: K iterations are captured once into a HIP graph (kept on `venv` for later episodes) that writes rows
    0 .. K-1 of a chunk buffer; every replay is followed by one device-to-device copy per field into the episode's tensors.

    The loop ends as the reference's does, after the step in which the last agent crashed; that is tested every `check_every`
    steps (once per chunk with a graph), and rows written past that point are trimmed, so T does not depend on either number.  The
    environment itself may have taken those extra steps (crashed agents stand still)."""
    assert venv.reward_kind == capi.REWARD_STEP, 'create the VectorEnvironment with reward="step"'
    assert not venv.auto_reset or max_steps is not None, "with auto-reset on the episode never ends: pass max_steps"
    assert getattr(venv, "_actor_nets", None) is not None, "call venv.enable_actor(actor, critic) first"
    K = int(graph_chunk)
    venv.reset()
    block = 256 if K <= 0 else K * max(1, 256 // K)
    if max_steps is not None:  # everything in one block: the result is a view
        block = max_steps if K <= 0 else K * ((max_steps + K - 1) // K)
    buf = _EpisodeBuffers(venv, block, venv.actor_has_value)
    steps = 0
    start = venv.env.step_count
    if K <= 0:
        while True:
            slot = buf.slot(steps)
            venv.actor_act(_record_of(slot))
            venv.step()
            slot["reward"].copy_(venv.reward)
            steps += 1
            if steps % check_every == 0 and venv.env.alive_count() == 0:
                break
            if max_steps is not None and steps >= max_steps:
                break
    else:
        graph, chunk, offset, base = _chunk_graph(venv, K)
        if offset is not None:  # the captured launches carry base + k as their draw index
            offset.fill_(((start - base + 2 ** 31) % 2 ** 32) - 2 ** 31)
        try:
            while True:
                graph.replay()
                for k, dst in buf.rows(steps, K).items():
                    dst.copy_(chunk[k])
                steps += K
                if venv.env.alive_count() == 0:
                    break
                if max_steps is not None and steps >= max_steps:
                    break
        finally:
            if offset is not None:
                venv.env.step_count = start + steps  # (replays do not advance the host's count)
    out = buf.finish(steps)
    T = steps
    if not venv.auto_reset:  # the reference loop's length: the rows in which somebody was still driving
        T = int(out["alive"].any(dim=1).sum())
    if max_steps is not None:
        T = min(T, max_steps)
    res = {"states": out["state"][:T], "actions": out["action"][:T], "log_probs": torch.log(out["prob"][:T]),
           "rewards": out["reward"][:T], "alive": out["alive"][:T]}
    if venv.actor_has_value:
        res["values"] = out["value"][:T]
    return res


def _chunk_graph(venv, K):
    """The captured chunk of K iterations for this environment: (graph, chunk tensors, draw-offset word or None, the host step
    count the launches were captured with)."""
    if K in venv._actor_graphs:
        return venv._actor_graphs[K]
    chunk = _EpisodeBuffers(venv, K, venv.actor_has_value).rows(0, K)
    # Without auto-reset the step kernels do not advance the device-side step count, and a captured okenv_actor_act carries the
    # host's count of the moment of capture: the graph's last node advances a word of ours by K instead (okenv_actor_act adds it).
    offset = None if venv.auto_reset else torch.zeros(1, dtype=torch.int32, device=venv.device)

    def body():
        for k in range(K):
            venv.actor_act({name: t[k] for name, t in chunk.items() if name != "reward"})
            venv.step()
            chunk["reward"][k].copy_(venv.reward)
        if offset is not None:
            offset.add_(K)

    base = venv.env.step_count
    chunk["reward"][0].copy_(venv.reward)  # torch's own kernels are loaded before the capture; ours are already
    if offset is not None:
        offset.add_(0)
    venv.env.actor_set_draw_offset(offset)  # the captured launches keep the pointer; eager calls afterwards get none
    try:
        graph = venv.capture(body, warmup=0)  # no warm-up iterations: they would move the count the launches are captured with
    finally:
        venv.env.actor_set_draw_offset(None)
    venv._actor_graphs[K] = (graph, chunk, offset, base)
    return venv._actor_graphs[K]


def discounted_returns(rewards, gamma=0.99, normalize=True):
    """Reward-to-go along the time axis of a [T, N] reward tensor, then (optionally) the whole-buffer normalisation of
    ExperienceBuffer::calculateDiscountedRewards (RLRacers/PPO/ExperienceBuffer.hpp:47-71).  The reference discounts
    across its single interleaved (step-major, agent-minor) buffer; per agent along time is what that code intends
    and what makes sense for thousands of agents."""
    out = torch.empty_like(rewards)
    running = torch.zeros_like(rewards[0])
    for t in range(rewards.shape[0] - 1, -1, -1):
        running = rewards[t] + gamma * running
        out[t] = running
    if normalize:
        out = (out - out.mean()) / (out.std() + torch.finfo(torch.float32).eps)
    return out
