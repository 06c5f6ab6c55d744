"""Episode collection for the policy-gradient callers (RLRacers/PPO/ppo_sim.cpp:46-92, RLRacers/Reinforce) on the
device environment.

The reference runs 15 agents until ALL have crashed, pushing (state, action, log-prob, +1 reward) per agent and step
into one shared buffer -- crashed agents keep contributing their frozen observation.  `collect_episode` is that loop
for N agents with everything kept on the GPU as [T, N, ...] tensors; `alive[t, i]` marks the entries an agent produced
before it crashed, so a learner can mask the frozen tail (or keep it, as the reference does).
"""
import collections
import warnings

import torch

from . import _capi as capi

# PPOAgent::kActionMap (RLRacers/PPO/PPOAgent.hpp:41-43): action index -> (throttle, steering)
PPO_ACTIONS = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0))
# DQLearnAgent::kActionMap (RLRacers/Deep_Q_Learning/DQAgent.hpp:40-45)
DQN_ACTIONS = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0), (30.0, 2.5), (30.0, -2.5))


# What a collector hands _run_episode for graph_chunk = K > 0: the cache `graphs` and the `key` of its captured chunk in it; the acting
# object's actor_set_draw_offset / ddpg_set_draw_offset; build() -> (iteration(k) for the chunk's k-th iteration, the tensors the graph
# reads and writes), called when the chunk has to be captured; after_replay(steps, tensors), or None, called after every replay.
_Chunk = collections.namedtuple("_Chunk", "K graphs key set_draw_offset build after_replay")


def _run_episode(venv, iteration, max_steps, check_every, chunk=None):
    """The episode loop of every collector: reset, then iteration(t) for t = 0, 1, ... until nobody is alive -- tested with
    alive_count(), which synchronises, on the multiples of `check_every` only -- or `max_steps` steps have run.  Returns (the host's
    step count after the reset, steps taken).

    chunk (a _Chunk) with K > 0: the loop replays a HIP graph of K iterations instead and tests once per replay, so the steps are a
    multiple of K.  The graph is chunk.graphs[chunk.key]; when it is not there, it is captured from chunk.build() and kept there with
    the tensors it reads and writes."""
    venv.reset()  # resetAgent for every agent + the initial-observation step (ppo_sim.cpp:53-60)
    start = venv.env.step_count
    steps, stride, offset = 0, 1, None
    K = 0 if chunk is None else chunk.K
    if K > 0:
        graphs, key, set_draw_offset = chunk.graphs, chunk.key, chunk.set_draw_offset
        if key not in graphs:
            chunk_iteration, kept = chunk.build()
            # Without auto-reset the step kernels do not advance the device-side step count, and a captured act carries the host's
            # count of the moment of capture: the graph's last node advances a word of ours by K instead (the act kernels add it).
            offset = None if venv.auto_reset else torch.zeros(1, dtype=torch.int32, device=venv.device)

            def body():
                for k in range(K):
                    chunk_iteration(k)
                if offset is not None:
                    offset.add_(K)

            base = venv.env.step_count
            if offset is not None:
                offset.add_(0)  # torch's own kernel is loaded before the capture; ours are already
            set_draw_offset(offset)  # the captured launches keep the pointer; eager calls afterwards get none
            try:
                # no warm-up iterations: they would push into a ring and move the count the launches are captured with
                graph = venv.capture(body, warmup=0)
            finally:
                set_draw_offset(None)
            graphs[key] = (graph, offset, base, kept)  # (the tensors are the graph's: kept alive with it)
        graph, offset, base, kept = graphs[key]
        if offset is not None:  # the captured launches carry base + k as their draw index
            offset.fill_(((start - base + 2 ** 31) % 2 ** 32) - 2 ** 31)
        stride = check_every = K  # one test per replay
    try:
        while True:
            if K > 0:
                graph.replay()
                if chunk.after_replay is not None:
                    chunk.after_replay(steps, kept)
            else:
                iteration(steps)
            steps += stride
            if steps % check_every == 0 and venv.env.alive_count() == 0:
                break
            if max_steps is not None and steps >= max_steps:
                break
    finally:
        if offset is not None:
            venv.env.step_count = start + steps  # (replays do not advance the host's count)
    return start, steps


def collect_episode(venv, policy, max_steps=None, check_every=8, actions=PPO_ACTIONS):
    """One pass of the episode loop (ppo_sim.cpp:49-89).

    policy(states [N, R]) -> action probabilities [N, len(actions)] (an Actor::forward, RLRacers/PPO/Actor.hpp:20-27).
    Returns a dict of stacked device tensors: states [T, N, R] (sensor_hits_.norm() / kSensorRange), actions [T, N] i64,
    log_probs [T, N], rewards [T, N] (= 1), alive [T, N] bool.
    """
    assert venv.reward_kind == capi.REWARD_STEP, 'create the VectorEnvironment with reward="step"'
    assert not venv.auto_reset or max_steps is not None, "with auto-reset on the episode never ends: pass max_steps"
    table = torch.tensor(actions, dtype=torch.float32, device=venv.device)
    states, acts, logps, rewards, alive = [], [], [], [], []

    def iteration(_):
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

    _run_episode(venv, iteration, max_steps, check_every)
    return {"states": torch.stack(states), "actions": torch.stack(acts), "log_probs": torch.stack(logps),
            "rewards": torch.stack(rewards), "alive": torch.stack(alive)}


class _EpisodeBuffers:
    """[T, N, ...] tensors of an episode, preallocated in blocks of `block` steps; slot(t) gives step t's record pointers."""

    def __init__(self, venv, block, with_value, fields=None):
        self.venv, self.block, self.blocks = venv, block, []
        self.fields = {"state": ((venv.num_rays,), torch.float32), "action": ((), torch.int64), "prob": ((), torch.float32),
                       "alive": ((), torch.bool), "reward": ((), torch.float32)} if fields is None else dict(fields)
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


def _act_step_record(venv, slot):
    """One iteration of collect_episode_device into the row `slot` of the episode's (or a chunk's) tensors."""
    venv.actor_act({k: v for k, v in slot.items() if k != "reward"})
    venv.step()
    slot["reward"].copy_(venv.reward)


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
    block = 256 if K <= 0 else K * max(1, 256 // K)
    if max_steps is not None:  # everything in one block: the result is a view
        block = max_steps if K <= 0 else K * ((max_steps + K - 1) // K)
    buf = _EpisodeBuffers(venv, block, venv.actor_has_value)

    def build():
        chunk = _EpisodeBuffers(venv, K, venv.actor_has_value).rows(0, K)
        chunk["reward"][0].copy_(venv.reward)  # torch's own kernels are loaded before the capture; ours are already
        return (lambda k: _act_step_record(venv, {name: t[k] for name, t in chunk.items()})), chunk

    def copy_rows(steps, chunk):  # one device-to-device copy per field into the episode's tensors
        for name, dst in buf.rows(steps, K).items():
            dst.copy_(chunk[name])

    captured = _Chunk(K=K, graphs=venv._actor_graphs, key=K, set_draw_offset=venv.env.actor_set_draw_offset, build=build, after_replay=copy_rows)
    start, steps = _run_episode(venv, lambda t: _act_step_record(venv, buf.slot(t)), max_steps, check_every, captured)
    out = buf.finish(steps)
    T = steps
    if not venv.auto_reset:  # the reference loop's length: the rows in which somebody was still driving
        T = int(out["alive"].any(dim=1).sum())
    if max_steps is not None:
        T = min(T, max_steps)
    res = {"states": out["state"][:T], "actions": out["action"][:T], "log_probs": torch.log(out["prob"][:T]),
           "rewards": out["reward"][:T], "alive": out["alive"][:T]}
    venv._episode_probs = (res["log_probs"], out["prob"][:T])  # the probabilities as recorded, for prepare_batch -> ppo_update
    venv._episode_draw_first = (res["log_probs"], start)  # row 0's draw index, for prepare_batch -> reinforce_update's dropout masks
    if venv.actor_has_value:
        res["values"] = out["value"][:T]
    return res


def _rows_of(x, width):
    """(tensor to hand over, its row stride in agent slots) of a [T, N] / [T, N, width] tensor: a view whose rows are dense and a
    whole number of slots apart is passed as it is (the block buffers of _EpisodeBuffers), anything else is made contiguous."""
    T, N = x.shape[0], x.shape[1]
    dense = x.stride(1) == width and (x.dim() == 2 or x.stride(2) == 1)
    if dense and (T == 1 or (x.stride(0) % width == 0 and x.stride(0) // width >= N)):
        return x, (N if T == 1 else x.stride(0) // width)
    return x.contiguous(), N


_NORMALIZE = {True: capi.BATCH_NORMALIZE_RETURN | capi.BATCH_NORMALIZE_ADVANTAGE, False: 0, None: 0, "returns": capi.BATCH_NORMALIZE_RETURN,
              "advantages": capi.BATCH_NORMALIZE_ADVANTAGE}


def prepare_batch(venv, ep, gamma=0.99, lam=None, normalize=True, last_value=None, block_threads=0):
    """From a recorded episode to the learner's batch on the device (okenv_batch_prepare): what
    ExperienceBuffer::calculateDiscountedRewards + ::sample do in the reference (RLRacers/PPO/ExperienceBuffer.hpp:15-68), for the
    dict `ep` that collect_episode_device or collect_episode returns.

    Returns per agent along time with `alive` as the episode boundary (a dead row ends an episode: with auto-reset on a column holds
    several), GAE(lam) advantages when `lam` is given and the episode has values (`last_value` [N]: the critic's value after the last
    row, for episodes cut by max_steps), normalised over the M alive samples ((x - mean) / (std + eps), unbiased std; normalize:
    True / False / "returns" / "advantages"), and the alive samples packed in step-major, agent-minor order -- the order of
    x.reshape(-1)[alive.reshape(-1)].

    Returns a dict of device tensors: states [M, R], actions [M] i64, log_probs [M], returns [M], advantages [M] (with values), index
    [M] i32 (t * N + i), count (M, an int: the call waits for the stream once to read it), stats (the okenv_batch_stats words on
    the device; batch_stats(batch) reads them) and, for an episode dict collect_episode_device returned, draw_first (an int: the
    device actor's draw index of row 0)."""
    rewards, alive = ep["rewards"], ep["alive"]
    T, N = rewards.shape
    R = ep["states"].shape[2]
    dev = rewards.device
    use_value = lam is not None and "values" in ep
    if alive.dtype not in (torch.bool, torch.uint8):
        alive = alive != 0
    record = [_rows_of(rewards.float(), 1), _rows_of(alive, 1)] + ([_rows_of(ep["values"].float(), 1)] if use_value else [])
    if len({s for _, s in record}) > 1:
        record = [(x.contiguous(), N) for x, _ in record]
    fields = [_rows_of(ep["states"].float(), R), _rows_of(ep["actions"], 1), _rows_of(ep["log_probs"].float(), 1)]
    if len({s for _, s in fields}) > 1:
        fields = [(x.contiguous(), N) for x, _ in fields]
    assert fields[1][0].dtype == torch.int64, "actions must be int64"
    inputs = {"reward": record[0][0], "alive": record[1][0], "state": fields[0][0], "action": fields[1][0], "prob": fields[2][0]}
    cap = T * N
    out = {"state": torch.empty((cap, R), dtype=torch.float32, device=dev), "action": torch.empty(cap, dtype=torch.int64, device=dev),
           "prob": torch.empty(cap, dtype=torch.float32, device=dev), "ret": torch.empty(cap, dtype=torch.float32, device=dev),
           "index": torch.empty(cap, dtype=torch.int32, device=dev), "stats": torch.empty(capi.BATCH_STATS_BYTES // 8, dtype=torch.float64, device=dev)}
    if use_value:
        inputs["value"] = record[2][0]
        out["adv"] = torch.empty(cap, dtype=torch.float32, device=dev)
        if last_value is not None:
            inputs["last_value"] = last_value.to(device=dev, dtype=torch.float32).contiguous()
            assert inputs["last_value"].numel() == N
    venv.env.batch_prepare(T, N, inputs, out, state_width=R, record_stride=record[0][1], field_stride=fields[0][1], gamma=gamma,
                           lam=lam if use_value else 1.0, normalize=_NORMALIZE[normalize], block_threads=block_threads)
    M = venv.env.batch_count()  # waits for the stream: the inputs above may go now
    res = {"states": out["state"][:M], "actions": out["action"][:M], "log_probs": out["prob"][:M], "returns": out["ret"][:M],
           "index": out["index"][:M], "count": M, "stats": out["stats"]}
    if use_value:
        res["advantages"] = out["adv"][:M]
    drawn = getattr(venv, "_episode_draw_first", None)
    if drawn is not None and drawn[0] is ep["log_probs"]:
        res["draw_first"] = drawn[1]  # the device actor's draw index of the episode's row 0 (reinforce_update's masks)
    recorded = getattr(venv, "_episode_probs", None) if getattr(venv, "learner_enabled", False) else None
    if recorded is not None and recorded[0] is ep["log_probs"]:
        # the probabilities as the device actor recorded them (ppo_update's ratio divides by them), by the samples' flat indices
        res["probs"] = recorded[1].reshape(-1)[res["index"].long()].contiguous()
    return res


def ppo_update(venv, batch, epochs=5, minibatch=4096, shuffle=True, use_advantages=False, grads=False):
    """PPOAgent::updatePolicy's minibatch loop on the device (okenv_ppo_update) for the dict prepare_batch
    returns: `epochs` passes over the M samples in minibatches of `minibatch`, per minibatch the clipped-surrogate actor loss and the
    critic's squared error, their gradients and one Adam step on each network, in place in the parameters the device actor acts
    with (venv.enable_learner first; no sync_actor afterwards, venv.pull_actor() brings them back to the modules).

    shuffle: a fresh torch.randperm per epoch (False: the buffer's order, as the reference walks it).  The advantage is
    returns - v(s) with the critic's value from before the minibatch's steps, or batch["advantages"] with use_advantages.  The old
    probabilities are batch["probs"] (an episode recorded by collect_episode_device carries them), else exp(batch["log_probs"]).

    Everything is enqueued on the environment's stream; nothing is read back.  Returns a dict of device tensors, one entry per
    minibatch in the order they ran: actor_loss, critic_loss (float32), clipped (int32: samples whose ratio left
    [1 - clip, 1 + clip]); with grads=True also grad_policy and grad_value of the last minibatch."""
    M = int(batch["states"].shape[0])
    dev = batch["states"].device
    if "probs" in batch:
        probs = batch["probs"]
    else:
        # exp(log p) is p only up to rounding: the ratio of the first minibatch is then no longer exactly 1
        warnings.warn("ppo_update: the batch carries no recorded probabilities (\"probs\"); using exp(log_probs).  prepare_batch adds them "
                      "for the episode dict collect_episode_device returned, unchanged, once venv.enable_learner has been called.", stacklevel=2)
        probs = torch.exp(batch["log_probs"])
    data = {"state": batch["states"].float().contiguous(), "action": batch["actions"].reshape(-1).contiguous(),
            "prob": probs.reshape(-1).float().contiguous(), "ret": batch["returns"].reshape(-1).float().contiguous()}
    assert data["action"].dtype == torch.int64, "actions must be int64"
    if use_advantages:
        data["adv"] = batch["advantages"].reshape(-1).float().contiguous()
    order = torch.stack([torch.randperm(M, device=dev) for _ in range(epochs)]).to(torch.int32).contiguous() if shuffle else None
    n = epochs * ((M + minibatch - 1) // minibatch)
    out = {"actor_loss": torch.empty(n, dtype=torch.float32, device=dev), "critic_loss": torch.empty(n, dtype=torch.float32, device=dev),
           "clipped": torch.empty(n, dtype=torch.int32, device=dev)}
    if grads:
        n_policy, n_value = venv.env.actor_num_params()
        out["grad_policy"] = torch.empty(n_policy, dtype=torch.float32, device=dev)
        if n_value:
            out["grad_value"] = torch.empty(n_value, dtype=torch.float32, device=dev)
    venv.env.ppo_update(data, M, minibatch, epochs, order, out)
    venv._update_inputs = (data, order)  # alive until the next update: the kernels are only enqueued
    return out


def reinforce_update(venv, batch, slice=16384, accumulate=True, reduce="sum", shuffle=False, grads=False):
    """ReinforceAgent::updatePolicy on the device (okenv_reinforce_update) for the dict prepare_batch returns:
    loss = sum of -log p(a) * return over the M samples, its gradient through the policy network -- with the dropout masks the device
    actor drew while acting, regenerated from batch["index"] and the draw index collect_episode_device kept -- and one Adam step, in
    place in the parameters the device actor acts with (venv.enable_actor, venv.enable_learner(lr=0.01) first; no sync_actor
    afterwards, venv.pull_actor() brings them back to the module).

    slice: samples per pair of launches; it bounds the scratch, and the sums' order (so the last bits) depends on it.
    accumulate=False steps after every slice instead (minibatch REINFORCE); reduce "sum" (the reference) or "mean"; shuffle: a
    torch.randperm over the samples.  While dropout is on the batch must carry "draw_first", which prepare_batch adds for the episode dict
    collect_episode_device returned: a batch of an older episode keeps its own draw index.

    Everything is enqueued on the environment's stream; nothing is read back.  Returns a dict of device tensors: loss [steps]
    (float32, one per optimiser step) and, with grads=True, grad_policy of the last step."""
    M = int(batch["states"].shape[0])
    dev = batch["states"].device
    data = {"state": batch["states"].float().contiguous(), "action": batch["actions"].reshape(-1).contiguous(),
            "ret": batch["returns"].reshape(-1).float().contiguous()}
    assert data["action"].dtype == torch.int64, "actions must be int64"
    draw_first = 0
    if getattr(venv, "actor_dropout", 0.0) > 0.0:
        # the masks are those of the episode the batch was cut from: prepare_batch puts its draw index beside the samples' indices
        assert "draw_first" in batch, ("with dropout on, the batch must be prepare_batch's of the episode dict collect_episode_device returned, "
                                       "unchanged: it carries that episode's draw index")
        data["index"] = batch["index"].reshape(-1).to(torch.int32).contiguous()
        draw_first = batch["draw_first"]
    order = torch.randperm(M, device=dev).to(torch.int32).contiguous() if shuffle else None
    out = {"loss": torch.empty(1 if accumulate else (M + slice - 1) // slice, dtype=torch.float32, device=dev)}
    if grads:
        out["grad_policy"] = torch.empty(venv.env.actor_num_params()[0], dtype=torch.float32, device=dev)
    venv.env.reinforce_update(data, M, slice, accumulate, reduce, venv.num_envs, draw_first, order, out)
    venv._update_inputs = (data, order)  # alive until the next update: the kernels are only enqueued
    return out


def _ring_record(venv, action_shape, action_dtype):
    """The record an act kernel fills and a push reads: "state" [N, R], "action" [N, *action_shape] and "alive" [N]."""
    return {"state": torch.empty((venv.num_envs, venv.num_rays), dtype=torch.float32, device=venv.device),
            "action": torch.empty((venv.num_envs,) + action_shape, dtype=action_dtype, device=venv.device),
            "alive": torch.empty(venv.num_envs, dtype=torch.uint8, device=venv.device)}


# What tells the Deep-Q collector from the DDPG collector: the act and push methods, the action's shape and dtype in the record, the
# attribute of venv that keeps the eager episodes' record, the cache of captured chunks with the key's prefix in it, and the setter
# of the acting object's draw-offset word.
_RingCollector = collections.namedtuple("_RingCollector", "act push action_shape action_dtype eager_record graphs key set_draw_offset")


def _collect_into_ring(venv, kind, max_steps, check_every, K, reward):
    """What collect_episode_dqn and collect_episode_ddpg share (`kind`: a _RingCollector): `act -> step -> push` on one record, the one
    kept on venv for eager episodes and one of its own for every captured chunk, which also keeps `reward`."""
    def iteration_on(rec):
        def iteration(_):
            kind.act(rec)
            venv.step()
            kind.push(rec, reward)
        return iteration

    def build():
        rec = _ring_record(venv, kind.action_shape, kind.action_dtype)
        return iteration_on(rec), (rec, reward)

    rec = None
    if K <= 0:
        rec = getattr(venv, kind.eager_record, None) or _ring_record(venv, kind.action_shape, kind.action_dtype)
        setattr(venv, kind.eager_record, rec)
    chunk = _Chunk(K=K, graphs=kind.graphs, key=kind.key + (K, None if reward is None else reward.data_ptr()),
                   set_draw_offset=kind.set_draw_offset, build=build, after_replay=None)
    return {"steps": _run_episode(venv, iteration_on(rec), max_steps, check_every, chunk)[1]}


def collect_episode_dqn(venv, max_steps=None, check_every=8, graph_chunk=0, reward=None):
    """One episode of dq_racer_sim.cpp:61-130 on the device: reset, then `actor_act (eps-greedy) -> step -> replay_push` until every
    agent has crashed (tested every `check_every` steps) or `max_steps` steps have run.  Nothing but that test crosses to the host:
    the transitions go straight into the ring of venv.enable_replay, which keeps them for later episodes.  reward: None for the
    reference's clearance reward (DQAgent.hpp:162-181), "tracker" for the environment's own `reward` tensor, or a device tensor [N]
    that the caller keeps up to date.

    graph_chunk = K > 0: K iterations are captured once into a HIP graph (kept on `venv` until set_actor_epsilon changes what it
    carries) and replayed; the test runs once per chunk.  Without auto-reset the graph's last node advances the word the actor adds
    to its draw index, so replays keep drawing fresh numbers; eager and chunked episodes fill the ring with the same bits.

    Returns {"steps": steps taken}; a multiple of K with a graph (crashed agents stand still, and only agents that entered a step
    alive are pushed unless the ring was created with push_all)."""
    assert getattr(venv, "_actor_nets", None) is not None, "call venv.enable_actor(q_network, mode=\"eps_greedy\") first"
    assert getattr(venv, "replay_push_all", None) is not None, "call venv.enable_replay(capacity) first"
    assert not venv.auto_reset or max_steps is not None, "with auto-reset on the episode never ends: pass max_steps"
    if isinstance(reward, str):
        assert reward == "tracker" and venv.reward_kind is not None, 'reward="tracker" needs a VectorEnvironment with a reward'
        reward = venv.reward
    kind = _RingCollector(act=venv.actor_act, push=venv.replay_push, action_shape=(), action_dtype=torch.int64, eager_record="_dqn_rec",
                          graphs=venv._actor_graphs, key=("dqn",), set_draw_offset=venv.env.actor_set_draw_offset)
    return _collect_into_ring(venv, kind, max_steps, check_every, int(graph_chunk), reward)


def dqn_update(venv, batch=100, iterations=200, resample=False, draw=None, grads=False):
    """DQLearnAgent::updateDQN on the device (okenv_dqn_update): `iterations` gradient steps of the mean squared
    temporal-difference error on `batch` uniform samples of the ring, with Adam, in place in the parameters the device actor acts with
    (venv.enable_actor, venv.enable_learner(lr=1e-4) and venv.enable_replay first; no sync_actor afterwards, venv.pull_actor() brings
    them back to the module).  resample=False draws one batch for all iterations, as the reference does; True draws a fresh one per
    iteration (its commented alternative).  draw: the number of the first draw; by default a count kept on `venv`, so that every call
    samples afresh.

    Everything is enqueued on the environment's stream; the ring's size is read on the device and nothing is read back.  Returns the
    loss of every iteration as a device tensor [iterations]; with grads=True a dict with "loss", "grad_policy" and "index" (the slots
    of the last iteration's batch)."""
    used = int(iterations) if resample else 1
    if draw is None:
        draw = venv._dqn_draw
        venv._dqn_draw = (draw + used) % 2 ** 32
    out = {"loss": torch.empty(int(iterations), dtype=torch.float32, device=venv.device)}
    if grads:
        out["grad_policy"] = torch.empty(venv.env.actor_num_params()[0], dtype=torch.float32, device=venv.device)
        out["index"] = torch.empty(int(batch), dtype=torch.int32, device=venv.device)
    venv.env.dqn_update(batch, iterations, resample, draw, out)
    venv._update_inputs = out  # alive until the next update: the kernels are only enqueued
    return out if grads else out["loss"]


def collect_episode_ddpg(venv, max_steps=None, check_every=8, graph_chunk=0, reward=None):
    """One episode of ddpg_sim.cpp:55-95 on the device: reset, then `ddpg_act -> step -> ddpg_replay_push` until every agent has
    crashed (tested every `check_every` steps) or `max_steps` steps have run.  The transitions go straight into the ring of
    venv.enable_ddpg_replay.  reward: None for the reference's +1 per step, "tracker" for the environment's own `reward` tensor, or a
    device tensor [N] that the caller keeps up to date.

    graph_chunk = K > 0: K iterations are captured once into a HIP graph (kept on `venv` until the ring is re-created) and replayed;
    the test runs once per chunk.  Without auto-reset the graph's last node advances the word the actor adds to its draw index, so
    replays keep drawing fresh exploration noise; eager and chunked episodes fill the ring with the same bits.

    Returns {"steps": steps taken}; a multiple of K with a graph."""
    assert getattr(venv, "_ddpg_nets", None) is not None, "call venv.enable_ddpg(actor, critic) first"
    assert getattr(venv, "ddpg_push_all", None) is not None, "call venv.enable_ddpg_replay(capacity) first"
    assert not venv.auto_reset or max_steps is not None, "with auto-reset on the episode never ends: pass max_steps"
    if isinstance(reward, str):
        assert reward == "tracker" and venv.reward_kind is not None, 'reward="tracker" needs a VectorEnvironment with a reward'
        reward = venv.reward
    kind = _RingCollector(act=venv.ddpg_act, push=venv.ddpg_replay_push, action_shape=(2,), action_dtype=torch.float32, eager_record="_ddpg_rec",
                          graphs=venv._ddpg_graphs, key=(), set_draw_offset=venv.env.ddpg_set_draw_offset)
    return _collect_into_ring(venv, kind, max_steps, check_every, int(graph_chunk), reward)


def ddpg_update(venv, batch=250, iterations=50, resample=True, draw=None, grads=False):
    """DDPGAgent::update on the device (okenv_ddpg_update): `iterations` iterations of the critic's step, the
    actor's step through the stepped critic and both soft updates on `batch` uniform samples of the ring, in place in the parameters
    the device actor acts with (venv.enable_ddpg and venv.enable_ddpg_replay first; venv.pull_ddpg() brings them back to the
    modules).  resample=True draws a fresh batch per iteration, as the reference does (one sample() per update() call).  draw: the
    number of the first draw; by default a count kept on `venv`.

    Everything is enqueued on the environment's stream and nothing is read back.  Returns (critic_loss, actor_loss), device tensors
    [iterations]; with grads=True a dict that also holds "grad_critic", "grad_actor" and "index"."""
    used = int(iterations) if resample else 1
    if draw is None:
        draw = venv._ddpg_draw
        venv._ddpg_draw = (draw + used) % 2 ** 32
    out = {"critic_loss": torch.empty(int(iterations), dtype=torch.float32, device=venv.device),
           "actor_loss": torch.empty(int(iterations), dtype=torch.float32, device=venv.device)}
    if grads:
        na, nc = venv.env.ddpg_num_params()
        out["grad_actor"] = torch.empty(na, dtype=torch.float32, device=venv.device)
        out["grad_critic"] = torch.empty(nc, dtype=torch.float32, device=venv.device)
        out["index"] = torch.empty(int(batch), dtype=torch.int32, device=venv.device)
    venv.env.ddpg_update(batch, iterations, resample, draw, out)
    venv._update_inputs = out  # alive until the next update: the kernels are only enqueued
    return out if grads else (out["critic_loss"], out["actor_loss"])


# ---- continuous REINFORCE --------------------------------------------------------------------------------

def _gauss_fields(venv):
    return {"state": ((venv.num_rays,), torch.float32), "eps": ((2,), torch.float32), "pre": ((2,), torch.float32), "action": ((2,), torch.float32),
            "logp": ((), torch.float32), "alive": ((), torch.bool), "reward": ((), torch.float32)}


def _gauss_act_step_record(venv, slot, prev, crash_reward):
    """One iteration of collect_episode_gauss into the row `slot`: gauss_act -> step -> reward.  The reward is the distance moved in
    the step, |pos - prev_pos| with prev_pos refreshed every step, and `crash_reward` on the crashing step (reinforce_sim.cpp:67-73)."""
    venv.gauss_act({k: v for k, v in slot.items() if k != "reward"})
    prev[0].copy_(venv.pos_x)
    prev[1].copy_(venv.pos_y)
    venv.step()
    dx, dy = venv.pos_x - prev[0], venv.pos_y - prev[1]
    moved = torch.sqrt(dx * dx + dy * dy)
    slot["reward"].copy_(moved.masked_fill_(venv.done, crash_reward))


def collect_episode_gauss(venv, max_steps=None, check_every=8, graph_chunk=0, crash_reward=-5.0):
    """The episode loop of RLRacers/ReinforceContinuous (reinforce_sim.cpp:46-108) with the acting on the device: `gauss_act -> step
    -> reward` for the actor given to venv.enable_gauss_actor, eagerly or, with graph_chunk = K > 0, as a replayed HIP graph of K
    iterations (collect_episode_device's contract: rows past the step in which the last agent crashed are trimmed).  The reward comes
    from torch elementwise operations on the position fields.  Returns a dict of device tensors: states [T, N, R], eps, pre, actions
    [T, N, 2], log_probs, rewards [T, N], alive [T, N] bool.  (While acting greedily nothing is drawn and eps is left as allocated.)"""
    assert not venv.auto_reset or max_steps is not None, "with auto-reset on the episode never ends: pass max_steps"
    assert getattr(venv, "_gauss_nets", None) is not None, "call venv.enable_gauss_actor(policy) first"
    K = int(graph_chunk)
    block = 256 if K <= 0 else K * max(1, 256 // K)
    if max_steps is not None:
        block = max_steps if K <= 0 else K * ((max_steps + K - 1) // K)
    buf = _EpisodeBuffers(venv, block, False, _gauss_fields(venv))
    crash_reward = float(crash_reward)

    def scratch():
        prev = torch.empty((2, venv.num_envs), dtype=torch.float32, device=venv.device)
        prev[0].copy_(venv.pos_x)
        dx = venv.pos_x - prev[0]
        torch.sqrt(dx * dx + dx).masked_fill_(venv.done, crash_reward)  # torch's own kernels are loaded before a capture
        return prev

    def build():
        chunk = _EpisodeBuffers(venv, K, False, _gauss_fields(venv)).rows(0, K)
        prev = scratch()
        chunk["reward"][0].copy_(prev[0])
        return (lambda k: _gauss_act_step_record(venv, {name: t[k] for name, t in chunk.items()}, prev, crash_reward)), chunk

    def copy_rows(steps, chunk):
        for name, dst in buf.rows(steps, K).items():
            dst.copy_(chunk[name])

    eager_prev = scratch() if K <= 0 else None
    captured = _Chunk(K=K, graphs=venv._gauss_graphs, key=(K, crash_reward), set_draw_offset=venv.env.gauss_set_draw_offset, build=build,
                      after_replay=copy_rows)
    _, steps = _run_episode(venv, lambda t: _gauss_act_step_record(venv, buf.slot(t), eager_prev, crash_reward), max_steps, check_every, captured)
    out = buf.finish(steps)
    T = steps
    if not venv.auto_reset:
        T = int(out["alive"].any(dim=1).sum())
    if max_steps is not None:
        T = min(T, max_steps)
    return {"states": out["state"][:T], "eps": out["eps"][:T], "pre": out["pre"][:T], "actions": out["action"][:T], "log_probs": out["logp"][:T],
            "rewards": out["reward"][:T], "alive": out["alive"][:T]}


def prepare_gauss_batch(venv, ep, gamma=0.99, normalize="returns"):
    """From the dict collect_episode_gauss returns to the continuous learner's batch on the device: okenv_batch_prepare without action
    and prob (discounted returns per agent with `alive` as the episode boundary, normalised over the M alive samples -- the
    reference's (G - mean) / (std + eps) -- and the alive samples packed in step-major order), then eps and pre gathered by the
    samples' flat indices.  Returns a dict of device tensors: states [M, R], eps, pre [M, 2], returns [M], index [M] i32, count (an
    int: the call waits for the stream once to read it) and stats."""
    rewards, alive = ep["rewards"], ep["alive"]
    T, N = rewards.shape
    R = ep["states"].shape[2]
    dev = rewards.device
    if alive.dtype not in (torch.bool, torch.uint8):
        alive = alive != 0
    record = [_rows_of(rewards.float(), 1), _rows_of(alive, 1)]
    if len({s for _, s in record}) > 1:
        record = [(x.contiguous(), N) for x, _ in record]
    state, field_stride = _rows_of(ep["states"].float(), R)
    cap = T * N
    out = {"state": torch.empty((cap, R), dtype=torch.float32, device=dev), "ret": torch.empty(cap, dtype=torch.float32, device=dev),
           "index": torch.empty(cap, dtype=torch.int32, device=dev), "stats": torch.empty(capi.BATCH_STATS_BYTES // 8, dtype=torch.float64, device=dev)}
    venv.env.batch_prepare(T, N, {"reward": record[0][0], "alive": record[1][0], "state": state}, out, state_width=R, record_stride=record[0][1],
                           field_stride=field_stride, gamma=gamma, lam=1.0, normalize=_NORMALIZE[normalize])
    M = venv.env.batch_count()  # waits for the stream: the inputs above may go now
    index = out["index"][:M]
    flat = index.long()
    return {"states": out["state"][:M], "eps": ep["eps"].reshape(-1, 2)[flat].contiguous(), "pre": ep["pre"].reshape(-1, 2)[flat].contiguous(),
            "returns": out["ret"][:M], "index": index, "count": M, "stats": out["stats"]}


def reinforce_continuous_update(venv, batch, slice=16384, accumulate=True, reduce="sum", grad="reference", shuffle=False, grads=False):
    """ReinforceAgent::updatePolicy of RLRacers/ReinforceContinuous on the device (okenv_gauss_update) for the
    dict prepare_gauss_batch returns: loss = sum of -log_prob * return over the M samples, its gradient through the two-hidden-layer
    network and log_std, one Adam step, in place in the parameters the device actor acts with (venv.enable_gauss_actor,
    venv.enable_gauss_learner first; venv.pull_gauss() brings them back to the module).

    grad "reference": the gradient autograd gives for the reference's graph, in which the pre-tanh sample is not detached (all of it
    flows through the tanh correction); "score": the score-function estimator.  slice, accumulate, reduce and shuffle are
    reinforce_update's.  Everything is enqueued on the environment's stream; nothing is read back.  Returns a dict of device tensors:
    loss [steps] and, with grads=True, grad of the last step."""
    assert getattr(venv, "gauss_learner_enabled", False), "call venv.enable_gauss_learner() first"
    M = int(batch["states"].shape[0])
    dev = batch["states"].device
    data = {"state": batch["states"].float().contiguous(), "eps": batch["eps"].float().contiguous(), "pre": batch["pre"].float().contiguous(),
            "ret": batch["returns"].reshape(-1).float().contiguous()}
    order = torch.randperm(M, device=dev).to(torch.int32).contiguous() if shuffle else None
    out = {"loss": torch.empty(1 if accumulate else (M + slice - 1) // slice, dtype=torch.float32, device=dev)}
    if grads:
        out["grad"] = torch.empty(venv.env.gauss_num_params(), dtype=torch.float32, device=dev)
    venv.env.gauss_update(data, M, slice, accumulate, reduce, grad, order, out)
    venv._update_inputs = (data, order)  # alive until the next update: the kernels are only enqueued
    return out


# ---- guided cost learning --------------------------------------------------------------------------------

def gcl_expert_rows(demonstrations):
    """The expert bank's rows from the dict demonstrations.collect_demonstrations returns (ReadExpertData.hpp:98,111), alive rows only:
    state [E, R] = (rel_x^2 + rel_y^2) / 200^2 and action [E, 2] = (((throttle / 100) - 0.5) * 2, steering / 10).  Every operation is
    one torch kernel and the divisions are tensor by tensor, so the state is the device actor's own, bit for bit (torch divides a tensor
    by a Python number as a multiplication by the reciprocal)."""
    rel, actions, alive = demonstrations["rel_xy"].float(), demonstrations["actions"].float(), demonstrations["alive"]
    keep = (alive != 0).reshape(-1)
    rel = rel.reshape(-1, rel.shape[-2], 2)[keep]
    actions = actions.reshape(-1, 2)[keep]
    xx, yy = rel[..., 0] * rel[..., 0], rel[..., 1] * rel[..., 1]
    total = xx + yy
    state = total / torch.full_like(total, 40000.0)
    thr = actions[:, 0] / torch.full_like(actions[:, 0], 100.0)
    thr = (thr - 0.5) * 2.0
    steer = actions[:, 1] / torch.full_like(actions[:, 1], 10.0)
    return state.contiguous(), torch.stack([thr, steer], dim=1).contiguous()


def _gcl_fields(venv):
    pair = ((2,), torch.float32)
    return {"state": ((venv.num_rays,), torch.float32), "eps": pair, "pre": pair, "squashed": pair, "action": pair, "logp": ((), torch.float32),
            "alive": ((), torch.bool)}


def _gcl_act_step_record(venv, slot):
    """One iteration of collect_episode_gcl into the row `slot`: gcl_act -> step.  The reward is the cost network's (gcl_rewards)."""
    venv.gcl_act(slot)
    venv.step()


def collect_episode_gcl(venv, max_steps, check_every=8, graph_chunk=0):
    """A rollout of `max_steps` steps of the reference's guided-cost-learning agent (GCLAgent.hpp:102-135, main.cpp:84-112) with the
    acting on the device: `gcl_act -> step` for the policy given to venv.enable_gcl, eagerly or, with graph_chunk = K > 0, as a replayed
    HIP graph of K iterations (then max_steps is rounded up to a multiple of K and trimmed afterwards).  Auto-reset must be on: the
    reference re-places a crashed agent and goes on, and a row recorded while an agent stands crashed is marked dead.  Returns a dict of
    device tensors: states [T, N, R], eps, pre, squashed, actions [T, N, 2], log_probs [T, N], alive [T, N] bool."""
    assert venv.auto_reset, "create the VectorEnvironment with auto_reset=True: the reference re-places crashed agents and goes on"
    assert getattr(venv, "_gcl_nets", None) is not None, "call venv.enable_gcl(policy, value, cost) first"
    K = int(graph_chunk)
    block = max_steps if K <= 0 else K * ((max_steps + K - 1) // K)
    buf = _EpisodeBuffers(venv, block, False, _gcl_fields(venv))

    def build():
        chunk = _EpisodeBuffers(venv, K, False, _gcl_fields(venv)).rows(0, K)
        return (lambda k: _gcl_act_step_record(venv, {name: t[k] for name, t in chunk.items()})), chunk

    def copy_rows(steps, chunk):
        for name, dst in buf.rows(steps, K).items():
            dst.copy_(chunk[name])

    captured = _Chunk(K=K, graphs=venv._gcl_graphs, key=K, set_draw_offset=venv.env.gcl_set_draw_offset, build=build, after_replay=copy_rows)
    _, steps = _run_episode(venv, lambda t: _gcl_act_step_record(venv, buf.slot(t)), max_steps, check_every, captured)
    out = buf.finish(steps)
    T = min(steps, max_steps)
    return {"states": out["state"][:T], "eps": out["eps"][:T], "pre": out["pre"][:T], "squashed": out["squashed"][:T], "actions": out["action"][:T],
            "log_probs": out["logp"][:T], "alive": out["alive"][:T]}


def gcl_rewards(venv, ep):
    """rewards [T, N] = -cost(state, squashed action) of every row of the dict collect_episode_gcl returns, with the device's cost
    network as it stands (okenv_gcl_cost): one kernel, no synchronisation."""
    T, N = ep["alive"].shape
    states, squashed = ep["states"].reshape(T * N, -1).contiguous(), ep["squashed"].reshape(T * N, 2).contiguous()
    cost = torch.empty(T * N, dtype=torch.float32, device=states.device)
    venv.env.gcl_cost(states, squashed, cost)
    venv._gcl_cost_inputs = (states, squashed)  # alive until the next call: the kernel is only enqueued
    return (-cost).reshape(T, N)


def gcl_cost_update(venv, ep, expert_samples=None, grads=False):
    """One step of the cost network on the device (okenv_gcl_cost_update, main.cpp:150-176): BCEWithLogits(c_expert, 0) +
    BCEWithLogits(c_policy, 1), the policy samples being the alive rows of the dict collect_episode_gcl returns and the expert samples
    `expert_samples` uniform draws with replacement from the bank (default: as many as policy samples).  The call reads the number of
    alive rows (one synchronisation).  Returns a dict of device tensors: loss [1] and, with grads=True, grad."""
    assert getattr(venv, "gcl_learner_enabled", False), "call venv.enable_gcl_learner() first"
    keep = ep["alive"].reshape(-1)
    data = {"state": ep["states"].reshape(keep.numel(), -1)[keep].contiguous(), "squashed": ep["squashed"].reshape(-1, 2)[keep].contiguous()}
    Mp = int(data["state"].shape[0])
    out = {"loss": torch.empty(1, dtype=torch.float32, device=keep.device)}
    if grads:
        out["grad"] = torch.empty(venv.env.gcl_num_params("cost"), dtype=torch.float32, device=keep.device)
    venv.env.gcl_cost_update(data, Mp, Mp if expert_samples is None else int(expert_samples), out)
    venv._gcl_cost_update_inputs = data  # alive until the next update: the kernels are only enqueued
    return out


def prepare_gcl_batch(venv, ep, rewards, gamma=0.99):
    """From the dict collect_episode_gcl returns and its rewards [T, N] to the policy / value update's batch: prepare_batch without a
    value plane and without normalisation (discounted returns per agent, a dead row an episode boundary, the alive samples packed in
    step-major order; the recorded log-probabilities ride in its probability plane), then pre gathered by the samples' flat indices.
    Returns a dict of device tensors: states [M, R], pre [M, 2], log_probs [M], returns [M], index [M] i32, count and stats."""
    T, N = rewards.shape
    plain = {"states": ep["states"], "actions": torch.zeros((T, N), dtype=torch.int64, device=rewards.device), "log_probs": ep["log_probs"],
             "rewards": rewards, "alive": ep["alive"]}
    batch = prepare_batch(venv, plain, gamma=gamma, lam=None, normalize=False)
    return {"states": batch["states"], "pre": ep["pre"].reshape(-1, 2)[batch["index"].long()].contiguous(), "log_probs": batch["log_probs"],
            "returns": batch["returns"], "index": batch["index"], "count": batch["count"], "stats": batch["stats"]}


def gcl_policy_update(venv, batch, slice=16384, accumulate=True, reduce="mean", shuffle=False, grads=False):
    """updatePolicy of RLRacers/GuidedCostLearning on the device (okenv_gcl_policy_update, GCLAgent.hpp:146-177) for the dict
    prepare_gcl_batch returns: advantages returns - V(state), normalised over the batch; the clipped surrogate on the ratio of the
    recomputed to the recorded log-probability of the recorded pre-squash sample; the value network's squared error; one Adam step on
    each, in place in the parameters the device acts with (venv.pull_gcl() brings them back to the modules).  slice, accumulate, reduce
    and shuffle are reinforce_update's; the reference is one step on the mean.  Everything is enqueued on the environment's stream.
    Returns a dict of device tensors: policy_loss, value_loss (float32), clipped (int32), one per optimiser step, adv [M] and, with
    grads=True, grad_policy and grad_value of the last step."""
    assert getattr(venv, "gcl_learner_enabled", False), "call venv.enable_gcl_learner() first"
    M = int(batch["states"].shape[0])
    dev = batch["states"].device
    data = {"state": batch["states"].float().contiguous(), "pre": batch["pre"].float().contiguous(), "logp": batch["log_probs"].reshape(-1).float().contiguous(),
            "ret": batch["returns"].reshape(-1).float().contiguous()}
    order = torch.randperm(M, device=dev).to(torch.int32).contiguous() if shuffle else None
    steps = 1 if accumulate else (M + slice - 1) // slice
    out = {"policy_loss": torch.empty(steps, dtype=torch.float32, device=dev), "value_loss": torch.empty(steps, dtype=torch.float32, device=dev),
           "clipped": torch.empty(steps, dtype=torch.int32, device=dev), "adv": torch.empty(M, dtype=torch.float32, device=dev)}
    if grads:
        out["grad_policy"] = torch.empty(venv.env.gcl_num_params("policy"), dtype=torch.float32, device=dev)
        out["grad_value"] = torch.empty(venv.env.gcl_num_params("value"), dtype=torch.float32, device=dev)
    venv.env.gcl_policy_update(data, M, slice, accumulate, reduce, order, out)
    venv._update_inputs = (data, order)  # alive until the next update: the kernels are only enqueued
    return out


def batch_stats(batch):
    """The statistics of a prepare_batch result as a dict (one small copy to the host): sum_ret, sumsq_ret, sum_adv, sumsq_adv (fp64, in
    the rule's order), mean_ret, std_ret, mean_adv, std_adv, count."""
    return capi.batch_stats_dict(batch["stats"].cpu().numpy().view("uint8"))


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
