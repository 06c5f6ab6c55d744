"""The learners' device kernels at the edges of their launch geometry (openkitchen_amd/csrc/ok_learn.h, ok_dqn.h, ok_ddpg.h): every
chunk count 1 .. 130 of the tree the three step kernels share (okLearnColumnSum), the same tree at the widths the examples run,
calls of different B on one handle (the partials' buffer grows and is reused while larger than needed), pushes over more than
256 workgroups (okReplayScatterKernel's count loop), Deep-Q's ring and DDPG's on one handle, and the two whole-episode updates
(REINFORCE's and the Gaussian actor's) on one handle.  Everything is compared bit for bit with the host entries, whose own link to
the numpy restatements at these B is in tests/test_learn_rule.py, test_dqn_rule.py and test_ddpg_rule.py."""
import numpy as np
import pytest
import torch

import _learn_numpy as L_
import test_gpu_ddpg as G
import test_gpu_dqn as Q
import test_gpu_gauss as C
import test_gpu_learn as P
import test_gpu_reinforce as F

pytestmark = pytest.mark.gpu
f32 = np.float32
LEARNERS = ("ppo", "dqn", "ddpg")
SMALLEST = {"ppo": (1, 1, 2, 1), "dqn": (1, 1, 2), "ddpg": (1, 1, 1)}
EXAMPLE = {"ppo": (5, 128, 3, 128), "dqn": (5, 128, 5), "ddpg": (5, 128, 128)}
LARGEST = {"ppo": (64, 256, 8, 256), "dqn": (64, 256, 8), "ddpg": (62, 256, 256)}
N_RING, RING = 257, 1000  # ring_on_device pushes 4 x 257 transitions of real steps: a full ring of 1000


def sweep_batch(C):
    """B of chunk count C: C - 1 full chunks and a last one of 1 + C mod 32 positions (every fill 1 .. 32 occurs in 1 .. 130)."""
    return 32 * (C - 1) + 1 + C % 32


class PpoCases:
    """One handle; a case is a fresh random batch of M = B samples in one minibatch, fresh parameters and zeroed moments."""

    def __init__(self, gpu, shape, seed):
        self.gpu, self.shape, self.rng = gpu, shape, np.random.default_rng(seed)
        self.lp = gpu.capi.learner_params(**P.HP)
        self.dev = P.handle_for(gpu, shape, P.fresh_state(self.rng, shape))

    def run(self, B, case, iterations=1, tail=0):
        """`tail` > 0 adds a second, partial minibatch of that many positions to every epoch."""
        shape, rng, M = self.shape, self.rng, B + tail
        batch = P.random_batch(rng, shape, M, with_adv=case % 2 == 1)
        order = np.stack([rng.permutation(M) for _ in range(iterations)]).astype(np.int32) if case % 3 != 0 else None
        st = P.fresh_state(rng, shape, 0.3 if shape[0] < 64 else 0.05)
        self.dev.actor_set_params(st["policy"], st.get("value"))
        self.dev.learner_reset()
        got = P.on_device(self.dev, batch, M, B, iterations, order, shape)
        want_state, want = self.gpu.ppo_update_host(self.lp, shape, st, batch, B, iterations, order)
        what = ("ppo", shape, B, case, iterations, tail)
        assert set(got) == set(P.OUTS), what
        P.assert_outputs_equal(got, want, what)
        P.assert_state_equal(P.device_state(self.dev), want_state, what)

    def close(self):
        self.dev.close()


class DqnCases:
    """One handle and one ring of 1000 real transitions; a case is fresh parameters, a new learner (zeroed moments, t = 0) and the
    mask-done / target-network switches of its number."""

    def __init__(self, gpu, shape, seed):
        R, H, A = shape
        self.gpu, self.shape, self.rng = gpu, shape, np.random.default_rng(seed)
        self.lp = gpu.capi.learner_params(**Q.HP)
        self.dev, _ = Q.make_env(gpu, N_RING, R, H, A, seed=seed)
        self.ring = Q.ring_on_device(gpu, self.dev, N_RING, R, RING, self.rng)

    def run(self, B, case, iterations=1, tail=0):
        gpu, dev, shape, rng = self.gpu, self.dev, self.shape, self.rng
        R, H, A = shape
        resample, mask_done, target_on = case % 2 == 1, case % 3 == 1, case % 4 >= 2
        policy = (rng.standard_normal(L_.n_params(R, H, A)) * (0.3 if R < 64 else 0.05)).astype(f32)
        target = (policy + rng.standard_normal(policy.size).astype(f32) * f32(0.05)) if target_on else None
        st = {"policy": policy, "policy_m": np.zeros_like(policy), "policy_v": np.zeros_like(policy), "t": 0}
        if target_on:  # the target network is a copy of what the actor holds at sync time
            dev.actor_set_params(target, None)
            dev.dqn_params(0.99, mask_done, True, seed=R + case)
            dev.dqn_sync_target()
        else:
            dev.dqn_params(0.99, mask_done, False, seed=R + case)
        dev.actor_set_params(policy, None)
        dev.learner_create(**Q.HP)
        cfg = gpu.capi.dqn_config(0.99, mask_done, target_on, R + case)
        got = Q.device_update(dev, shape, B, iterations, resample, 5 + case)
        want_state, want = gpu.dqn_update_host(self.lp, cfg, shape, st, self.ring, B, iterations, resample, 5 + case, target)
        what = ("dqn", shape, B, case, iterations, resample, mask_done, target_on)
        assert set(got) == {"loss", "grad_policy", "index"}, what
        Q.assert_update_equal(dev, got, want_state, want, what)

    def close(self):
        self.dev.close()


class DdpgCases:
    """One handle and one ring of 1000 real transitions; a case is a new DDPG object on the same ring (fresh parameters, targets
    equal to them, zeroed moments, t = 0) with the tau of its number."""

    def __init__(self, gpu, shape, seed):
        R, H, Hc = shape
        self.gpu, self.shape, self.rng = gpu, shape, np.random.default_rng(seed)
        self.dev, _, _ = G.make_env(gpu, N_RING, R, H, Hc, env_seed=seed, noise=(5.0, 0.5))
        self.ring = G.ring_on_device(self.dev, N_RING, R, RING)

    def run(self, B, case, iterations=1, tail=0):
        gpu, dev, rng = self.gpu, self.dev, self.rng
        R, H, Hc = self.shape
        resample, tau = case % 2 == 1, (0.005, 1.0, 0.0, 0.005)[case % 4]
        cfg = dict(G.CFG, tau=tau, sample_seed=R + case, noise=(5.0, 0.5))
        dev.ddpg_create(H, Hc, **cfg)  # (the ring stays; parameters, moments and t are forgotten)
        scale = 0.3 if R < 62 else 0.05
        actor, critic = (rng.standard_normal(G.n_actor(R, H)) * scale).astype(f32), (rng.standard_normal(G.n_critic(R, Hc)) * scale).astype(f32)
        dev.ddpg_set_params(actor, critic)
        st = {"actor": actor, "critic": critic, "actor_target": actor, "critic_target": critic, "t": 0}
        for net in ("actor", "critic"):
            st[net + "_m"], st[net + "_v"] = np.zeros_like(st[net]), np.zeros_like(st[net])
        got = G.device_update(dev, R, H, Hc, B, iterations, resample, 5 + case)
        want_state, want = gpu.ddpg_update_host(gpu.capi.ddpg_config(H, Hc, **cfg), R, st, self.ring, B, iterations, resample, 5 + case)
        what = ("ddpg", self.shape, B, case, iterations, resample, tau)
        assert set(got) == set(G.OUTPUTS), what
        G.assert_update_equal(dev, got, want_state, want, what)

    def close(self):
        self.dev.close()


CASES = {"ppo": PpoCases, "dqn": DqnCases, "ddpg": DdpgCases}


# ---- A: every chunk count, smallest network ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("learner", LEARNERS)
def test_every_chunk_count_1_to_130(gpu, learner):
    """One update per C = 1 .. 130 with B = 32 (C - 1) + 1 + C mod 32, on the smallest shape of the ABI (one step workgroup,
    7 live columns for Deep-Q and for each of DDPG's networks, 12 for PPO), one iteration each.  What okLearnColumnSum executes for the first time
    on the device, by C (w is C padded to a power of two; "in place" are the levels h >= 16 of `for (h = w >> 1; h >= kLearnStepRows`):
      C = 9 .. 16    the LDS level h = 8 of the last loop (`for (h = min(w >> 1, 8)`), its guard `i + h < n` false for C < 16 and
                     never false at C = 16; C = 9, 10, ... also has a last chunk of 10, 11, ... positions, and C = 32 k (k = 1 .. 4)
                     a last chunk of ONE position, whose 31 spare groups borrow its sample (with C = 9 .. 16 in the test below)
      C = 17         the first in-place level (h = 16): only thread 0's partial passes the guard `i + h < n`
      C = 18 .. 31   that guard true for the threads r < C - 16 and false for the others
      C = 33 .. 64   two in-place levels (h = 32, 16); at h = 32 a thread owns two partials of one level (i = r and r + 16), the
                     guard cutting the level after the first (C <= 48) or inside the second; no power of two above 32 ran before
      C = 65 .. 128  three in-place levels; four partials per thread at h = 64
      C = 129, 130   w = 256: four in-place levels, eight partials per thread at h = 128, of which only one or two pass the guard
    (for PPO C = 32 was reached before, for Deep-Q nothing above C = 4, for DDPG nothing above C = 8)."""
    cases = CASES[learner](gpu, SMALLEST[learner], seed=11)
    fills = set()
    for C in range(1, 131):
        B = sweep_batch(C)
        assert (B + 31) // 32 == C
        fills.add(B - 32 * (C - 1))
        cases.run(B, case=C)
    assert fills == set(range(1, 33))
    cases.close()


@pytest.mark.parametrize("learner", LEARNERS)
def test_the_lds_level_8_with_a_last_chunk_of_one_position(gpu, learner):
    """C = 9 .. 16 with B = 32 (C - 1) + 1: the LDS level h = 8 of okLearnColumnSum with its guard `i + h < n` (false from i = C - 8
    on), and in the same launch a last chunk of one position, whose 31 spare groups take part in the gradient kernel's shuffles with
    that sample (`g < n ? g : n - 1`) and whose rows the chunk sums must not read.  Both on the smallest shape and on the example's,
    where the last of the step workgroups is partly live."""
    for shape in (SMALLEST[learner], EXAMPLE[learner]):
        cases = CASES[learner](gpu, shape, seed=12)
        for C in range(9, 17):
            cases.run(32 * (C - 1) + 1, case=C)
        cases.close()


# ---- B: the tree at real widths ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("learner", LEARNERS)
def test_the_tree_at_the_examples_width(gpu, learner):
    """The shape of the example and of the bench tool, (5, 128, 3, 128) / (5, 128, 5) / (5, 128, 128): 129, 89 and 73 + 65 step
    workgroups of which the last is partly live (`live = column < cols`), on ONE handle in the order B = 257, 4096, 513, 1500, 1025:
      B = 257   C = 9: the LDS level h = 8, a last chunk of one position
      B = 4096  C = 128: three in-place levels with every guard true, the shape tools/ddpg_bench.py times; the partials' buffer
                grows (the handle frees the old one behind a stream synchronisation)
      B = 513   C = 17: the first in-place level with only thread 0's partial passing, in a buffer that is larger than needed
                and still holds the partials of B = 4096 behind row 17
      B = 1500  C = 47: two in-place levels, at h = 32 the guard passes only a thread's first partial, and not thread 15's (i + 32 < 47 for i < 15)
      B = 1025  C = 33: w = 64 with a single partial beyond 32
    Iterations in {1, 3}, resample, mask-done / the target network and tau in {0.005, 1, 0} rotate with the case number; PPO runs
    M = B + 100, so every epoch has a second minibatch of 100 positions (C = 4) between two large ones."""
    cases = CASES[learner](gpu, EXAMPLE[learner], seed=13)
    for case, B in enumerate((257, 4096, 513, 1500, 1025)):
        cases.run(B, case=case, iterations=(1, 3)[case % 2], tail=100 if learner == "ppo" else 0)
    cases.close()


@pytest.mark.parametrize("learner", LEARNERS)
def test_the_tree_at_the_largest_shape(gpu, learner):
    """(64, 256, 8, 256) / (64, 256, 8) / (62, 256, 256) at B = 1025 (C = 33: two in-place levels), three iterations with a new
    draw each: 2225, 1169 and 1057 + 1041 step workgroups, each column's partials 35 595 / 18 697 / 16 898 and 16 643 floats apart (the stride
    of `x[i * stride]`)."""
    cases = CASES[learner](gpu, LARGEST[learner], seed=14)
    cases.run(1025, case=1, iterations=3)
    cases.close()


# ---- D: pushes over more than 256 workgroups ---------------------------------------------------------------------------------------

BIG_N = 257 * 256 + 1


@pytest.mark.parametrize("learner", ["dqn", "ddpg"])
def test_push_over_more_than_256_workgroups(gpu, learner):
    """N = 65 793 agents, R = 1: 258 workgroups of the push kernels, so okReplayScatterKernel's count loop
    `for (b = threadIdx.x; b < gridDim.x; b += kReplayThreads)` takes a second round in threads 0 and 1 (five workgroups was the
    most before), and the last workgroup holds one agent.  Three consecutive act + step + push per case; capacity 1000 (fewer slots
    than one call's transitions: whole workgroups of selected agents do not survive), 100 000 (wraps at the second call) and 300 000
    (no wrap); masks "random" and "alternating", push-all and a caller's reward rotating as in test_push_equals_host_entry.  Every
    ring field and (size, pushed) against the host entry's ring after each case."""
    N, R = BIG_N, 1
    M = Q if learner == "dqn" else G
    if learner == "dqn":
        dev, _ = Q.make_env(gpu, N, R, 16, 5, seed=9)
        create, ring_of = dev.replay_create, gpu.replay_ring
    else:
        dev, _, _ = G.make_env(gpu, N, R, 16, 8, env_seed=9, noise=(10.0, 1.0))
        create, ring_of = dev.ddpg_replay_create, gpu.ddpg_ring
    rng = np.random.default_rng(N)
    rec = M.record_tensors(N, R)
    case = 1  # (so that push-all meets capacity 100 000: 2 N transitions wrap it at the second call)
    for capacity in (1000, 100_000, 300_000):
        for mask in ("random", "alternating"):
            push_all, own_reward = case % 3 == 1, case % 3 == 2
            case += 1
            create(capacity, push_all)
            host = ring_of(capacity, R)
            reward = torch.from_numpy(rng.standard_normal(N).astype(f32)).cuda() if own_reward else None
            for push in range(3):
                if push == 0:  # (afterwards the flags are what the last step left: crashed agents stay crashed)
                    crashed = (np.arange(N) % 2).astype(np.uint8) if mask == "alternating" else (rng.random(N) < 0.25).astype(np.uint8)
                    dev.set(gpu.capi.F_CRASHED, crashed)
                M.act_step_push(gpu, dev, rec, host, reward, push_all)
            what = (learner, capacity, mask, push_all, own_reward)
            assert host["pushed"] > max(65536, capacity if capacity == 100_000 else 0) and (not push_all or host["pushed"] == 3 * N), what
            M.same_ring(dev, host, what)
    dev.close()


# ---- E: both rings on one handle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("push_all", [False, True])
def test_both_rings_on_one_handle(gpu, push_all):
    """Deep-Q's ring and DDPG's on ONE handle, each with its own counter words and count scratch: N = 300 agents (two workgroups of
    the push kernels, the second partly live), R = 5, both rings of capacity 257, so that the second push of each wraps (with
    push-all the first one already drops its 43 oldest transitions).  The pushes alternate Deep-Q, DDPG, Deep-Q, DDPG, each after
    an act of its own learner and a step, so the recorded actions differ (an index / two floats) and so do the states of the four
    pushes.  Without push-all `alive` selects about half the agents (crashed_ is set to a fresh mask of 45 % before every act, so
    two pushes of about 165 transitions pass 257 with room for the agents that crash in the step between).  Every field and (size, pushed) of both rings against the host entries' rings after every push: a ring that took the
    other's counter, snapshot or counts shows in its slots at once."""
    N, R, capacity = 300, 5, 257
    dev, _ = Q.make_env(gpu, N, R, 16, 5, seed=21)
    assert dev.ddpg_create(16, 8, **dict(G.CFG, noise=(10.0, 1.0))) == (G.n_actor(R, 16), G.n_critic(R, 8))
    rng = np.random.default_rng(21)
    dev.ddpg_set_params((rng.standard_normal(G.n_actor(R, 16)) * 0.3).astype(f32), (rng.standard_normal(G.n_critic(R, 8)) * 0.3).astype(f32))
    dev.replay_create(capacity, push_all)
    dev.ddpg_replay_create(capacity, push_all)
    host_q, host_g = gpu.replay_ring(capacity, R), gpu.ddpg_ring(capacity, R)
    rec_q, rec_g = Q.record_tensors(N, R), G.record_tensors(N, R)
    for push in range(2):
        dev.set(gpu.capi.F_CRASHED, (rng.random(N) < 0.45).astype(np.uint8))
        Q.act_step_push(gpu, dev, rec_q, host_q, None, push_all)
        Q.same_ring(dev, host_q, ("dqn", push, push_all))
        G.same_ring(dev, host_g, ("ddpg before its push", push, push_all))
        dev.set(gpu.capi.F_CRASHED, (rng.random(N) < 0.45).astype(np.uint8))
        G.act_step_push(gpu, dev, rec_g, host_g, None, push_all)
        G.same_ring(dev, host_g, ("ddpg", push, push_all))
        Q.same_ring(dev, host_q, ("dqn after ddpg's push", push, push_all))
    for host in (host_q, host_g):
        assert host["pushed"] > capacity and (not push_all or host["pushed"] == 2 * N), (host["pushed"], push_all)
    if not push_all:  # about half: neither nobody nor everybody
        assert N // 2 < host_q["pushed"] < 2 * N - N // 2, host_q["pushed"]
    dev.close()


# ---- F: both whole-episode updates on one handle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("accumulate", [True, False])
def test_both_sliced_updates_on_one_handle(gpu, accumulate):
    """REINFORCE's update and the Gaussian actor's on ONE handle of 33 agents, R = 5: a shared-network actor (H = 8, A = 3, no value
    network, dropout p = 0.25) with its learner, and a Gaussian actor (H1 = H2 = 8) with a learner of another lr.  They share the loop
    over slices and the join kernel, and must keep their own t, moments, scratch and event log.  M = 70, B = 33: three slices of 33, 33
    and 4 positions, that is 2, 2 and 1 chunks, the last with a fill of 4; a random order; REINFORCE's flat indices from [0, 33 * 3)
    with num_agents = 33 and draw_first = 5.  accumulate on is one step per call, off three.  The calls alternate REINFORCE, Gauss,
    REINFORCE, Gauss, each on a fresh batch; after every call loss, gradient, parameters, both moments and t of the learner just
    updated equal its host entry continued from its own previous state, bit for bit, and the other learner's parameters, moments
    and t are what they were.  The second round runs timed: each timing entry answers two finite positive numbers after its own
    update, and REINFORCE's still does after the Gaussian update that followed it."""
    N, R, M, B = 33, 5, 70, 33
    r_shape, g_shape, p_drop, steps = (R, 8, 3), (R, 8, 8), 0.25, 1 if accumulate else 3
    rng = np.random.default_rng(31 + accumulate)
    r_st, g_st = F.fresh_state(rng, r_shape), C.fresh_state(gpu, rng, g_shape)
    r_hp, g_hp = F.HP, dict(C.HP, lr=0.003)
    dev = F.handle_for(gpu, r_shape, r_st, n_agents=N)
    dev.actor_set_dropout(p_drop, 21)
    assert dev.gauss_create(8, 8, seed=11) == C.n_params(gpu, g_shape)
    dev.gauss_set_params(g_st["params"])
    dev.gauss_learner_create(**g_hp)
    r_cfg = dict(accumulate=accumulate, reduce="mean", num_agents=N, draw_first=5)
    g_cfg = dict(accumulate=accumulate, reduce="sum", grad="reference")

    def timing_ok(times, names):
        return set(times) == set(names) and len(times) == 2 and all(np.isfinite(v) and v > 0.0 for v in times.values())

    for rnd in range(2):
        dev.set_timing(rnd == 1)
        what = ("reinforce", accumulate, rnd)
        batch, order = F.random_batch(rng, r_shape, M, N), rng.permutation(M).astype(np.int32)
        batch["index"] = np.sort(rng.choice(N * 3, M, replace=False)).astype(np.int32)
        got = F.on_device(dev, r_shape, batch, M, B, order=order, **r_cfg)
        r_st, want = gpu.reinforce_update_host(gpu.capi.learner_params(**r_hp), r_shape, r_st, batch, B, p=p_drop, dropout_seed=21, agent_base=0,
                                               order=order, **r_cfg)
        assert set(got) == {"loss", "grad_policy"} and got["loss"].size == steps and r_st["t"] == (rnd + 1) * steps, what
        F.assert_equal(got, F.device_state(dev), want, r_st, what)
        C.assert_equal({}, dev.gauss_state(), {}, g_st, ("gauss after reinforce's update", accumulate, rnd))
        assert rnd == 0 or timing_ok(dev.reinforce_timing(), gpu.capi.REINFORCE_KERNELS), what
        what = ("gauss", accumulate, rnd)
        batch, order = dict(C.random_batch(rng, M), state=rng.random((M, R)).astype(f32)), rng.permutation(M).astype(np.int32)
        got = C.on_device(gpu, dev, g_shape, batch, M, B, order=order, **g_cfg)
        g_st, want = gpu.gauss_update_host(gpu.capi.learner_params(clip=0.0, **g_hp), g_shape, g_st, batch, B, order=order, **g_cfg)
        assert set(got) == {"loss", "grad"} and got["loss"].size == steps and g_st["t"] == (rnd + 1) * steps, what
        C.assert_equal(got, dev.gauss_state(), want, g_st, what)
        F.assert_equal({}, F.device_state(dev), {}, r_st, ("reinforce after gauss's update", accumulate, rnd))
        assert rnd == 0 or (timing_ok(dev.gauss_timing(), gpu.capi.GAUSS_KERNELS) and timing_ok(dev.reinforce_timing(), gpu.capi.REINFORCE_KERNELS)), what
    dev.close()
