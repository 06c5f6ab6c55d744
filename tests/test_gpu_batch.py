"""From a recorded episode to the learner's batch on the device (okenv_batch_prepare, openkitchen_amd/csrc/ok_batch.h): bit-equal to
the host entry that shares its rule for every output, the same bits from every launch shape, end to end behind
collect_episode_device against the parent's torch path, auto-reset records, validation on a handle and the example."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _batch_numpy as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPO_FAN = np.array([-70, -30, 0, 30, 70], dtype=np.float32)
DENSE = ("state", "action", "prob", "ret", "adv", "index")
ALL = DENSE + ("ret_plane", "adv_plane", "stats", "count")


@pytest.fixture(scope="module")
def handle(gpu):
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), 8, ray_angles_deg=PPO_FAN)  # lends its stream and scratch only
    yield dev
    dev.close()


def on_device(gpu, dev, rec, N, want=ALL, gamma=0.99, lam=0.95, normalize=3, use_value=True, use_last=True, block_threads=0):
    """okenv_batch_prepare on the record's arrays (padded rows passed with their strides), read back in the form of
    batch_prepare_host: dense outputs cut to M, planes, statistics, the count word and M from okenv_batch_count.  The unused tail of
    every dense output must be left alone."""
    T, S = rec["reward"].shape
    R = rec["state"].shape[2]
    names = ["reward", "alive", "state", "action", "prob"] + (["value"] if use_value else []) + (["last_value"] if use_value and use_last else [])
    inputs = {k: torch.from_numpy(rec[k]).cuda() for k in names}
    cap = T * N
    shapes = {"state": ((cap, R), torch.float32), "action": ((cap,), torch.int64), "prob": ((cap,), torch.float32), "ret": ((cap,), torch.float32),
              "adv": ((cap,), torch.float32), "index": ((cap,), torch.int32), "ret_plane": ((T, N), torch.float32), "adv_plane": ((T, N), torch.float32),
              "stats": ((gpu.capi.BATCH_STATS_BYTES,), torch.uint8), "count": ((1,), torch.int32)}
    out = {k: torch.full(shapes[k][0], 77, dtype=shapes[k][1], device="cuda") for k in want if use_value or k not in ("adv", "adv_plane")}
    torch.cuda.synchronize()
    dev.batch_prepare(T, N, inputs, out, state_width=R, record_stride=S, field_stride=S, gamma=gamma, lam=lam, normalize=normalize,
                      block_threads=block_threads)
    M = dev.batch_count()
    res = {"M": M}
    for k, v in out.items():
        a = v.cpu().numpy()
        if k in DENSE:
            assert np.all(a[M:] == 77), "%s: written past M" % k
            a = a[:M]
        res[k] = gpu.capi.batch_stats_dict(a) if k == "stats" else a
    return res


def on_host(gpu, rec, N, want=None, gamma=0.99, lam=0.95, normalize=3, use_value=True, use_last=True):
    return gpu.batch_prepare_host(rec["reward"], rec["alive"], rec["value"] if use_value else None,
                                  rec["last_value"] if use_value and use_last else None, rec["state"], rec["action"], rec["prob"], num_agents=N,
                                  gamma=gamma, lam=lam, normalize=normalize, want=want)


@pytest.mark.parametrize("T", (1, 7, 600, 3000))
@pytest.mark.parametrize("N", (1, 257, 4096))
def test_device_equals_host(gpu, handle, T, N):
    """Every output, M and the statistics included, for the three kinds of mask (monotone, interior boundaries, the edge cases), both
    reward kinds, padded (strided) rows, with and without the value plane and the bootstrap."""
    for k, mask in enumerate(B.MASKS):
        rec = B.make_record(T, N, mask, B.REWARDS[k % 2], seed=T * 13 + N + k, pad=(0, 7)[k % 2])
        for use_value, use_last, lam, normalize in ((True, True, 0.95, 3), (False, False, 1.0, 1)) if k < 2 else ((True, k % 2 == 0, 1.0, 3),):
            got = on_device(gpu, handle, rec, N, lam=lam, normalize=normalize, use_value=use_value, use_last=use_last)
            want = on_host(gpu, rec, N, lam=lam, normalize=normalize, use_value=use_value, use_last=use_last)
            assert got["M"] == want["M"] == int(got["count"][0]) == got["stats"]["count"]
            assert set(got) == set(want)
            B.assert_same(got, want, (T, N, mask, use_value))


def test_null_slots_and_switches(gpu, handle):
    rec = B.make_record(600, 257, "interior", "progress", seed=21, pad=3)
    for normalize, lam in ((0, 0.0), (1, 0.95), (2, 1.0), (3, 0.5)):
        want = on_host(gpu, rec, 257, lam=lam, normalize=normalize)
        for leave_out in ALL:
            names = tuple(k for k in ALL if k != leave_out)
            got = on_device(gpu, handle, rec, 257, want=names, lam=lam, normalize=normalize)
            assert leave_out not in got
            B.assert_same(got, want, (normalize, leave_out))
    got = on_device(gpu, handle, rec, 257, want=())
    assert got == {"M": want["M"]}


def test_same_bits_from_every_launch(gpu, handle):
    """A second call gives identical bits, and so does every workgroup size of the column walk (the knob
    okenv_batch_params.block_threads; the other four kernels have one fixed size each): the order of the sums and of the samples
    belongs to the rule, not to the launch."""
    for T, N, mask in ((600, 4096, "interior"), (3000, 257, "monotone"), (7, 1, "one_to_last")):
        rec = B.make_record(T, N, mask, "progress", seed=T + N)
        first = on_device(gpu, handle, rec, N)
        for block_threads in (0, 64, 128, 256, 512, 1024):
            again = on_device(gpu, handle, rec, N, block_threads=block_threads)
            assert set(again) == set(first)
            B.assert_same(again, first, (T, N, block_threads))


def make_venv(N, auto_reset, seed=5):
    from openkitchen_amd.torch_env import VectorEnvironment
    return VectorEnvironment("Silverstone", N, ray_angles_deg=PPO_FAN, auto_reset=auto_reset, seed=seed, reward="step")


def ppo_networks(seed=0):
    torch.manual_seed(seed)
    actor = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 3), torch.nn.Softmax(dim=1)).cuda()
    critic = torch.nn.Sequential(torch.nn.Linear(5, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)).cuda()
    return actor, critic


def episode_as_record(ep):
    return {"reward": ep["rewards"].cpu().numpy(), "alive": ep["alive"].cpu().numpy().astype(np.uint8), "value": ep["values"].cpu().numpy(),
            "state": ep["states"].cpu().numpy(), "action": ep["actions"].cpu().numpy(), "prob": ep["log_probs"].cpu().numpy()}


@pytest.mark.parametrize("graph_chunk", (0, 32))
def test_end_to_end_against_the_parent_path(gpu, graph_chunk):
    """collect_episode_device on Silverstone, then prepare_batch against lines 56-62 of the example as the parent has them, computed
    with torch on the same tensors: states, actions, log-probs and unnormalised returns exactly equal; normalised returns within the
    derived bound of torch's float64 over the alive samples."""
    from openkitchen_amd.rollout import batch_stats, collect_episode_device, discounted_returns, prepare_batch

    N = 1024
    venv = make_venv(N, auto_reset=False, seed=3)
    actor, critic = ppo_networks(2)
    venv.enable_actor(actor, critic)
    ep = collect_episode_device(venv, max_steps=3000, graph_chunk=graph_chunk)
    alive = ep["alive"]
    T = alive.shape[0]
    assert T >= 8
    returns = discounted_returns(ep["rewards"] * alive, normalize=False)
    mask = alive.reshape(-1)
    states, actions = ep["states"].reshape(-1, 5)[mask], ep["actions"].reshape(-1)[mask]
    old_logp, ret = ep["log_probs"].reshape(-1)[mask], returns.reshape(-1)[mask]
    raw = prepare_batch(venv, ep, gamma=0.99, normalize=False)
    M = int(mask.sum())
    assert raw["count"] == M and "advantages" not in raw
    assert torch.equal(raw["states"], states) and torch.equal(raw["actions"], actions) and torch.equal(raw["log_probs"], old_logp)
    assert torch.equal(raw["returns"], ret)
    assert torch.equal(raw["index"].long(), torch.nonzero(mask).squeeze(1))
    batch = prepare_batch(venv, ep, gamma=0.99, lam=0.95, normalize=True)
    assert torch.equal(batch["states"], states) and torch.equal(batch["actions"], actions) and torch.equal(batch["log_probs"], old_logp)
    x = ret.double()
    mean64, std64 = float(x.mean()), float(x.std())
    ref = ((x - mean64) / (std64 + float(B.EPS))).cpu().numpy()
    bound, e_mean, e_std = B.normalized_bound(ret.cpu().numpy(), M, mean64, std64, float(x.abs().sum()), float((x * x).sum()))
    err = np.abs(batch["returns"].cpu().numpy().astype(np.float64) - ref)
    print("T %d, M %d, normalised returns: largest error / bound %.3f" % (T, M, float((err / bound).max())))
    assert np.all(err <= bound)
    st = batch_stats(batch)
    assert st["count"] == M and abs(st["mean_ret"] - mean64) <= e_mean and abs(st["std_ret"] - std64) <= e_std
    # and the whole batch equals the host entry on the same record
    want = gpu.batch_prepare_host(**{k: v for k, v in episode_as_record(ep).items()}, gamma=0.99, lam=0.95, normalize=3)
    for mine, theirs in (("states", "state"), ("actions", "action"), ("log_probs", "prob"), ("returns", "ret"), ("advantages", "adv"), ("index", "index")):
        assert np.array_equal(B.bits(batch[mine].cpu().numpy()), B.bits(want[theirs])), mine
    B.assert_same({"stats": st}, {"stats": want["stats"]})
    venv.close()


def test_auto_reset_episode(gpu):
    """max_steps with auto-reset on: columns hold several episodes; device == host with the critic's bootstrap for the cut."""
    from openkitchen_amd.rollout import batch_stats, collect_episode_device, prepare_batch

    N, T = 512, 700
    venv = make_venv(N, auto_reset=True, seed=9)
    actor, critic = ppo_networks(5)
    venv.enable_actor(actor, critic)
    ep = collect_episode_device(venv, max_steps=T)
    alive = ep["alive"].cpu().numpy()
    assert alive.shape == (T, N)
    before = np.maximum.accumulate(alive, axis=0)[:-2]                       # alive in some older row
    after = np.flip(np.maximum.accumulate(np.flip(alive, 0), axis=0), 0)[2:]   # alive in some newer row
    interior = (~alive[1:-1]) & before & after
    assert interior.any(), "no column has a dead row with live rows on both sides: the record would not test the boundary"
    last_value = torch.randn(N, device="cuda")
    batch = prepare_batch(venv, ep, gamma=0.99, lam=0.95, normalize=True, last_value=last_value)
    rec = episode_as_record(ep)
    want = gpu.batch_prepare_host(**rec, last_value=last_value.cpu().numpy(), gamma=0.99, lam=0.95, normalize=3)
    assert batch["count"] == want["M"] == int(alive.sum())
    for mine, theirs in (("states", "state"), ("actions", "action"), ("log_probs", "prob"), ("returns", "ret"), ("advantages", "adv"), ("index", "index")):
        assert np.array_equal(B.bits(batch[mine].cpu().numpy()), B.bits(want[theirs])), mine
    B.assert_same({"stats": batch_stats(batch)}, {"stats": want["stats"]})
    venv.close()


def test_validation_on_a_handle(gpu):
    dev = gpu.BatchedEnvironment.from_track(gpu.Track("Austin"), 8, ray_angles_deg=PPO_FAN)
    E = gpu.capi.OkenvError
    with pytest.raises(E) as e:
        dev.batch_count()
    assert e.value.code == -5
    with pytest.raises(E) as e:
        dev.batch_timing()
    assert e.value.code == -5
    reward, alive = torch.ones((4, 3), device="cuda"), torch.ones((4, 3), dtype=torch.uint8, device="cuda")
    ret = torch.zeros(12, device="cuda")
    torch.cuda.synchronize()
    for kwargs in (dict(num_steps=0), dict(num_agents=0), dict(gamma=float("nan")), dict(gamma=1.5), dict(lam=-0.1), dict(record_stride=2),
                   dict(field_stride=2), dict(normalize=8), dict(block_threads=100), dict(num_steps=1 << 16, num_agents=1 << 15)):
        args = dict(num_steps=4, num_agents=3, inputs={"reward": reward, "alive": alive}, outputs={"ret": ret})
        args.update(kwargs)
        with pytest.raises(E) as e:
            dev.batch_prepare(**args)
        assert e.value.code == -1, kwargs
    for inputs, outputs in (({"alive": alive}, {"ret": ret}), ({"reward": reward}, {"ret": ret}), ({"reward": reward, "alive": alive}, {"adv": ret}),
                            ({"reward": reward, "alive": alive}, {"state": ret}), ({"reward": reward, "alive": alive, "last_value": ret}, {})):
        with pytest.raises(E) as e:
            dev.batch_prepare(4, 3, inputs, outputs)
        assert e.value.code == -1
    dev.batch_prepare(4, 3, {"reward": reward, "alive": alive}, {"ret": ret})
    assert dev.batch_count() == 12
    with pytest.raises(E) as e:
        dev.batch_timing()  # that call ran untimed
    assert e.value.code == -5
    dev.set_timing(True)
    dev.batch_prepare(4, 3, {"reward": reward, "alive": alive}, {"ret": ret})
    times = dev.batch_timing()
    assert set(times) == set(gpu.capi.BATCH_KERNELS) and all(v > 0.0 for v in times.values())
    dev.set_timing(False)
    dev.close()


def test_example_runs_with_the_device_batch(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_racer.py"), "--device-actor", "--device-batch", "--agents", "256",
                        "--episodes", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [line for line in r.stdout.splitlines() if line.startswith("episode")]
    assert len(lines) == 2 and all("the batch" in line for line in lines), r.stdout
    lengths = [float(line.split("mean episode length")[1].split("(")[0]) for line in lines]
    assert all(np.isfinite(v) and v > 0 for v in lengths)
