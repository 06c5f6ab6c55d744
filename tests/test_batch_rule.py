"""The episode-to-batch rule (include/okenv_batch.h) on the CPU: okenv_batch_prepare_host against the
independent numpy restatement of tests/_batch_numpy.py bit for bit, against the parent's torch code, against the reference's
flat recurrence, and against float64 evaluations with bounds derived from the operations involved.

Margins seen (largest error / bound over all cases of the test; printed with -s): normalised values 0.44, mean 0.88, std 0.73
(test_statistics_against_float64; the bound on the mean is little more than the half unit of its rounding to fp32, so a ratio near 1
is what a mean just below a power of two gives), advantages 0.15 (test_advantage_against_float64)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _batch_numpy as B

STEPS, AGENTS = (1, 2, 7, 600, 3000), (1, 3, 64, 257, 4096)
OUTPUTS = ("state", "action", "prob", "ret", "adv", "index", "ret_plane", "adv_plane", "stats", "count")


def host(ok, rec, N, want=None, gamma=0.99, lam=1.0, normalize=0, use_value=True, use_last=True):
    return ok.batch_prepare_host(rec["reward"], rec["alive"], rec.get("value") if use_value else None,
                                 rec.get("last_value") if (use_value and use_last) else None, rec["state"], rec["action"], rec["prob"], num_agents=N,
                                 gamma=gamma, lam=lam, normalize=normalize, want=want)


def restated(rec, N, gamma=0.99, lam=1.0, normalize=0, use_value=True, use_last=True):
    return B.prepare(rec["reward"], rec["alive"], rec.get("value") if use_value else None, rec.get("last_value") if (use_value and use_last) else None,
                     rec["state"], rec["action"], rec["prob"], num_agents=N, gamma=gamma, lam=lam, normalize_ret=bool(normalize & 1),
                     normalize_adv=bool(normalize & 2))


@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("N", AGENTS)
def test_host_equals_restatement_every_size(ok, T, N):
    """Every size, both reward kinds, monotone and interior masks, with and without the value plane, padded strides."""
    for k, (mask, reward) in enumerate((("monotone", "step"), ("interior", "progress"))):
        rec = B.make_record(T, N, mask, reward, seed=1000 * T + N + k, pad=3 * k)
        for use_value, lam, normalize in ((False, 1.0, 1), (True, 0.95, 3)):
            got = host(ok, rec, N, lam=lam, normalize=normalize, use_value=use_value)
            want = restated(rec, N, lam=lam, normalize=normalize, use_value=use_value)
            assert got["M"] == want["M"] == int(got["count"][0])
            B.assert_same(got, want, (T, N, mask, use_value))
            assert ("adv" in got) == use_value


@pytest.mark.parametrize("T,N", [(1, 1), (2, 3), (7, 64), (7, 257), (600, 3), (600, 257)])
def test_host_equals_restatement_every_switch(ok, T, N):
    """The full cross of mask kind, reward kind, lambda, normalisation switch, bootstrap and padding at small and middle sizes."""
    seen = 0
    for mask, reward, pad in itertools.product(B.MASKS, B.REWARDS, (0, 5)):
        rec = B.make_record(T, N, mask, reward, seed=T * 31 + N + pad, pad=pad)
        for lam, normalize, use_last in itertools.product((0.0, 0.95, 1.0), (0, 1, 2, 3), (False, True)):
            got = host(ok, rec, N, lam=lam, normalize=normalize, use_last=use_last)
            B.assert_same(got, restated(rec, N, lam=lam, normalize=normalize, use_last=use_last), (mask, reward, pad, lam, normalize, use_last))
            seen += 1
        got = host(ok, rec, N, normalize=1, use_value=False)
        B.assert_same(got, restated(rec, N, normalize=1, use_value=False), (mask, reward, pad, "no value"))
    assert seen == len(B.MASKS) * 2 * 2 * 3 * 4 * 2


def test_each_output_may_be_null(ok):
    rec = B.make_record(37, 70, "interior", "progress", seed=5, pad=2)
    want = restated(rec, 70, lam=0.95, normalize=3)
    for leave_out in OUTPUTS:
        names = [k for k in OUTPUTS if k != leave_out]
        got = host(ok, rec, 70, want=names, lam=0.95, normalize=3)
        assert leave_out not in got and set(names) <= set(got)
        B.assert_same(got, want, leave_out)
    got = host(ok, rec, 70, want=[], lam=0.95, normalize=3)  # nothing but the out-parameter
    assert got == {"M": want["M"]}


def test_edge_masks(ok):
    """M = 0 and M = 1 give neither NaN nor inf: mean 0 / the sample, std 0, the normalised sample 0."""
    for T, N in ((1, 1), (7, 3), (50, 257)):
        rec = B.make_record(T, N, "all_dead", "progress", seed=3)
        got = host(ok, rec, N, normalize=3)
        assert got["M"] == 0 and got["ret"].size == 0 and got["index"].size == 0 and got["state"].shape == (0, 5)
        assert not got["ret_plane"].any() and not got["adv_plane"].any()
        assert got["stats"] == {"sum_ret": 0.0, "sumsq_ret": 0.0, "sum_adv": 0.0, "sumsq_adv": 0.0, "mean_ret": 0.0, "std_ret": 0.0, "mean_adv": 0.0,
                                "std_adv": 0.0, "count": 0}
        rec = B.make_record(T, N, "one_sample", "progress", seed=4)
        got = host(ok, rec, N, normalize=3)
        raw = host(ok, rec, N, normalize=0)
        assert got["M"] == 1 and got["stats"]["std_ret"] == 0.0 and got["stats"]["std_adv"] == 0.0
        assert got["stats"]["mean_ret"] == raw["ret"][0] and got["stats"]["mean_adv"] == raw["adv"][0]
        assert got["ret"][0] == 0.0 and got["adv"][0] == 0.0
        t, i = divmod(int(got["index"][0]), N)
        assert rec["alive"][t, i] and raw["ret"][0] == rec["reward"][t, i]
        rec = B.make_record(T, N, "one_to_last", "step", seed=6)
        got = host(ok, rec, N, normalize=0)
        assert got["M"] == T and np.all(np.isfinite(got["ret"])) and got["ret"][-1] == 1.0


@pytest.mark.parametrize("T,N", [(1, 1), (7, 3), (700, 300), (3000, 64)])
def test_against_the_parent_torch_path(ok, T, N):
    """Monotone masks: the unnormalised return plane is discounted_returns(rewards * alive, normalize=False) of
    openkitchen_amd/rollout.py bit for bit; the dense fields are the parent's boolean-mask selections; `index` reproduces them."""
    import torch
    from openkitchen_amd.rollout import discounted_returns

    for reward in B.REWARDS:
        rec = B.make_record(T, N, "monotone", reward, seed=T + N)
        got = host(ok, rec, N, normalize=0, use_value=False)
        alive = torch.from_numpy(rec["alive"].astype(bool))
        parent = discounted_returns(torch.from_numpy(rec["reward"]) * alive, normalize=False)
        assert np.array_equal(B.bits(got["ret_plane"]), B.bits(parent.numpy()))
        mask = alive.reshape(-1)
        for name, width in (("state", 5), ("action", 1), ("prob", 1)):
            sel = torch.from_numpy(rec[name]).reshape(-1, width)[mask]
            assert np.array_equal(B.bits(got[name].reshape(-1, width)), B.bits(sel.numpy())), name
            again = torch.from_numpy(rec[name]).reshape(-1, width).index_select(0, torch.from_numpy(got["index"]).long())
            assert torch.equal(again, sel), name
        assert np.array_equal(B.bits(got["ret"]), B.bits(parent.reshape(-1)[mask].numpy()))


def test_single_agent_is_the_flat_recurrence(ok):
    """N = 1: ExperienceBuffer::calculateDiscountedRewards (RLRacers/PPO/ExperienceBuffer.hpp:52-62) as a plain float32 loop."""
    rng = np.random.default_rng(11)
    for T in (1, 2, 7, 600, 3000):
        rewards = (rng.standard_normal(T) * 0.37).astype(np.float32)
        got = ok.batch_prepare_host(rewards.reshape(T, 1), np.ones((T, 1), np.uint8), gamma=0.99, normalize=0)
        out, cumulative, gamma = np.zeros(T, np.float32), np.float32(0.0), np.float32(0.99)
        for k in range(T - 1, -1, -1):
            cumulative = np.float32(rewards[k] + np.float32(gamma * cumulative))
            out[k] = cumulative
        assert np.array_equal(B.bits(got["ret"]), B.bits(out)) and np.array_equal(got["index"], np.arange(T, dtype=np.int32))


def test_statistics_against_float64(ok):
    """Mean, unbiased std and the normalised returns / advantages against torch in float64 (two-pass) over the same samples, within
    the bound B.normalized_bound derives from the rule's operations; no case excused."""
    import torch

    worst = {"normalized": 0.0, "mean": 0.0, "std": 0.0}
    for (T, N), mask, reward in itertools.product(((7, 3), (600, 257), (3000, 64), (700, 4096)), ("monotone", "interior", "one_to_last"), B.REWARDS):
        rec = B.make_record(T, N, mask, reward, seed=T + 7 * N)
        raw, got = host(ok, rec, N, lam=0.95, normalize=0), host(ok, rec, N, lam=0.95, normalize=3)
        for q in ("ret", "adv"):
            x = torch.from_numpy(raw[q]).double()
            M = x.numel()
            if M < 2:
                continue
            mean64, std64 = float(x.mean()), float(x.std())
            ref = ((x - mean64) / (std64 + float(B.EPS))).numpy()
            bound, e_mean, e_std = B.normalized_bound(raw[q], M, mean64, std64, float(x.abs().sum()), float((x * x).sum()))
            err = np.abs(got[q].astype(np.float64) - ref)
            worst["normalized"] = max(worst["normalized"], float((err / bound).max()))
            worst["mean"] = max(worst["mean"], abs(float(got["stats"]["mean_" + q]) - mean64) / e_mean)
            worst["std"] = max(worst["std"], abs(float(got["stats"]["std_" + q]) - std64) / e_std)
            assert np.all(err <= bound), (T, N, mask, reward, q, float((err / bound).max()))
            assert abs(float(got["stats"]["mean_" + q]) - mean64) <= e_mean and abs(float(got["stats"]["std_" + q]) - std64) <= e_std
            assert got["stats"]["count"] == M
    print("largest error / bound: %s" % worst)
    assert worst["normalized"] > 0.0


def advantage_float64(rec, N, gamma, lam, use_last):
    T = rec["reward"].shape[0]
    g, gl = float(np.float32(gamma)), float(np.float32(np.float64(np.float32(gamma)) * np.float64(np.float32(lam))))
    r, v, al = rec["reward"][:, :N].astype(np.float64), rec["value"][:, :N].astype(np.float64), rec["alive"][:, :N] != 0
    a, v_next = np.zeros(N), (rec["last_value"].astype(np.float64) if use_last else np.zeros(N))
    A, scale = np.zeros((T, N)), 0.0
    for t in range(T - 1, -1, -1):
        delta = (r[t] + g * v_next) - v[t]
        a = np.where(al[t], delta + gl * a, 0.0)
        scale = max(scale, float(np.where(al[t], np.abs(r[t]) + np.abs(v_next) + np.abs(v[t]) + np.abs(a), 0.0).max()))
        v_next = np.where(al[t], v[t], 0.0)
        A[t] = a
    return A, scale, gl


def test_advantage_against_float64(ok):
    """The advantage plane against the same recurrence in float64.  A row rounds five times (gamma * v_next, the target, delta,
    gl * A_next, the sum), each by at most 2^-24 of a magnitude below `scale` = max(|r| + |v_next| + |value| + |A|); an error made in
    one row reaches the older rows multiplied by gl per row, so the total stays below 5 * 2^-24 * scale * min(T, 1 / (1 - gl))."""
    worst = 0.0
    for (T, N), mask, lam, use_last in itertools.product(((7, 3), (600, 257), (3000, 64)), ("monotone", "interior"), (0.0, 0.95, 1.0), (False, True)):
        rec = B.make_record(T, N, mask, "progress", seed=T + N)
        got = host(ok, rec, N, gamma=0.99, lam=lam, normalize=0, use_last=use_last)
        ref, scale, gl = advantage_float64(rec, N, 0.99, lam, use_last)
        bound = 5.0 * 2.0 ** -24 * scale * (min(T, 1.0 / (1.0 - gl)) if gl < 1.0 else T)
        err = float(np.abs(got["adv_plane"].astype(np.float64) - ref).max())
        worst = max(worst, err / bound)
        assert err <= bound, (T, N, mask, lam, use_last, err, bound)
    print("largest advantage error / bound: %.3f" % worst)


def test_lambda_zero_is_delta(ok):
    for mask in ("monotone", "interior"):
        rec = B.make_record(600, 257, mask, "progress", seed=9)
        got = host(ok, rec, 257, gamma=0.99, lam=0.0, normalize=0)
        al = rec["alive"][:, :257] != 0
        v = rec["value"][:, :257]
        v_next = np.zeros_like(v)
        v_next[:-1] = np.where(al[1:], v[1:], np.float32(0.0))
        v_next[-1] = rec["last_value"]
        delta = (rec["reward"][:, :257] + np.float32(0.99) * v_next) - v
        assert np.array_equal(B.bits(got["adv_plane"]), B.bits(np.where(al, delta, np.float32(0.0)).astype(np.float32)))


def test_validation(ok):
    L, cap = ok.capi.load(), ok.capi
    T, N = 4, 3
    rec = B.make_record(T, N, "monotone", "step", seed=1)
    keep = {k: np.ascontiguousarray(v) for k, v in rec.items()}
    outs = {"state": np.zeros((T * N, 5), np.float32), "action": np.zeros(T * N, np.int64), "prob": np.zeros(T * N, np.float32),
            "ret": np.zeros(T * N, np.float32), "adv": np.zeros(T * N, np.float32), "adv_plane": np.zeros((T, N), np.float32)}

    def call(params=None, drop_in=(), only_out=("ret",), null=()):
        bp = cap.OkenvBatchParams(**dict(dict(num_steps=T, num_agents=N, state_width=5, gamma=0.99, lam=0.95), **(params or {})))
        bi, bo = cap.OkenvBatchInput(), cap.OkenvBatchOutput()
        for k, v in keep.items():
            if k not in drop_in:
                setattr(bi, k, v.ctypes.data)
        for k in only_out:
            setattr(bo, k, outs[k].ctypes.data)
        args = [None if "params" in null else C.byref(bp), None if "in" in null else C.byref(bi), None if "out" in null else C.byref(bo)]
        return L.okenv_batch_prepare_host(*args, None)

    assert call() == 0
    for null in ("params", "in", "out"):
        assert call(null=(null,)) == -1
    assert b"NULL" in L.okenv_last_error(None)
    assert call(drop_in=("reward",)) == -1 and call(drop_in=("alive",)) == -1
    assert call({"num_steps": 0}) == -1 and call({"num_agents": 0}) == -1 and call({"num_steps": -3}) == -1
    assert call({"num_steps": 1 << 16, "num_agents": 1 << 15}) == -1  # T * N = 2^31
    assert b"2^31" in L.okenv_last_error(None)
    for bad in (float("nan"), -0.01, 1.01, float("inf")):
        assert call({"gamma": bad}) == -1 and call({"lam": bad}) == -1
    assert call({"gamma": 0.0, "lam": 1.0}) == 0 and call({"gamma": 1.0, "lam": 0.0}) == 0
    assert call({"record_stride": N - 1}) == -1 and call({"field_stride": N - 1}) == -1
    assert b"stride" in L.okenv_last_error(None)
    assert call({"normalize": 4}) == -1 and call({"block_threads": 96}) == -1 and call({"block_threads": 256}) == 0
    assert call(drop_in=("value", "last_value"), only_out=("adv",)) == -1 and call(drop_in=("value", "last_value"), only_out=("adv_plane",)) == -1
    assert call(drop_in=("value",)) == -1  # last_value without value
    for name in ("state", "action", "prob"):
        assert call(drop_in=(name,), only_out=(name,)) == -1
    assert call({"state_width": 0}, only_out=("state",)) == -1
    # the handle entry points: a NULL handle is invalid
    assert L.okenv_batch_prepare(None, None, None, None) == -1
    assert L.okenv_batch_count(None, None) == -1
    assert L.okenv_debug_batch_timing(None, None) == -1
