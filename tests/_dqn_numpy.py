"""The rule of Deep-Q learning (include/okenv_dqn.h) read again in numpy, written from the header's prose and not from its code: the
replay ring's push transition by transition, Philox4x32-10 and the multiply-shift index in Python integers, the target, the seed, the
scale 2 / (B A) and the loss.  The forward pass, the backward terms, the rule's sums and Adam are tests/_learn_numpy.py's (the
restatement of okenv_learn.h, which this rule is built on).  Every fp32 operation is one numpy float32 operation."""
import numpy as np

import _learn_numpy as L_

f32 = np.float32
M32 = 0xFFFFFFFF


def philox4x32(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers: counter c[4], key k[2] -> four 32-bit words."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def sample(seed, draw, size, B):
    """Slots of positions 0 .. B-1 of draw number `draw`: stream 7, key (seed, "oken")."""
    return np.array([(philox4x32((q, draw & M32, 7, 0), (seed & M32, 0x6F6B656E))[0] * size) >> 32 for q in range(B)], dtype=np.int64)


def ring(capacity, R):
    return {"state": np.zeros((capacity, R), f32), "next_state": np.zeros((capacity, R), f32), "action": np.zeros(capacity, np.int64),
            "reward": np.zeros(capacity, f32), "done": np.zeros(capacity, f32), "pushed": 0}


def push(rg, state, action, alive, dist, crashed, reward=None, push_all=False):
    """One push, literally one transition after the other: a later one overwrites an earlier one that shares its slot."""
    Cn = rg["state"].shape[0]
    for a in range(len(action)):
        if not (push_all or alive[a]):
            continue
        slot = rg["pushed"] % Cn
        rg["state"][slot] = state[a]
        rg["next_state"][slot] = dist[a].astype(f32) / f32(200.0)
        rg["action"][slot] = action[a]
        rg["done"][slot] = f32(1.0) if crashed[a] else f32(0.0)
        if reward is not None:
            rg["reward"][slot] = reward[a]
        elif crashed[a]:
            rg["reward"][slot] = f32(-200.0)
        else:
            m = f32(200.0)
            for d in dist[a]:
                if m > d:
                    m = d
            rg["reward"][slot] = m
        rg["pushed"] += 1
    return rg


def targets(q_next, reward, done, gamma, mask_done):
    """y [n] from q' [n, A]."""
    m = q_next[:, 0].copy()
    for k in range(1, q_next.shape[1]):
        m = np.where(q_next[:, k] > m, q_next[:, k], m)
    g = ((f32(1.0) - done) * f32(gamma)).astype(f32) if mask_done else np.full(len(reward), f32(gamma), dtype=f32)
    return (reward + (g * m).astype(f32)).astype(f32)


def update(hp, cfg, shape, state, rg, B, iterations=1, resample=False, draw_base=0, target=None, size=None):
    """The whole rule.  hp = dict(lr, beta1, beta2, eps); cfg = dict(gamma, mask_done, target_network, seed); state: policy,
    policy_m, policy_v, t.  Returns (new state, outputs: loss [iterations], grad_policy, index [B])."""
    R, H, A = shape
    st = {k: np.array(state[k], dtype=f32, copy=True) for k in ("policy", "policy_m", "policy_v")}
    t = int(state.get("t", 0))
    size = min(rg["pushed"], rg["state"].shape[0]) if size is None else size
    count = f32(B * A)
    out = {"loss": []}
    with np.errstate(all="ignore"):
        for it in range(iterations):
            draw = (draw_base + (it if resample else 0)) & M32
            if size > 0:
                idx = sample(cfg["seed"], draw, size, B)
                x, xn = rg["state"][idx].astype(f32), rg["next_state"][idx].astype(f32)
                r, d, a = rg["reward"][idx].astype(f32), rg["done"][idx].astype(f32), np.clip(rg["action"][idx], 0, A - 1)
            else:
                idx = np.zeros(B, np.int64)
                x, xn = np.zeros((B, R), f32), np.zeros((B, R), f32)
                r, d, a = np.zeros(B, f32), np.zeros(B, f32), np.zeros(B, np.int64)
            zn, _, _ = L_.forward(target if cfg["target_network"] else st["policy"], R, H, A, xn)
            y = targets(zn, r, d, cfg["gamma"], cfg["mask_done"])
            z, s, h = L_.forward(st["policy"], R, H, A, x)
            e = (z[np.arange(B), a] - y).astype(f32) if size > 0 else np.zeros(B, f32)
            dz = np.zeros((B, A), f32)
            dz[np.arange(B), a] = e
            total = L_.rule_sum(L_.backward_terms(st["policy"], R, H, A, x, s, h, dz))
            g = ((f32(2.0) * total).astype(f32) / count).astype(f32)
            out["loss"].append(L_.rule_sum((e * e).astype(f32)[:, None])[0] / count)
            out["grad_policy"], out["index"] = g, idx.astype(np.int32)
            t += 1
            st["policy"], st["policy_m"], st["policy_v"] = L_.adam(st["policy"], st["policy_m"], st["policy_v"], g, hp, t)
    st["t"] = t
    out["loss"] = np.array(out["loss"], dtype=f32)
    return st, out
