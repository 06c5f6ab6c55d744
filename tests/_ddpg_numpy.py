"""The rule of DDPG (include/okenv_ddpg.h) read again in numpy float32, written from the header's prose and not from its code: the
action tanh * scale + bias, the exploration draw with Philox4x32-10 in Python integers, the ring's push transition by transition,
the target, the critic's step, the actor's step through the stepped critic with da summed in the join order, and the soft updates.
The forward pass, the backward terms, the rule's sums and Adam are tests/_learn_numpy.py's, Philox and the sampling index
tests/_dqn_numpy.py's.  It shares with the library only ok_tanhf, passed in as `tanhf` (the oracle's export of the same header
function).  Every fp32 operation is one numpy float32 operation."""
import numpy as np

import _dqn_numpy as D_
import _learn_numpy as L_

f32 = np.float32
M32 = 0xFFFFFFFF
VECTORS = ("actor", "critic", "actor_target", "critic_target", "actor_m", "actor_v", "critic_m", "critic_v")


def n_actor(R, H):
    return L_.n_params(R, H, 2)


def n_critic(R, Hc):
    return L_.n_params(R + 2, Hc, 1)


def sample(seed, draw, size, B):
    """Slots of positions 0 .. B-1: section 17's sampling with DDPG's own seed."""
    return D_.sample(seed, draw, size, B)


def action(z, scale, bias, tanhf):
    """z [n, 2] -> (a [n, 2], t [n, 2]): one multiplication and one addition per component."""
    t = tanhf(z.astype(f32)).reshape(z.shape).astype(f32)
    scale, bias = np.asarray(scale, f32), np.asarray(bias, f32)
    return ((t * scale[None, :]).astype(f32) + bias[None, :]).astype(f32), t


def act(cfg, actor, R, dist, draw_index, tanhf):
    """cfg: dict(hidden, scale, bias, noise, seed, agent_base).  -> (action [n, 2], state [n, R])."""
    x = (np.asarray(dist, f32) / f32(200.0)).astype(f32)
    z, _, _ = L_.forward(actor, R, cfg["hidden"], 2, x)
    a, _ = action(z, cfg["scale"], cfg["bias"], tanhf)
    noise = np.asarray(cfg.get("noise", (0, 0)), f32)
    for k in range(2):
        if not noise[k] > 0:
            continue  # untouched: no addition, no clamp
        s, b = f32(cfg["scale"][k]), f32(cfg["bias"][k])
        lo, hi = f32(b - s), f32(b + s)
        for i in range(x.shape[0]):
            w = D_.philox4x32(((cfg.get("agent_base", 0) + i) & M32, draw_index & M32, 8, 0), (cfg.get("seed", 0) & M32, 0x6F6B656E))[k]
            u = f32(w >> 8) * f32(2.0 ** -24)
            v = f32(a[i, k] + f32(noise[k] * f32(f32(f32(2.0) * u) - f32(1.0))))
            a[i, k] = lo if v < lo else (hi if v > hi else v)
    return a, x


def ring(capacity, R):
    return {"state": np.zeros((capacity, R), f32), "next_state": np.zeros((capacity, R), f32), "action": np.zeros((capacity, 2), f32),
            "reward": np.zeros(capacity, f32), "done": np.zeros(capacity, f32), "pushed": 0}


def push(rg, state, act_, alive, dist, crashed, reward=None, push_all=False):
    """One push, literally one transition after the other: a later one overwrites an earlier one that shares its slot."""
    Cn = rg["state"].shape[0]
    for a in range(len(act_)):
        if not (push_all or alive[a]):
            continue
        slot = rg["pushed"] % Cn
        rg["state"][slot] = state[a]
        rg["next_state"][slot] = dist[a].astype(f32) / f32(200.0)
        rg["action"][slot] = act_[a]
        rg["done"][slot] = f32(1.0) if crashed[a] else f32(0.0)
        rg["reward"][slot] = reward[a] if reward is not None else f32(1.0)
        rg["pushed"] += 1
    return rg


def join8(terms):
    """[n, Hc] per-unit terms -> [n]: unit j into partial j mod 8 ascending from +0.0, the eight joined by the fixed tree."""
    n, Hc = terms.shape
    Hp = (Hc + 7) // 8 * 8
    padded = np.zeros((n, Hp), f32)
    padded[:, :Hc] = terms
    part = np.zeros((n, 8), f32)
    for t in range(Hp // 8):
        part = part + padded[:, 8 * t:8 * t + 8]
    return ((part[:, 0] + part[:, 4]) + (part[:, 2] + part[:, 6])) + ((part[:, 1] + part[:, 5]) + (part[:, 3] + part[:, 7]))


def soft(p, target, tau):
    tau = f32(tau)
    omt = f32(f32(1.0) - tau)
    return ((tau * p).astype(f32) + (omt * target).astype(f32)).astype(f32)


def update(cfg, R, state, rg, B, tanhf, iterations=1, resample=False, draw_base=0, size=None, stale_critic=False):
    """The whole rule.  cfg: dict(hidden, critic_hidden, scale, bias, gamma, tau, lr_actor, lr_critic, beta1, beta2, eps, sample_seed);
    state: the eight vectors and t.  stale_critic: the WRONG rule whose actor step reads the critic from before its step (a test shows
    that the two differ).  Returns (new state, outputs)."""
    H, Hc = cfg["hidden"], cfg["critic_hidden"]
    st = {k: np.array(state[k], dtype=f32, copy=True) for k in VECTORS}
    t = int(state.get("t", 0))
    size = min(rg["pushed"], rg["state"].shape[0]) if size is None else size
    count = f32(B)
    hp_a = dict(lr=cfg["lr_actor"], beta1=cfg["beta1"], beta2=cfg["beta2"], eps=cfg["eps"])
    hp_c = dict(hp_a, lr=cfg["lr_critic"])
    scale = np.asarray(cfg["scale"], f32)
    out = {"critic_loss": [], "actor_loss": []}
    with np.errstate(all="ignore"):
        for it in range(iterations):
            draw = (draw_base + (it if resample else 0)) & M32
            if size > 0:
                idx = sample(cfg["sample_seed"], draw, size, B)
                x, xn, a = rg["state"][idx].astype(f32), rg["next_state"][idx].astype(f32), rg["action"][idx].astype(f32)
                r, d = rg["reward"][idx].astype(f32), rg["done"][idx].astype(f32)
            else:
                idx = np.zeros(B, np.int64)
                x, xn, a = np.zeros((B, R), f32), np.zeros((B, R), f32), np.zeros((B, 2), f32)
                r, d = np.zeros(B, f32), np.zeros(B, f32)
            t += 1
            # 1: the target
            zn, _, _ = L_.forward(st["actor_target"], R, H, 2, xn)
            an, _ = action(zn, cfg["scale"], cfg["bias"], tanhf)
            qn, _, _ = L_.forward(st["critic_target"], R + 2, Hc, 1, np.concatenate([xn, an], axis=1))
            y = D_.targets(qn, r, d, cfg["gamma"], True)
            # 2: the critic
            xc = np.concatenate([x, a], axis=1)
            q, s, h = L_.forward(st["critic"], R + 2, Hc, 1, xc)
            e = (q[:, 0] - y).astype(f32) if size > 0 else np.zeros(B, f32)
            total = L_.rule_sum(L_.backward_terms(st["critic"], R + 2, Hc, 1, xc, s, h, e[:, None]))
            gc = ((f32(2.0) * total).astype(f32) / count).astype(f32)
            out["critic_loss"].append(L_.rule_sum((e * e).astype(f32)[:, None])[0] / count)
            before = st["critic"]
            st["critic"], st["critic_m"], st["critic_v"] = L_.adam(st["critic"], st["critic_m"], st["critic_v"], gc, hp_c, t)
            # 3: the actor, through the stepped critic
            critic = before if stale_critic else st["critic"]
            z, sa, ha = L_.forward(st["actor"], R, H, 2, x)
            act_, th = action(z, cfg["scale"], cfg["bias"], tanhf)
            q, s, _ = L_.forward(critic, R + 2, Hc, 1, np.concatenate([x, act_], axis=1))
            w1c, _, w2c, _ = L_.split(critic, R + 2, Hc, 1)
            seed = f32(1.0) if size > 0 else f32(0.0)
            dh = np.where(s > 0, (w2c[0][None, :] * seed).astype(f32), f32(0)).astype(f32)
            dz = np.zeros((B, 2), f32)
            for k in range(2):
                da = join8((w1c[None, :, R + k] * dh).astype(f32))
                dz[:, k] = ((da * scale[k]).astype(f32) * (f32(1.0) - (th[:, k] * th[:, k]).astype(f32)).astype(f32)).astype(f32)
            total = L_.rule_sum(L_.backward_terms(st["actor"], R, H, 2, x, sa, ha, dz))
            ga = ((-total).astype(f32) / count).astype(f32)
            qterm = q[:, 0].astype(f32) if size > 0 else np.zeros(B, f32)
            out["actor_loss"].append(-(L_.rule_sum(qterm[:, None])[0] / count))
            st["actor"], st["actor_m"], st["actor_v"] = L_.adam(st["actor"], st["actor_m"], st["actor_v"], ga, hp_a, t)
            # 4: the soft updates, after both steps
            st["critic_target"] = soft(st["critic"], st["critic_target"], cfg["tau"])
            st["actor_target"] = soft(st["actor"], st["actor_target"], cfg["tau"])
            out["grad_critic"], out["grad_actor"], out["index"] = gc, ga, idx.astype(np.int32)
    st["t"] = t
    out["critic_loss"] = np.array(out["critic_loss"], dtype=f32)
    out["actor_loss"] = np.array(out["actor_loss"], dtype=f32)
    return st, out
