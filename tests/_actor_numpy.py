"""The shared-network actors' rule (include/okenv_math.h, "RLRacers: the shared-network actors") read again in numpy float32, written
from the header's prose and not from its code.  It shares with the library only ok_expf (through okenv_debug_expf); Philox4x32-10
and the 24-bit uniform are restated here from their definitions.  Every fp32 operation is one numpy float32 operation, so the bits
are those of separate IEEE multiplications and additions."""
import numpy as np

f32 = np.float32
SAMPLE, GREEDY, EPS_GREEDY = 0, 1, 2


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def u01(word):
    return (word >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)


def split(params, R, H, A):
    params = np.asarray(params, dtype=f32)
    w1 = params[:H * R].reshape(H, R)
    b1 = params[H * R:H * R + H]
    w2 = params[H * R + H:H * R + H + A * H].reshape(A, H)
    b2 = params[H * R + H + A * H:]
    assert b2.size == A
    return w1, b1, w2, b2


def forward(params, R, H, A, x):
    """x [n, R] float32 -> the A outputs [n, A]: the hidden sums in ascending input order from the bias, eight interleaved partial
    sums per output joined by the fixed tree, the bias first in the last addition."""
    w1, b1, w2, b2 = split(params, R, H, A)
    n = x.shape[0]
    h = np.empty((n, H), dtype=f32)
    for j in range(H):
        s = np.full(n, b1[j], dtype=f32)
        for i in range(R):
            s = s + w1[j, i] * x[:, i]
        h[:, j] = np.where(s > 0, s, f32(0))
    z = np.empty((n, A), dtype=f32)
    for k in range(A):
        part = [np.zeros(n, dtype=f32) for _ in range(8)]
        for j in range(H):
            part[j % 8] = part[j % 8] + w2[k, j] * h[:, j]
        tree = ((part[0] + part[4]) + (part[2] + part[6])) + ((part[1] + part[5]) + (part[3] + part[7]))
        z[:, k] = b2[k] + tree
    return z


def softmax_clamped(z, expf):
    """(unclamped p, clamped p): the maximum, ok_expf of the differences, the ascending sum, one division each, the clamp."""
    m = z.max(axis=1, keepdims=True)
    e = expf((z - m).astype(f32)).reshape(z.shape)
    s = e[:, 0].copy()
    for k in range(1, z.shape[1]):
        s = s + e[:, k]
    p = (e / s[:, None]).astype(f32)
    return p, np.minimum(np.maximum(p, f32(1e-8)), f32(1.0))


def act(expf, mode, epsilon, seed, agent_base, table, policy, value, R, H, A, Hv, dist, draw_index):
    """The whole rule for n agents; returns dict(action, prob, value, throttle, steer, state, p) with p the unclamped softmax."""
    with np.errstate(all="ignore"):
        dist = np.asarray(dist, dtype=f32)
        n = dist.shape[0]
        x = dist / f32(200.0)
        z = forward(policy, R, H, A, x)
        out = {"state": x}
        if Hv > 0:
            out["value"] = forward(value, R, Hv, 1, x)[:, 0]
        agents = (np.arange(n, dtype=np.uint64) + np.uint64(agent_base)) & np.uint64(0xFFFFFFFF)
        w = philox4x32(agents, np.uint32(draw_index), 6, 0, seed, 0x6F6B656E)
        best = np.zeros(n, dtype=np.int64)  # lowest index wins ties, NaN never wins
        top = z[:, 0].copy()
        for k in range(1, A):
            better = z[:, k] > top
            best[better] = k
            top[better] = z[better, k]
        rows = np.arange(n)
        if mode == EPS_GREEDY:
            explore = u01(w[0]) < f32(epsilon)
            uniform = ((w[1].astype(np.uint64) * np.uint64(A)) >> np.uint64(32)).astype(np.int64)
            action = np.where(explore, uniform, best)
            prob = z[rows, action]
        else:
            p, pc = softmax_clamped(z, expf)
            out["p"] = p
            if mode == GREEDY:
                action = best
            else:
                u = u01(w[0])
                action = np.full(n, A - 1, dtype=np.int64)
                found = np.zeros(n, dtype=bool)
                cum = pc[:, 0].copy()
                for k in range(A):
                    if k > 0:
                        cum = cum + pc[:, k]
                    hit = ~found & (u < cum)
                    action[hit] = k
                    found |= hit
            prob = pc[rows, action]
        table = np.asarray(table, dtype=f32)
        out.update(action=action, prob=prob.astype(f32), throttle=table[action, 0], steer=table[action, 1])
        return out
