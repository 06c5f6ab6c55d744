// qcnn_host_check.cpp -- the host side of the Deep-Q image racers' rule (include/okenv_qcnn.h) as a stand-alone program, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_qcnn_rule.py: the frames, the parameters, the work space of exactly
// ok_qcnn_work_floats floats, the ring of exactly `capacity` slots and the batch of exactly B rows on the heap, so that a forward, a
// push or a batch that reads or writes past any of them is reported.
// Arguments: "S k0 k1 k2 s0 s1 s2 p0 p1 p2 c0 c1 c2 H A", any number of them.  Prints "ok <shapes run>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "okenv_qcnn.h"

static uint32_t state = 12345u;

static uint32_t next()
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

int main(int argc, char **argv)
{
    int runs = 0;
    for (int a = 1; a + 14 < argc; a += 15)
    {
        ok_qcnn_shape s;
        s.S = std::atoi(argv[a]);
        for (int l = 0; l < 3; ++l)
            s.k[l] = std::atoi(argv[a + 1 + l]), s.s[l] = std::atoi(argv[a + 4 + l]), s.p[l] = std::atoi(argv[a + 7 + l]), s.c[l] = std::atoi(argv[a + 10 + l]);
        s.H = std::atoi(argv[a + 13]);
        s.A = std::atoi(argv[a + 14]);
        if (ok_qcnn_shape_bad(s))
            return 2;
        std::vector<float> params(static_cast<size_t>(ok_qcnn_offsets(s).total));
        for (float &x : params)
            x = (static_cast<float>(next()) / 8388608.0f - 1.0f) * 0.02f;
        const int    n  = 5;
        const size_t px = static_cast<size_t>(s.S) * s.S;
        std::vector<uint8_t> frames(n * px * 4U), next_frames(n * px * 4U);
        for (uint8_t &b : frames)
            b = static_cast<uint8_t>(next());
        for (uint8_t &b : next_frames)
            b = static_cast<uint8_t>(next());
        std::vector<float>   work(static_cast<size_t>(ok_qcnn_work_floats(s)));
        std::vector<int64_t> action(n);
        for (int i = 0; i < n; ++i)
        {
            std::vector<float> q(static_cast<size_t>(s.A), NAN);
            ok_qcnn_forward(s, params.data(), frames.data() + i * px * 4U, work.data(), q.data());
            for (const float v : q)
                if (!std::isfinite(v))
                    return 3;
            action[i] = ok_qcnn_choose(OK_ACTOR_EPS_GREEDY, 0.5f, 7u, static_cast<uint32_t>(i), static_cast<uint32_t>(runs), q.data(), s.A);
            if (action[i] < 0 || action[i] >= s.A)
                return 4;
        }
        // a ring smaller than one push, pushed into three times (it wraps), then read back in both modes with batches larger than it
        const uint64_t       capacity = 3;
        std::vector<float>   st(capacity * px), nx(capacity * px), rw(capacity), dn(capacity), dist(static_cast<size_t>(n) * 2U, 50.0f);
        std::vector<int64_t> ac(capacity);
        const ok_qcnn_ring   ring{st.data(), nx.data(), ac.data(), rw.data(), dn.data()};
        const uint8_t        alive[n] = {1, 0, 1, 1, 1}, crashed[n] = {0, 1, 0, 1, 0};
        uint64_t             pushed = 0;
        const int            B = 7;
        std::vector<float>   bs(B * px), bn(B * px), br(B), bd(B);
        std::vector<int64_t> ba(B);
        std::vector<int32_t> bi(B);
        const ok_qcnn_batch_out out{bs.data(), bn.data(), ba.data(), br.data(), bd.data(), bi.data()};
        ok_qcnn_batch(ring, capacity, s.S, pushed, 1u, B, OK_QCNN_BATCH_SEQUENTIAL, 0u, out); // the empty ring
        for (int round = 0; round < 3; ++round)
        {
            ok_qcnn_push(ring, capacity, s.S, &pushed, round == 1 ? OK_REPLAY_PUSH_ALL : 0u, n, action.data(), round == 1 ? nullptr : alive, frames.data(),
                         next_frames.data(), crashed, nullptr, dist.data(), 2);
            ok_qcnn_batch(ring, capacity, s.S, pushed, 1u, B, OK_QCNN_BATCH_SEQUENTIAL, static_cast<uint64_t>(round) * 5u, out);
            ok_qcnn_batch(ring, capacity, s.S, pushed, 1u, B, OK_QCNN_BATCH_UNIFORM, static_cast<uint64_t>(round), out);
            for (int q = 0; q < B; ++q)
                if (bi[q] < 0 || bi[q] >= static_cast<int32_t>(capacity) || !std::isfinite(bs[q * px]) || !std::isfinite(bn[q * px + px - 1]))
                    return 5;
        }
        if (pushed != 4 + 5 + 4)
            return 6;
        ++runs;
    }
    std::printf("ok %d\n", runs);
    return (argc - 1) % 15 == 0 ? 0 : 2;
}
