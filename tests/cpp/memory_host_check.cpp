// memory_host_check.cpp -- the host forward of the world-model racers' memory (include/okenv_memory.h) as a stand-alone program, built
// with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_memory_rule.py: the frame, the three parameter vectors, the hidden
// state, the state, the prediction and the work spaces of exactly ok_memory_work_floats / ok_memory_step_floats floats on the heap, so
// that a forward or a step that reads or writes past any of them is reported.
// Arguments: "S c0 c1 c2 c3 Z H L h carry", any number of them.  Prints "ok <forwards run>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "okenv_memory.h"

static uint32_t state = 2463534242u;

static uint32_t next()
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

static float uniform(const float scale)
{
    return (static_cast<float>(next()) / 8388608.0f - 1.0f) * scale;
}

int main(int argc, char **argv)
{
    int runs = 0;
    for (int a = 1; a + 9 < argc; a += 10)
    {
        ok_world_shape w;
        w.S = std::atoi(argv[a]);
        for (int l = 0; l < 4; ++l)
            w.c[l] = std::atoi(argv[a + 1 + l]);
        w.Z = std::atoi(argv[a + 5]);
        w.h = 2;
        ok_memory_shape s;
        s.Z     = w.Z;
        s.H     = std::atoi(argv[a + 6]);
        s.L     = std::atoi(argv[a + 7]);
        s.h     = std::atoi(argv[a + 8]);
        s.carry = std::atoi(argv[a + 9]);
        if (ok_world_shape_bad(w) || ok_memory_shape_bad(s))
            return 2;
        const ok_memory_layout at = ok_memory_offsets(s);
        std::vector<float>     encoder(static_cast<size_t>(ok_world_offsets(w).total)), network(static_cast<size_t>(at.total)),
            controller(static_cast<size_t>(ok_memory_controller_params(s)));
        for (float &x : encoder)
            x = uniform(0.02f);
        for (float &x : network)
            x = uniform(1.0f / std::sqrt(static_cast<float>(s.H)));
        for (int j = 0; j < s.Z; ++j)
            network[at.z_std + j] = 0.5f + std::fabs(uniform(1.0f));
        network[at.a_std] = 20.0f, network[at.a_std + 1] = 2.5f;
        if (ok_memory_params_bad(s, network.data()))
            return 5;
        for (float &x : controller)
            x = uniform(2.0f / std::sqrt(static_cast<float>(s.Z + s.H)));
        std::vector<uint8_t> frame(static_cast<size_t>(w.S) * w.S * 4U);
        for (uint8_t &b : frame)
            b = static_cast<uint8_t>(next());
        std::vector<float> work(static_cast<size_t>(ok_memory_work_floats(w, s))), x(static_cast<size_t>(s.Z + s.H)), pred(static_cast<size_t>(s.Z)),
            hidden(static_cast<size_t>(s.L * s.H));
        for (float &v : hidden)
            v = uniform(0.9f);
        const std::vector<float> before = hidden;
        const float              action[2] = {100.0f, uniform(5.0f)};
        float                    y = NAN;
        ok_memory_forward(w, s, encoder.data(), network.data(), controller.data(), frame.data(), action, hidden.data(), work.data(), x.data(), pred.data(), &y);
        if (!std::isfinite(y) || std::fabs(y) > 1.0f || !std::isfinite(x[0]) || !std::isfinite(pred[s.Z - 1]))
            return 3;
        for (int j = 0; j < s.H; ++j)
            if (x[s.Z + j] != hidden[(s.L - 1) * s.H + j] || !(std::fabs(hidden[j]) < 1.0f))
                return 4;
        // the step alone, on a work space of exactly its own size and without a prediction: the same hidden state again
        std::vector<float> step_work(static_cast<size_t>(ok_memory_step_floats(s))), again = before, mu(x.begin(), x.begin() + s.Z);
        ok_memory_step(s, network.data(), mu.data(), action, again.data(), step_work.data(), nullptr);
        if (again != hidden)
            return 6;
        network[at.z_std + s.Z - 1] = 0.0f;
        if (!ok_memory_params_bad(s, network.data()))
            return 7;
        ++runs;
    }
    std::printf("ok %d\n", runs);
    return (argc - 1) % 10 == 0 ? 0 : 2;
}
