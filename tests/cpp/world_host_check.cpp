// world_host_check.cpp -- the host forward and score of the world-model racers' rule (include/okenv_world.h) as a stand-alone program,
// built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_world_rule.py: the frame, both parameter vectors, the state and
// the work space of exactly ok_world_work_floats floats on the heap, so that a forward that reads or writes past any of them is reported.
// Arguments: "S c0 c1 c2 c3 Z h", any number of them.  Prints "ok <forwards run>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "okenv_world.h"

static uint32_t state = 12345u;

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
    for (int a = 1; a + 6 < argc; a += 7)
    {
        ok_world_shape s;
        s.S = std::atoi(argv[a]);
        for (int l = 0; l < 4; ++l)
            s.c[l] = std::atoi(argv[a + 1 + l]);
        s.Z = std::atoi(argv[a + 5]);
        s.h = std::atoi(argv[a + 6]);
        if (ok_world_shape_bad(s))
            return 2;
        std::vector<float> encoder(static_cast<size_t>(ok_world_offsets(s).total)), controller(static_cast<size_t>(ok_world_controller_params(s)));
        for (float &x : encoder)
            x = uniform(0.02f);
        for (float &x : controller)
            x = uniform(1.0f);
        std::vector<uint8_t> frame(static_cast<size_t>(s.S) * s.S * 4U);
        for (uint8_t &b : frame)
            b = static_cast<uint8_t>(next());
        std::vector<float> work(static_cast<size_t>(ok_world_work_floats(s))), x(static_cast<size_t>(s.Z) + 2U);
        float              y = NAN;
        ok_world_forward(s, encoder.data(), controller.data(), frame.data(), uniform(180.0f), work.data(), x.data(), &y);
        if (!std::isfinite(y) || std::fabs(y) > 1.0f || !std::isfinite(x[0]) || std::fabs(x[s.Z] * x[s.Z] + x[s.Z + 1] * x[s.Z + 1] - 1.0f) > 1e-5f)
            return 3;
        // the score on a centre line of exactly P points
        const int          P = 5 + runs;
        std::vector<float> cx(P), cy(P), wl(P), wr(P);
        for (int i = 0; i < P; ++i)
            cx[i] = static_cast<float>(i), cy[i] = uniform(1.0f), wl[i] = 2.0f, wr[i] = 3.0f;
        const float alive = ok_world_score(1.0f, 0, 0, cx.data(), cy.data(), wl.data(), wr.data(), P, static_cast<float>(P - 1), 0.0f);
        const float gone  = ok_world_score(1.0f, 1, 0, cx.data(), cy.data(), wl.data(), wr.data(), P, 0.0f, 0.0f);
        const float timed = ok_world_score(1.0f, 1, 1, cx.data(), cy.data(), wl.data(), wr.data(), P, 0.0f, 0.0f);
        if (!(alive > 1.5f && alive <= 2.0f) || gone != 1.0f || timed != 0.0f)
            return 4;
        ++runs;
    }
    std::printf("ok %d\n", runs);
    return (argc - 1) % 7 == 0 ? 0 : 2;
}
