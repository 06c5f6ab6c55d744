// cnn_host_check.cpp -- the host forward of the image policy's rule (include/okenv_cnn.h) as a stand-alone program, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_cnn_rule.py: the frame, the parameters and the work space of exactly
// ok_cnn_work_floats floats on the heap, so that a forward that reads or writes past any of them is reported.
// Arguments: "S k0 k1 k2 s0 s1 s2 c0 c1 c2 H", any number of them.  Prints "ok <forwards run>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "okenv_cnn.h"

static uint32_t state = 12345u;

static uint32_t next()
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

int main(int argc, char **argv)
{
    int runs = 0;
    for (int a = 1; a + 10 < argc; a += 11)
    {
        ok_cnn_shape s;
        s.S = std::atoi(argv[a]);
        for (int l = 0; l < 3; ++l)
            s.k[l] = std::atoi(argv[a + 1 + l]), s.s[l] = std::atoi(argv[a + 4 + l]), s.c[l] = std::atoi(argv[a + 7 + l]);
        s.H = std::atoi(argv[a + 10]);
        if (ok_cnn_shape_bad(s))
            return 2;
        std::vector<float> params(static_cast<size_t>(ok_cnn_offsets(s).total));
        for (float &x : params)
            x = (static_cast<float>(next()) / 8388608.0f - 1.0f) * 0.02f;
        std::vector<uint8_t> frame(static_cast<size_t>(s.S) * s.S * 4U);
        for (uint8_t &b : frame)
            b = static_cast<uint8_t>(next());
        std::vector<float> work(static_cast<size_t>(ok_cnn_work_floats(s)));
        float              o = NAN, act[3];
        ok_cnn_forward(s, params.data(), frame.data(), work.data(), &o);
        ok_cnn_action(o, 100.0f, 10.0f, act);
        if (!std::isfinite(o) || !std::isfinite(act[0]) || act[1] != 100.0f)
            return 3;
        ++runs;
    }
    std::printf("ok %d\n", runs);
    return (argc - 1) % 11 == 0 ? 0 : 2;
}
