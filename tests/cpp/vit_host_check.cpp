// vit_host_check.cpp -- the host forward of the image transformer's rule (include/okenv_vit.h) as a stand-alone program, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_vit_rule.py: the parameters, the frame and the work space of exactly
// ok_vit_offsets(s).total / S S 4 / ok_vit_work_floats(s) elements on the heap, so that a forward that reads or writes past one of them
// is reported.  Arguments: "S P D heads depth ff h1 h2", any number of them.  Prints "ok <forwards run>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "okenv_vit.h"

static uint32_t state = 12345u;

static uint32_t next()
{
    state = state * 1664525u + 1013904223u;
    return state;
}

int main(int argc, char **argv)
{
    int runs = 0;
    for (int a = 1; a + 7 < argc; a += 8)
    {
        ok_vit_shape s;
        s.S = std::atoi(argv[a]), s.P = std::atoi(argv[a + 1]), s.D = std::atoi(argv[a + 2]), s.heads = std::atoi(argv[a + 3]);
        s.depth = std::atoi(argv[a + 4]), s.ff = std::atoi(argv[a + 5]), s.h1 = std::atoi(argv[a + 6]), s.h2 = std::atoi(argv[a + 7]);
        if (ok_vit_shape_bad(s))
            return 2;
        const ok_vit_consts  k = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}, 1e-6f, 100.0f, 10.0f};
        std::vector<float>   params(static_cast<size_t>(ok_vit_offsets(s).total));
        for (float &x : params)
            x = (static_cast<float>(next() >> 8) / 8388608.0f - 1.0f) * 0.1f;
        std::vector<uint8_t> frame(static_cast<size_t>(s.S) * s.S * 4);
        for (uint8_t &b : frame)
            b = static_cast<uint8_t>(next() >> 24);
        std::vector<float> work(ok_vit_work_floats(s)), emb(static_cast<size_t>(s.D));
        float              o = NAN;
        ok_vit_forward(s, k, params.data(), frame.data(), work.data(), emb.data(), &o);
        if (!std::isfinite(o) || !std::isfinite(emb[0]) || !std::isfinite(ok_vit_steer(o, k.steer_scale)))
            return 3;
        ++runs;
    }
    std::printf("ok %d\n", runs);
    return 0;
}
