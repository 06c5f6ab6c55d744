// lidar_host_check.cpp -- the host forwards of the lidar and flow rules (include/okenv_lidar.h, okenv_flow.h) as a stand-alone program,
// built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_lidar_rule.py: the work space of exactly
// ok_lidar_work_floats / ok_flow_work_floats floats on the heap, so that a forward that needs more is reported.
// Arguments: "lidar R d ff h1 h2 nhead layers" or "flow C H S", any number of them.  Prints "ok <forwards run>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "okenv_flow.h"
#include "okenv_lidar.h"

static uint32_t state = 12345u;

static float draw(const float scale)
{
    state = state * 1664525u + 1013904223u;
    return (static_cast<float>(state >> 8) / 8388608.0f - 1.0f) * scale;
}

static std::vector<float> filled(const int n, const float scale)
{
    std::vector<float> v(static_cast<size_t>(n));
    for (float &x : v)
        x = draw(scale);
    return v;
}

int main(int argc, char **argv)
{
    int runs = 0;
    for (int a = 1; a < argc;)
    {
        float o[2] = {NAN, NAN};
        if (std::strcmp(argv[a], "lidar") == 0 && a + 7 < argc)
        {
            ok_lidar_shape s;
            s.R = std::atoi(argv[a + 1]), s.d = std::atoi(argv[a + 2]), s.ff = std::atoi(argv[a + 3]), s.h1 = std::atoi(argv[a + 4]);
            s.h2 = std::atoi(argv[a + 5]), s.nhead = std::atoi(argv[a + 6]), s.layers = std::atoi(argv[a + 7]);
            a += 8;
            if (ok_lidar_shape_bad(s))
                return 2;
            const std::vector<float> params = filled(ok_lidar_offsets(s).total, 0.1f), in = filled(2 * s.R, 1.0f);
            std::vector<float>       work(static_cast<size_t>(ok_lidar_work_floats(s)));
            ok_lidar_forward(s, params.data(), in.data(), work.data(), o);
        }
        else if (std::strcmp(argv[a], "flow") == 0 && a + 3 < argc)
        {
            ok_flow_shape s;
            s.C = std::atoi(argv[a + 1]), s.H = std::atoi(argv[a + 2]), s.S = std::atoi(argv[a + 3]);
            a += 4;
            if (ok_flow_shape_bad(s))
                return 2;
            const std::vector<float> params = filled(ok_flow_offsets(s).total, 0.05f), cond = filled(s.C, 1.0f), x0 = filled(2, 1.0f);
            std::vector<float>       work(static_cast<size_t>(ok_flow_work_floats(s)));
            ok_flow_forward(s, params.data(), cond.data(), x0.data(), work.data(), o);
        }
        else
            return 2;
        if (!std::isfinite(o[0]) || !std::isfinite(o[1]))
            return 3;
        ++runs;
    }
    std::printf("ok %d\n", runs);
    return 0;
}
