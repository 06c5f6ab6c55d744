"""Development aid (CPU only): how often the step kernels repeat the origin test on the bench recipe's poses.

usage: python tests/tools/cert_rerun_rate.py [track] [cell] [agents] [steps]
The oracle drives the bench recipe one step at a time; tests/cpp/origin_clearance_check.cpp applies the step loop's rule to every
agent's origins with the product's own okOriginClearScalar: the test runs again when the origin has left the square the last test
cleared (okOriginMoved, what the kernels do) -- and, for comparison, when it has left the diamond |dx| + |dy| < half-width inside
that square (what they did before).  Crashed agents do not cast and are not counted.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle as O  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "Silverstone"
    cell = float(sys.argv[2]) if len(sys.argv) > 2 else 28.0
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 300
    O.build_oracle(with_ref=False)
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libclearcheck.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "cpp", "origin_clearance_check.cpp")], check=True)
    G = C.CDLL(so)
    i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    G.clearcheck_reruns.argtypes = [O.f32p, C.c_int, C.c_float, O.f32p, O.f32p, C.c_int, C.c_int, i64p]
    t = O.Track(name)
    R = 64
    env = O.OracleEnv(t.segments, N, R, O.default_ray_fan(R), (t.x, t.y, t.heading))
    env.init_bench_state(0, 0)
    ox, oy = np.full((steps, N), np.nan, np.float32), np.full((steps, N), np.nan, np.float32)
    for s in range(steps):
        # the origin a step casts from is the pose after the step's move (the sensor offset is 0 in the bench recipe); an agent
        # found crashed before the step does not cast in it
        alive = env.snapshot()["crashed"] == 0
        env.rollout_random(1, 1234, 0, s, threads=8)
        sn = env.snapshot()
        ox[s, alive], oy[s, alive] = sn["pos_x"][alive], sn["pos_y"][alive]
    counts = np.zeros(3, np.int64)
    rc = G.clearcheck_reruns(np.ascontiguousarray(t.segments.reshape(-1)), t.S, cell, ox.reshape(-1), oy.reshape(-1), N, steps, counts)
    assert rc == 0, rc
    print("%s, cell %.0f px, %d agents x %d steps: %d casting agent-steps; origin test runs %d times (%.3f per agent-step) with the "
          "square, %d (%.3f) with the diamond" % (name, cell, N, steps, counts[2], counts[0], counts[0] / counts[2], counts[1], counts[1] / counts[2]))


if __name__ == "__main__":
    main()
