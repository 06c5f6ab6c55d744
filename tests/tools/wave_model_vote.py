"""Development aid: the lock-step model with the wave's vote that ends phase 1 (tests/tools/wave_model_vote.cpp).

usage: python tests/tools/wave_model_vote.py [agents] > profiles/r8_model.txt
For Silverstone, Monza and Spa and fans of 64, 32 and 16 rays (one, two and four agents per wave, each at its shipped cell edge),
on bench-recipe poses after 60 steps: phase 1 + phase 2 cell iterations / 8-slot point rounds / exact passes per wave-step on the
front image, for vote thresholds off and 8 ... 24 and phase-1 ranges of 48 px (32 for the 16-ray fans, as shipped), 64 px and none.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_model as WM  # noqa: E402

SO = WM.SO.replace("libwavemodel", "libwavemodel_vote")
SHAPES = {64: (28.0, 48.0), 32: (20.0, 48.0), 16: (24.0, 32.0)}  # fan -> shipped cell edge, shipped phase-1 range (okPlanLanes)
THRESHOLDS = (0, 8, 10, 12, 14, 16, 20, 24)


def build():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC"] + (WM.O.SAN_FLAGS if WM.O.SANITIZE else []) +
                   ["-I", os.path.join(WM.ROOT, "include"), "-I", os.path.join(WM.ROOT, "openkitchen_amd", "csrc"), "-o", SO, os.path.join(WM.ROOT, "tests", "tools", "wave_model_vote.cpp")], check=True)
    L = C.CDLL(SO)
    f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    L.wavemodel_vote.argtypes = [f32p, C.c_int, C.c_float, f32p, f32p, f32p, C.c_int, f32p, C.c_int, C.c_float, C.c_int, C.c_int,
                                 np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")]
    return L


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    L = build()
    for R in (64, 32, 16):
        cell, shipped = SHAPES[R]
        for tname in ("Silverstone", "Monza", "Spa"):
            track = WM.O.Track(tname)
            px, py, rot, fan = WM.poses(track, N, R)
            print("\n%s, %d rays (%d agents per wave), %d live poses, front image, %g px cells" % (tname, R, 64 // R, px.size, cell))
            print("threshold  range |  cells  point rounds  exact passes (phase 1 + phase 2) |   p1 cells  p2 cells | pending  voted | vs shipped: cells rounds passes")
            base = None
            for rng_px in (shipped, 64.0, 1.0e30):
                for thr in THRESHOLDS:
                    out = np.zeros(9)
                    rc = L.wavemodel_vote(track.segments, track.S, cell, px, py, rot, px.size, fan, R, rng_px, 8, thr, out)
                    assert rc == 0, rc
                    tot = out[0:3] + out[3:6]
                    if base is None:
                        base = tot.copy()  # (first row: no vote, shipped range)
                    print("%9s %6s | %6.2f %13.2f %13.2f | %10.2f %9.2f | %7.1f %6.2f | %+6.1f%% %+6.1f%% %+6.1f%%"
                          % ("off" if thr == 0 else thr, "none" if rng_px > 1e9 else "%g" % rng_px, tot[0], tot[1], tot[2], out[0], out[3], out[6], out[7],
                             *(100.0 * (tot - base) / base)))


if __name__ == "__main__":
    main()
