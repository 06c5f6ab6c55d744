"""A behavioural-cloning data set from the reference's potential-field expert, for a whole population at once: what
FieldNavigators/collect_data/collect_data_random.cpp records for one agent behind a window, in both of its file formats.

    python examples/collect_bc_dataset.py [--agents 1024] [--steps 64] [--track Silverstone] [--out bc_dataset] [--files 2000]

The expert (PotFieldAgent with the collector's 10-degree steering clamp), the step and the camera run on the GPU
(openkitchen_amd/demonstrations.py); the samples come back as [T, N, ...] tensors, saved whole as `<out>/<track>_random.npz`
and, for the first --files living samples, as the reference's `laser2d_<track>_<ctr>.txt` and
`birdseye_<track>_<ctr>.txt/.png` files.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd.dataset import BirdseyeWriter, Laser2dWriter  # noqa: E402
from openkitchen_amd.demonstrations import collect_demonstrations  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--out", default="bc_dataset")
    ap.add_argument("--files", type=int, default=2000, help="samples also written in the reference's per-sample file formats")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    fan = np.linspace(-90, 90, 7).astype(np.float32)  # PotentialFieldAgent.hpp:38-44
    venv = VectorEnvironment(a.track, a.agents, ray_angles_deg=fan, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=a.seed)
    venv.enable_expert("potfield", lookahead=2, goal_wrap=False, clamp_deg=10.0)
    venv.enable_camera(96, 96)
    t0 = time.perf_counter()
    out = collect_demonstrations(venv, a.steps, images=True, seed=a.seed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    alive = out["alive"].cpu().numpy()
    print("%d samples (%d of living agents) in %.3f s: %.3g samples/s" % (alive.size, int(alive.sum()), dt, alive.size / dt))
    os.makedirs(a.out, exist_ok=True)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    np.savez_compressed(os.path.join(a.out, "%s_random.npz" % a.track), **host)
    # the reference's formats: a prefix of the recording (one file or pair per sample is a host-side cost)
    steps = max(1, min(a.steps, -(-a.files // a.agents)))
    laser = Laser2dWriter(os.path.join(a.out, "%s_random_laser2d" % a.track), a.track)
    bev = BirdseyeWriter(os.path.join(a.out, "%s_random_birdseye" % a.track), a.track)
    n1 = laser.save_recorded(host["actions"][:steps], host["rel_xy"][:steps], host["alive"][:steps])
    n2 = bev.save_recorded(host["actions"][:steps], host["frames"][:steps], host["alive"][:steps])
    print("wrote %d laser2d files and %d birdseye pairs under %s" % (n1, n2, a.out))
    venv.close()


if __name__ == "__main__":
    main()
