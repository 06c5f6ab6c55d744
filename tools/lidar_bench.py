"""The lidar transformer driver: okenv_lidar_act per call at 1024 and 4096 agents, reference shape, against the
PyTorch module in eager fp32 with the same weights (its normalise and denormalise included), with a step launch beside both.

    python tools/lidar_bench.py [--out profiles/lidar/lidar_bench.json] [--reps 5] [--calls 20]

Every figure is the time between two HIP events on the environment's stream around --calls calls, per call, median / min / max of
--reps repetitions after one warm-up region.  The observation does not change between the calls (nothing steps in between), so both
sides do the same work in every call.  8.75 MFLOP per agent: 36 GFLOP per act at 4096 agents, 0.23 ms at the f32 peak."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import imitation  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

RAYS = np.linspace(-90, 90, 7).astype(np.float32)
FLOP_PER_AGENT = 8.75e6


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_us(fn, reps, calls):
    def region():
        for _ in range(calls):
            fn()

    region()
    return stats([1e3 * event_ms(region) / calls for _ in range(reps)])


def population(N, reps, calls):
    venv = VectorEnvironment("Austin", N, ray_angles_deg=RAYS, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=0)
    torch.manual_seed(0)
    model = imitation.LidarTransformer().to(venv.device).eval()
    venv.enable_lidar_policy(model.lidar_config(), imitation.lidar_params_from_state_dict(model.state_dict()))
    venv.reset()
    venv.step(n_steps=8)
    rec = {"action": torch.empty((N, 2), device=venv.device), "input": torch.empty((N, 7, 2), device=venv.device),
           "alive": torch.empty(N, dtype=torch.uint8, device=venv.device)}

    def torch_act():
        with torch.no_grad():
            points = torch.stack([venv.rel_x, venv.rel_y], dim=2)
            action = imitation.denormalize_controls(model.driven(imitation.normalize_points(points)))
            venv.set_action(action[:, 0], action[:, 1])

    out = {"lidar_act_us": timed_us(venv.lidar_act, reps, calls), "lidar_act_recording_us": timed_us(lambda: venv.lidar_act(rec), reps, calls),
           "torch_eager_fp32_us": timed_us(torch_act, reps, calls)}
    # the two agree on what they compute (fp32 both, other summation orders)
    venv.lidar_act(rec)
    torch_act()
    torch.cuda.synchronize()
    out["max_abs_action_difference"] = float((rec["action"] - torch.stack([venv.throttle, venv.steering], dim=1)).abs().max())
    out["step_us"] = timed_us(venv.step, reps, calls)
    out["lidar_act_tflops"] = FLOP_PER_AGENT * N / (out["lidar_act_us"]["median"] * 1e-6) / 1e12
    venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "lidar", "lidar_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "track": "Austin", "rays": 7, "network": "7 points, d_model 128, 8 heads, 3 layers, ff 512, head 896-256-64-2",
           "reps": a.reps, "calls_per_region": a.calls, "flop_per_agent": FLOP_PER_AGENT,
           "populations": {str(N): population(N, a.reps, a.calls) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
