"""The reference's imitation learner (ImitationLearningTransformer/) for a whole population: demonstrations from the device's
potential-field expert, the LidarTransformer trained on them in PyTorch with the reference's recipe, and N agents driven by the
trained policy with the device's act kernel.

    python examples/imitation_racer.py [--agents 1024] [--demo-steps 512] [--epochs 5] [--drive-steps 512] [--track Austin]
                                       [--graph-chunk 8] [--torch-driver] [--small]

1. record: 7 rays from -90 to 90 degrees; the hit points and the expert's actions of every living agent (demonstrations.py);
2. train: MSE on the normalised controls, Adam 1e-4, batches of 128 (train.py), on the device tensors;
3. hand over: the module's weights as one flat vector (imitation.lidar_params_from_state_dict -> enable_lidar_policy);
4. drive: `step`, then `lidar_act`, the loop of infer_torch_traced_main.cpp:138-148 (imitation.drive).
--torch-driver drives with the PyTorch module between the steps instead, for comparison.  --small is a reduced network and run.
"""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import imitation  # noqa: E402
from openkitchen_amd.demonstrations import collect_demonstrations  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

SMALL = dict(agents=64, demo_steps=256, epochs=2, drive_steps=64, net=dict(d_model=32, nhead=2, num_layers=2, dim_feedforward=64, head_hidden1=32,
                                                                         head_hidden2=16))


def torch_drive(venv, model, steps):
    """The same loop with the module's forward between single-step launches."""
    venv.reset()
    with torch.no_grad():
        for _ in range(steps):
            venv.step()
            points = torch.stack([venv.rel_x, venv.rel_y], dim=2)
            action = imitation.denormalize_controls(model.driven(imitation.normalize_points(points)))
            venv.set_action(action[:, 0], action[:, 1])
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--demo-steps", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--drive-steps", type=int, default=512)
    ap.add_argument("--track", default="Austin")
    ap.add_argument("--graph-chunk", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--torch-driver", action="store_true")
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    net = {}
    if a.small:
        a.agents, a.demo_steps, a.epochs, a.drive_steps, net = (SMALL[k] for k in ("agents", "demo_steps", "epochs", "drive_steps", "net"))
    torch.manual_seed(a.seed)
    fan = np.linspace(-90, 90, 7).astype(np.float32)  # infer_torch_traced_main.cpp:53-59
    venv = VectorEnvironment(a.track, a.agents, ray_angles_deg=fan, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=a.seed,
                             reward="step")
    # 1. demonstrations (the steering clamp keeps the expert inside the controls' range of +-2 degrees)
    venv.enable_expert("potfield", lookahead=2, goal_wrap=False, clamp_deg=2.0)
    demos = collect_demonstrations(venv, a.demo_steps, seed=a.seed)
    points, actions = imitation.demonstration_rows(demos)
    print("recorded %d samples of living agents out of %d" % (points.shape[0], a.agents * a.demo_steps))
    # 2. training
    model = imitation.LidarTransformer(n_points=7, **net).to(venv.device)
    t0 = time.perf_counter()
    losses = imitation.train(model, points, actions, epochs=a.epochs, seed=a.seed)
    print("trained %d epochs in %.1f s: loss %s" % (a.epochs, time.perf_counter() - t0, " ".join("%.4g" % v for v in losses)))
    # 3. hand-over
    cfg = model.lidar_config()
    venv.enable_lidar_policy(cfg, imitation.lidar_params_from_state_dict(model.state_dict(), positional=model.positional))
    # the first driven step, device against the module in float64 from the same weights
    venv.reset()
    venv.step()
    rec = {"action": torch.empty((a.agents, 2), device=venv.device), "input": torch.empty((a.agents, 7, 2), device=venv.device)}
    venv.lidar_act(rec)
    with torch.no_grad():
        want = copy.deepcopy(model).double().driven(rec["input"].double())
    got = imitation.normalize_controls(rec["action"].double())
    print("first step: max |device - float64 module| = %.4g (normalised outputs up to %.3g)" % (float((got - want).abs().max()), float(want.abs().max())))
    # 4. driving
    t0 = time.perf_counter()
    if a.torch_driver:
        steps = torch_drive(venv, model, a.drive_steps)
    else:
        steps = imitation.drive(venv, a.drive_steps, graph_chunk=a.graph_chunk)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    alive = int((~venv.done).sum())
    print("drove %d agents for %d steps with the %s in %.3f s (%.3g agent-steps/s); %d alive at the end, mean episode length so far %.1f"
          % (a.agents, steps, "PyTorch module" if a.torch_driver else "device act", dt, a.agents * steps / dt, alive, float(venv.episode_steps.float().mean())))
    print("actions finite %s" % bool(torch.isfinite(venv.throttle).all() and torch.isfinite(venv.steering).all()))
    venv.close()


if __name__ == "__main__":
    main()
