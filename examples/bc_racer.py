"""The reference's behavioural-cloning driver (BehavioralCloning/) for a whole population: demonstrations with bird's-eye frames from the
device's potential-field expert (examples/collect_bc_dataset.py's setup), the image policy trained on them in PyTorch with the
reference's recipe, and N agents driven by it at a constant throttle -- the forward once per step in PyTorch or, with
--device-policy, in the device's two act kernels.

    python examples/bc_racer.py [--agents 256] [--frame-size 96] [--demo-steps 128] [--epochs 3] [--steps 256] [--episodes 2]
                                [--graph-chunk 8] [--device-policy] [--track Austin]

1. record: every living agent's frame and the expert's action (demonstrations.collect_demonstrations(images=True));
2. train: MSE of the tanh output against the expert's steering / 10, clamped to +-1, Adam 3e-4 (env_train_bc.py);
3. hand over (--device-policy): the weights as one flat vector (bc.cnn_params_from_state_dict -> enable_image_policy);
4. drive: `step`, `camera()`, the forward, throttle 100 and steering 10 x output (bc.drive), and the share of agents that survive
   every episode.
--frame-size is the policy's image size: at least 36 for the reference's three convolutions, at most 119 for the conv kernel's LDS.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import bc  # noqa: E402
from openkitchen_amd.demonstrations import collect_demonstrations  # noqa: E402
from openkitchen_amd.flow import demonstration_rows  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--frame-size", type=int, default=96)
    ap.add_argument("--demo-steps", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--graph-chunk", type=int, default=8)
    ap.add_argument("--track", default="Austin")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-policy", action="store_true")
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    venv = VectorEnvironment(a.track, a.agents, auto_reset=False, randomize_lane=True, randomize_heading=True, seed=a.seed)
    venv.enable_camera(width=a.frame_size, height=a.frame_size, fmt="rgba")
    # 1. demonstrations (the steering clamp keeps the expert inside the policy's range of +-10 degrees)
    venv.enable_expert("potfield", lookahead=2, goal_wrap=False, clamp_deg=bc.STEER_SCALE)
    demos = collect_demonstrations(venv, a.demo_steps, images=True, seed=a.seed)
    frames, actions = demonstration_rows(demos)
    print("recorded %d frames of living agents out of %d" % (frames.shape[0], a.agents * a.demo_steps))
    # 2. training
    model = bc.PolicyCNN(a.frame_size).to(venv.device)
    t0 = time.perf_counter()
    losses = bc.train(model, frames, actions, epochs=a.epochs, seed=a.seed)
    print("trained %d epochs in %.1f s: loss %s" % (a.epochs, time.perf_counter() - t0, " ".join("%.4g" % v for v in losses)))
    # 3. hand-over
    sd = model.state_dict()
    cfg = bc.cnn_config_from_state_dict(sd, image_size=a.frame_size)
    if a.device_policy:
        venv.enable_image_policy(cfg, bc.cnn_params_from_state_dict(sd, image_size=a.frame_size))
    # the first driven step, recorded: the PyTorch forward's output and, with --device-policy, the device's on the same frames
    venv.reset()
    venv.step()
    frame = venv.camera()
    with torch.no_grad():
        out_torch = model(bc.frames_to_input(frame))[:, 0].contiguous()
    first = {"out_torch": out_torch, "out": out_torch}
    if a.device_policy:
        first["out"] = torch.empty(a.agents, device=venv.device)
        venv.image_act(frame, {"out": first["out"]})
        print("first step: max |device - PyTorch forward| = %.4g on the output" % float((first["out"] - out_torch).abs().max()))
    # 4. driving
    survival = []
    for episode in range(a.episodes):
        t0 = time.perf_counter()
        steps = bc.drive(venv, model, a.steps, graph_chunk=a.graph_chunk, policy="device" if a.device_policy else "torch")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        survival.append(float((~venv.done).float().mean()))
        print("episode %d: %d agents, %d steps with the %s in %.3f s (%.3g agent-steps/s); survival %.3f"
              % (episode, a.agents, steps, "device policy" if a.device_policy else "PyTorch forward", dt, a.agents * steps / dt, survival[-1]))
    out = {"model": model, "config": cfg, "first": first, "survival": survival, "losses": losses,
           "throttle": venv.throttle.clone(), "steering": venv.steering.clone()}
    print("actions finite %s" % bool(torch.isfinite(out["throttle"]).all() and torch.isfinite(out["steering"]).all()))
    venv.close()
    return out


if __name__ == "__main__":
    main()
