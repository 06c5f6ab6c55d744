"""The reference's Deep-Q learner on bird's-eye frames (RLRacers/DQN_CNN/dq_cnn_racer_sim.cpp) for a whole population instead of its
one agent: N agents act epsilon-greedily on their own camera frame, every transition's two grey planes go into the device's frame ring,
and after each episode the Q-network takes the reference's temporal-difference steps in PyTorch on batches gathered from that ring.

    python examples/dqn_cnn_racer.py [--agents 256] [--frame-size 96] [--episodes 3] [--max-steps 256] [--capacity 65536] [--batch 32]
                                     [--passes 4] [--uniform] [--graph-chunk 8] [--device-policy] [--track Austin]

1. act: the Q-network on gray(frame), epsilon-greedy (epsilon 0.99, 0.01 less every episode) -- in PyTorch or, with --device-policy,
   in the device's two act kernels with no PyTorch op in the loop;
2. step, camera (one call per step: the frame is the push's next_frames and the next act's frames), push into the ring;
3. update: --passes sequential walks over the ring in batches of --batch (the reference's updateDQN; --uniform samples instead), each
   batch one dqn_cnn.update (target = q with r + 0.99 amax(q') at the action, mse_loss, Adam 1e-4); then the ring is emptied;
4. hand over (--device-policy): the flattened parameters device to device.
--frame-size is the network's image size (the device path does not resize).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import dqn_cnn  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=256)
    ap.add_argument("--frame-size", type=int, default=96)
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=256)
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--uniform", action="store_true")
    ap.add_argument("--graph-chunk", type=int, default=0)
    ap.add_argument("--track", default="Austin")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-policy", action="store_true")
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    S = a.frame_size
    venv = VectorEnvironment(a.track, a.agents, auto_reset=False, randomize_lane=True, randomize_heading=True, seed=a.seed)
    venv.enable_camera(width=S, height=S, fmt="rgba")
    model = dqn_cnn.QCNN(S).to(venv.device)
    optimizer = torch.optim.Adam(model.parameters(), lr=dqn_cnn.LEARNING_RATE)
    epsilon = dqn_cnn.EPSILON

    def flat():
        return dqn_cnn.qcnn_params_from_state_dict(model.state_dict(), image_size=S)

    first = flat().clone()
    cfg = dqn_cnn.qcnn_config_from_state_dict(model.state_dict(), image_size=S, mode="eps_greedy", epsilon=epsilon, seed=a.seed)
    venv.enable_image_dqn(cfg, first, capacity=a.capacity)
    # the first step's Q-values from the device and from the module
    venv.reset()
    frames = venv.camera()
    q = torch.empty((a.agents, cfg.num_actions), device=venv.device)
    venv.image_dqn_act(frames, {"q": q})
    with torch.no_grad():
        q_torch = model(dqn_cnn.gray(frames))
    policy = "device" if a.device_policy else "torch"
    out = {"q": q.clone(), "q_torch": q_torch, "epsilon": [], "steps": [], "ring": [], "loss": []}
    draw = 0
    for episode in range(a.episodes):
        t0 = time.perf_counter()
        taken = dqn_cnn.run_episode(venv, model, max_steps=a.max_steps, graph_chunk=a.graph_chunk, policy=policy)["steps"]
        size, pushed = venv.env.qcnn_ring_size()
        t1 = time.perf_counter()
        losses = []
        for _ in range(a.passes):
            for at in range(0, size, a.batch):
                batch = venv.image_dqn_batch(a.batch, "uniform" if a.uniform else "sequential", draw if a.uniform else at)
                losses.append(dqn_cnn.update(model, optimizer, batch))
                draw += 1
        loss = float(torch.stack(losses).mean()) if losses else float("nan")
        venv.env.qcnn_ring_reset()
        if a.device_policy:
            venv.set_image_dqn_params(flat())
        out["epsilon"].append(epsilon), out["steps"].append(taken), out["ring"].append((size, pushed)), out["loss"].append(loss)
        print("episode %d: eps %.2f, %d steps in %.2f s, %d transitions (%d pushed), %d updates in %.2f s, mean loss %.4g" % (
            episode, epsilon, taken, t1 - t0, size, pushed, len(losses), time.perf_counter() - t1, loss))
        epsilon = epsilon - dqn_cnn.EPSILON_DISCOUNT if epsilon > dqn_cnn.EPSILON_DISCOUNT else 0.0
        venv.set_image_dqn_epsilon(epsilon)
    out["ring_after"] = venv.env.qcnn_ring_size()
    out["params_first"], out["params"] = first, flat()
    out["device_params"] = torch.from_numpy(venv.env.qcnn_get_params()).to(venv.device) if a.device_policy else None
    out["final_epsilon"] = epsilon
    venv.close()
    return out


if __name__ == "__main__":
    main()
