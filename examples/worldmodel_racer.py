"""The reference's world-model racer (WorldModelVaeRnn/) for a whole CMA-ES population at once: bird's-eye frames recorded from the
device's potential-field expert, the conv VAE trained on them in PyTorch with the reference's recipe, and generations of candidates --
every candidate an agent of one handle, its controller fed [mu | sin(rot), cos(rot)] from the shared encoder, scored by its distance
to the lane centre -- with the encoder's forward once per step in PyTorch or, with --device-encoder, in the device's act kernels.

    python examples/worldmodel_racer.py [--population 256] [--frame-size 128] [--base-ch 64] [--latent 32] [--demo-agents 64]
                                        [--demo-steps 64] [--epochs 2] [--generations 5] [--max-steps 400] [--graph-chunk 8]
                                        [--device-encoder] [--keep-crashed] [--track Silverstone]
                                        [--memory] [--memory-hidden 64] [--memory-epochs 2] [--no-carry] [--device-update]

1. record: every living agent's frame while the expert drives (demonstrations.collect_demonstrations(images=True));
2. train: binary cross-entropy of the reconstruction plus the KL term, Adam 2e-4 (train_vae.py);
3. generations: sample, one batched rollout (camera -> act -> step -> score, in graph chunks, until nobody is alive), tell
   (worldmodel.WorldModelRacers).  The reference evaluates its 30 candidates one after another.
--frame-size is the encoder's image size, a multiple of 16 up to 128; the camera renders at it, there is no resize.

With --memory the racer is the reference's Vision + Memory + Controller: between 2 and 3 the expert drives again, the latents come from
the device encoder (worldmodel.collect_latents), the GRU dynamics model is trained on them with the reference's recipe
(worldmodel.train_memory, or with --device-update on the device: worldmodel.train_memory_device, okenv_memory_update), and every
candidate's controller reads [mu | h_top] (okenv_memory_act with --device-encoder).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import worldmodel as wm  # noqa: E402
from openkitchen_amd.demonstrations import collect_demonstrations  # noqa: E402
from openkitchen_amd.flow import demonstration_rows  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=256)
    ap.add_argument("--frame-size", type=int, default=128)
    ap.add_argument("--base-ch", type=int, default=64)
    ap.add_argument("--latent", type=int, default=wm.Z_DIM)
    ap.add_argument("--demo-agents", type=int, default=64)
    ap.add_argument("--demo-steps", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--generations", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=400)
    ap.add_argument("--graph-chunk", type=int, default=8)
    ap.add_argument("--track", default="Silverstone")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-encoder", action="store_true")
    ap.add_argument("--keep-crashed", action="store_true", help="act for crashed candidates too (skip_crashed = 0)")
    ap.add_argument("--memory", action="store_true", help="train the GRU dynamics model and feed the controllers [mu | h_top]")
    ap.add_argument("--memory-hidden", type=int, default=64,
                    help="the memory's width H.  The solver keeps a full covariance over a controller's parameters: H = 64 gives 1 697 of them; "
                         "the reference's H = 512 gives 8 865, a 629 MB matrix -- the limit the reference's Readme names")
    ap.add_argument("--memory-layers", type=int, default=wm.MEMORY_LAYERS)
    ap.add_argument("--memory-epochs", type=int, default=2)
    ap.add_argument("--no-carry", action="store_true", help="the reference as written: the hidden state starts from zero at every act")
    ap.add_argument("--device-update", action="store_true", help="train the memory on the device (okenv_memory_update) instead of in PyTorch")
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    # 1. frames
    venv = VectorEnvironment(a.track, a.demo_agents, auto_reset=False, randomize_lane=True, randomize_heading=True, seed=a.seed)
    venv.enable_camera(width=a.frame_size, height=a.frame_size, fmt="rgba")
    venv.enable_expert("potfield", lookahead=2, goal_wrap=False, clamp_deg=wm.STEER_SCALE)
    frames, _ = demonstration_rows(collect_demonstrations(venv, a.demo_steps, images=True, seed=a.seed))
    print("recorded %d frames of living agents out of %d" % (frames.shape[0], a.demo_agents * a.demo_steps))
    device = venv.device
    # 2. the VAE
    channels = tuple(a.base_ch * m for m in (1, 2, 4, 8))
    model = wm.VAE(a.frame_size, a.latent, channels).to(device)
    t0 = time.perf_counter()
    losses = wm.train_vae(model, frames, epochs=a.epochs, seed=a.seed)
    print("trained %d epochs in %.1f s: loss per frame %s" % (a.epochs, time.perf_counter() - t0, " ".join("%.5g" % v for v in losses)))
    memory = memory_stats = memory_losses = None
    if a.memory:  # 2b. the memory: the expert drives again, the latents come from the device encoder
        model.eval()
        sd = model.enc.state_dict()
        venv.enable_world_racers(wm.world_config_from_state_dict(sd, a.frame_size), wm.world_params_from_state_dict(sd, a.frame_size).to(device))
        venv.set_world_controllers(torch.zeros(a.demo_agents, venv.env.world_num_params()[1], device=device))
        latents, actions, alive = wm.collect_latents(venv, a.demo_steps, drive=lambda v: v.expert_act())
        memory = wm.GRUDynamics(a.latent, a.memory_hidden, a.memory_layers).to(device)
        t0 = time.perf_counter()
        if a.device_update:  # the same recipe in the device's kernels; the trained vector carries its statistics
            memory_losses, memory_stats, memory = wm.train_memory_device(venv, memory, latents, actions, alive, epochs=a.memory_epochs, seed=a.seed,
                                                                         carry=not a.no_carry)
        else:
            memory_losses, memory_stats = wm.train_memory(memory, latents, actions, alive, epochs=a.memory_epochs, seed=a.seed)
        print("trained the memory (H = %d, %d layers) %d epochs %s in %.1f s: loss %s"
              % (a.memory_hidden, a.memory_layers, a.memory_epochs, "on the device" if a.device_update else "in PyTorch", time.perf_counter() - t0,
                 " ".join("%.5g" % v for v in memory_losses)))
    venv.close()
    # 3. generations
    racers = wm.WorldModelRacers(a.track, a.population, model.enc, seed=a.seed, encoder="device" if a.device_encoder else "torch",
                                 max_steps=a.max_steps, graph_chunk=a.graph_chunk, skip_crashed=not a.keep_crashed, memory=memory,
                                 memory_stats=memory_stats, carry=not a.no_carry, memory_shape=(a.memory_hidden, a.memory_layers))
    first = None
    if a.device_encoder and not a.memory:  # the first frames, both ways: the device's mu against the PyTorch module's
        racers.venv.reset()
        frame = racers.venv.camera()
        racers.set_params(racers.solver.sample())
        first = {"mu": torch.zeros(a.population, a.latent, device=device)}
        racers.venv.env.world_act(frame, first)
        with torch.no_grad():
            first["mu_torch"] = racers.model(wm.frames_to_input(frame))[0]
        alive = ~racers.venv.done
        print("first step: max |device - PyTorch module| = %.4g on mu (up to %.3g in size)"
              % (float((first["mu"] - first["mu_torch"])[alive].abs().max()), float(first["mu_torch"].abs().max())))
    best, means, fitnesses, all_steps = [], [racers.solver.mean.copy()], [], []
    for g in range(a.generations):
        t0 = time.perf_counter()
        top, steps = racers.run_generation()
        dt = time.perf_counter() - t0
        best.append(top)
        fitnesses.append(racers.fitness.copy())
        all_steps.append(steps)
        means.append(racers.solver.mean.copy())
        print("generation %d: %d candidates, %d steps with the %s in %.3f s; best fitness %.3f, mean %.3f"
              % (g, a.population, steps, "device encoder" if a.device_encoder else "PyTorch encoder", dt, top, float(racers.fitness.mean())))
    out = {"model": model, "config": racers.config, "first": first, "best": best, "fitness": racers.fitness, "means": means, "losses": losses,
           "memory": memory, "memory_stats": memory_stats, "memory_losses": memory_losses, "fitnesses": fitnesses, "steps": all_steps}
    print("fitness finite %s" % bool(torch.isfinite(torch.as_tensor(racers.fitness)).all()))
    racers.venv.close()
    return out


if __name__ == "__main__":
    main()
