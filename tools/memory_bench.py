"""The world-model racers' memory: okenv_memory_act per call at 256 and 1024 candidates on Silverstone, reference
shape (128 x 128 frames, the reference's encoder, latent 32; the GRU with H = 512 and L = 3; controller 544-16-8-1) with carry 0 and 1,
against okenv_world_act on the same frames (what the memory adds), each of its kernels alone (okenv_debug_memory_stages), and the
PyTorch path with the same weights on the same frames (the encoder module, GRUDynamics at T = 1 with a carried h,
cmaes.BatchedController), launched eagerly and as one replayed torch.cuda.graph.

    python tools/memory_bench.py [--out profiles/memory/memory_bench.json] [--reps 5] [--calls 5] [--populations 256 1024]

Every figure is the time between two HIP events on the environment's stream around --calls calls, per call, median / min / max of
--reps repetitions after one warm-up region.  Nothing steps between the calls and every agent acts (skip_crashed 0); with carry the
hidden state moves from call to call, which changes no kernel's work.  Derived, not measured: the memory's matrix work is 4.00 M
multiply-adds per agent and act with carry (8.2 GFLOP at 1024 candidates) and 1.64 M without, and its network vector is 16 MB, read at
least once per act."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd import worldmodel as wm  # noqa: E402
from world_bench import FRAME, TRACK, graphed, timed_us  # noqa: E402


def macs_per_agent(Z, H, L, carry):
    """Multiply-adds of the GRU's matrices for one agent and act."""
    total = 0
    for l in range(L):
        total += 3 * H * ((Z + 2 if l == 0 else H) + (H if carry else 0))
    return total


def population(N, reps, calls):
    torch.manual_seed(3)
    model, memory = wm.Encoder(FRAME, wm.Z_DIM), wm.GRUDynamics(wm.Z_DIM)
    out = {}
    for carry in (0, 1):
        racers = wm.WorldModelRacers(TRACK, N, model, seed=0, encoder="device", skip_crashed=False, memory=memory, carry=bool(carry))
        venv, env, res = racers.venv, racers.venv.env, {}
        venv.reset()
        venv.step(n_steps=8)
        frames = venv.camera()
        # a controller per candidate at the size a CMA-ES population has; the full-covariance solver is not asked for 8 865 dimensions
        racers.controller.set_params(torch.randn(N, racers.num_params, device=venv.device) * 0.05)
        env.memory_set_params("controllers", racers.controller.flat)
        if carry == 0:  # the racers without a memory, on the same frames
            env.world_set_params("controllers", torch.zeros(N, env.world_num_params()[1], device=venv.device))
            out["world_act_us"] = timed_us(lambda: env.world_act(frames), reps, calls)
        res["memory_act_us"] = timed_us(lambda: env.memory_act(frames), reps, calls)
        stages = [("encoder", capi.MEMORY_STAGE_ENCODER), ("input", capi.MEMORY_STAGE_INPUT)]
        stages += [("layer%d" % l, capi.MEMORY_STAGE_LAYER0 << l) for l in range(memory.layers)] + [("head", capi.MEMORY_STAGE_HEAD)]
        for name, stage in stages:
            res[name + "_kernel_us"] = timed_us(lambda: env.memory_act(frames, None, stages=stage), reps, calls)
        res["memory_adds_us"] = res["memory_act_us"]["median"] - out["world_act_us"]["median"]
        # the first act from a zero state and a zero stored action, both ways
        zeros = torch.zeros(N).numpy()

        def torch_act():
            racers.frame.copy_(frames)
            racers._memory_iteration()

        env.memory_reset()
        env.set(capi.F_THROTTLE, zeros)
        env.set(capi.F_STEER, zeros)
        got = torch.empty(N, device=venv.device)
        env.memory_act(frames, {"out": got})
        racers._h.zero_()
        env.set(capi.F_THROTTLE, zeros)
        env.set(capi.F_STEER, zeros)
        torch_act()
        res["max_abs_difference_first_act"] = float((got - venv.steering / wm.STEER_SCALE).abs().max())
        res["torch_eager_us"] = timed_us(torch_act, reps, calls)
        res["torch_graph_us"] = timed_us(graphed(venv.device, torch_act).replay, reps, calls)
        med = res["memory_act_us"]["median"]
        res["torch_eager_over_memory_act"] = res["torch_eager_us"]["median"] / med
        res["torch_graph_over_memory_act"] = res["torch_graph_us"]["median"] / med
        res["matrix_gflop_per_act"] = 2e-9 * macs_per_agent(wm.Z_DIM, memory.hidden, memory.layers, carry) * N
        out["carry_%d" % carry] = res
        venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "memory", "memory_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--populations", type=int, nargs="+", default=[256, 1024])
    a = ap.parse_args()
    wc, mc = capi.world_config(image_size=FRAME), capi.memory_config()
    res = {"device": torch.cuda.get_device_name(0), "track": TRACK, "frame": FRAME,
           "network": "GRU %d -> %d x %d, head %d; controller %d-%d-%d-1" % (wc.latent + 2, mc.hidden, mc.layers, wc.latent, wc.latent + mc.hidden,
                                                                              mc.ctrl_hidden, mc.ctrl_hidden // 2),
           "plan": {"carry_%d" % c: capi.memory_plan(wc, capi.memory_config(carry=c)) for c in (0, 1)}, "lds_bytes": capi.memory_lds_bytes(wc, mc),
           "network_floats": capi.memory_num_params(wc, mc)[0], "reps": a.reps, "calls_per_region": a.calls,
           "multiply_adds_per_agent": {"carry_%d" % c: macs_per_agent(wc.latent, mc.hidden, mc.layers, c) for c in (0, 1)},
           "populations": {str(N): population(N, a.reps, a.calls) for N in a.populations}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
