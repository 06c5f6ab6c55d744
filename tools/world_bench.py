"""The world-model racers: okenv_world_act per call at 256 and 1024 candidates on Silverstone, reference shape
(128 x 128 frames, four stride-2 convolutions 3-64-128-256-512, latent 32, controller 34-16-8-1), and each of its kernels alone,
against the PyTorch path with the same weights on the same frames (the encoder module behind frames_to_input, the heading and
cmaes.BatchedController), launched eagerly and as one replayed torch.cuda.graph; and one whole generation of
worldmodel.WorldModelRacers with skip_crashed 0 and 1.

    python tools/world_bench.py [--out profiles/world/world_bench.json] [--reps 5] [--calls 5] [--max-steps 400]

Every act figure is the time between two HIP events on the environment's stream around --calls calls, per call, median / min / max of
--reps repetitions after one warm-up region.  Nothing steps between the act's calls, so every call does the same work (every agent
acts: skip_crashed 0).  A generation is timed on the host around run_generation, which ends with a synchronising read of the fitness.
832.6 MFLOP per frame: 0.85 TFLOP per call at 1024 candidates, 5.42 ms at the f32 matrix peak (157.3 TFLOP/s), 1.36 ms at 256 --
derived, not measured."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd import worldmodel as wm  # noqa: E402

FRAME = 128
PEAK_TFLOPS = 157.3
TRACK = "Silverstone"


def flop_per_layer(cfg):
    """The four convolutions and fc_mu, in FLOP per frame."""
    out, cin = [], 3
    for l, c in enumerate(cfg.channels):
        side = cfg.image_size >> (l + 1)
        out.append(2.0 * side * side * c * cin * 16)
        cin = c
    return out + [2.0 * cin * (cfg.image_size // 16) ** 2 * cfg.latent]


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


def graphed(device, fn):
    """fn captured once on a side stream after one eager call there (the convolutions choose their kernels on the first call)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    torch.cuda.synchronize()
    return graph


def population(N, reps, calls, max_steps):
    torch.manual_seed(3)
    model = wm.Encoder(FRAME, wm.Z_DIM)
    out = {}
    for skip in (0, 1):
        racers = wm.WorldModelRacers(TRACK, N, model, seed=0, encoder="device", max_steps=max_steps, skip_crashed=bool(skip))
        venv, cfg = racers.venv, racers.config
        if skip == 0:
            venv.reset()
            venv.step(n_steps=8)
            frames = venv.camera()
            racers.set_params(racers.solver.sample())
            out["world_act_us"] = timed_us(lambda: venv.env.world_act(frames), reps, calls)
            for name, stage in capi.WORLD_STAGES:
                out[name + "_kernel_us"] = timed_us(lambda: venv.env.world_act(frames, None, stages=stage), reps, calls)
            got = torch.empty(N, device=venv.device)
            venv.env.world_act(frames, {"out": got})
            result = [None]

            def torch_act():
                with torch.no_grad():
                    mu = racers.model(wm.frames_to_input(frames))[0]
                    state = torch.cat([mu, torch.sin(venv.rot)[:, None], torch.cos(venv.rot)[:, None]], dim=1)
                    result[0] = racers.controller.forward(state)[:, 0]
                    venv.throttle.fill_(wm.THROTTLE)
                    torch.mul(result[0], wm.STEER_SCALE, out=venv.steering)

            out["torch_eager_us"] = timed_us(torch_act, reps, calls)
            out["max_abs_difference"] = float((got - result[0]).abs().max())
            out["torch_graph_us"] = timed_us(graphed(venv.device, torch_act).replay, reps, calls)
            flops = flop_per_layer(cfg)
            med = out["world_act_us"]["median"]
            out["world_act_tflops"] = sum(flops) * N / (med * 1e-6) / 1e12
            out["kernel_tflops"] = {("conv%d" % l if l < 4 else "latent"): f * N / (out[("conv%d" % l if l < 4 else "latent") + "_kernel_us"]["median"] * 1e-6) / 1e12
                                    for l, f in enumerate(flops)}
            out["matrix_peak_floor_us"] = sum(flops) * N / (PEAK_TFLOPS * 1e12) * 1e6
            out["fraction_of_matrix_peak"] = out["matrix_peak_floor_us"] / med
            out["torch_eager_over_world_act"] = out["torch_eager_us"]["median"] / med
            out["torch_graph_over_world_act"] = out["torch_graph_us"]["median"] / med
        racers.run_generation()  # (captures the chunk's graph)
        times, steps = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps.append(racers.run_generation()[1])
            times.append(1e3 * (time.perf_counter() - t0))
        out["generation_skip_crashed_%d" % skip] = {"ms": stats(times), "steps": steps}
        venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "world", "world_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=400)
    ap.add_argument("--populations", type=int, nargs="+", default=[256, 1024])
    a = ap.parse_args()
    cfg = capi.world_config(image_size=FRAME)
    res = {"device": torch.cuda.get_device_name(0), "track": TRACK,
           "network": "conv %s, k 4, stride 2, padding 1 -> flatten -> %d; controller %d-%d-%d-1" % (
               tuple(cfg.channels), cfg.latent, cfg.latent + 2, cfg.hidden, cfg.hidden // 2),
           "frame": FRAME, "plan": capi.world_plan(cfg), "lds_bytes": capi.world_lds_bytes(cfg), "reps": a.reps, "calls_per_region": a.calls,
           "max_steps": a.max_steps, "flop_per_frame": sum(flop_per_layer(cfg)), "flop_per_layer": flop_per_layer(cfg),
           "matrix_peak_tflops": PEAK_TFLOPS,
           "populations": {str(N): population(N, a.reps, a.calls, a.max_steps) for N in a.populations}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
