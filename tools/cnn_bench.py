"""The behavioural-cloning image policy: okenv_cnn_act per call at 1024 and 4096 agents, reference shape
(96 x 96 frames, k 8/4/3, stride 4/2/1, 32/64/64 channels, 256 hidden), and each of its two kernels alone, against the PyTorch module
with the same weights on the same frames -- with and without frames_to_input in front of it, launched eagerly and as one replayed
torch.cuda.graph -- one whole iteration of bc.drive's loop (step, camera, forward, action) both ways, and a step launch beside them.

    python tools/cnn_bench.py [--out profiles/cnn/cnn_bench.json] [--reps 5] [--calls 10]

Every figure is the time between two HIP events on the environment's stream around --calls calls, per call, median / min / max of
--reps repetitions after one warm-up region.  Nothing steps between the act's calls, so every call does the same work.
19.9 MFLOP per frame: 81.5 GFLOP per call at 4096 agents, 0.52 ms at the f32 matrix peak (157.3 TFLOP/s) -- derived, not measured."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd import bc  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

FRAME = 96
PEAK_TFLOPS = 157.3


def flop_per_frame(cfg):
    total, cin = 0.0, 3
    for k, c, side in zip(cfg.kernel, cfg.channels, capi.cnn_sides(cfg)):
        total += 2.0 * side * side * c * cin * k * k
        cin = c
    F = cfg.channels[2] * capi.cnn_sides(cfg)[2] ** 2
    return total + 2.0 * F * cfg.hidden + 2.0 * cfg.hidden


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


def graphed(venv, fn):
    """fn captured once on a side stream after one eager call there (the convolutions choose their kernels on the first call)."""
    side = torch.cuda.Stream(device=venv.device)
    side.wait_stream(torch.cuda.current_stream(venv.device))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(venv.device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    torch.cuda.synchronize()
    return graph


def population(N, reps, calls):
    venv = VectorEnvironment("Austin", N, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=0)
    venv.enable_camera(width=FRAME, height=FRAME, fmt="rgba")
    torch.manual_seed(3)
    model = bc.PolicyCNN(FRAME).to(venv.device).eval()
    sd = model.state_dict()
    cfg = bc.cnn_config_from_state_dict(sd, image_size=FRAME)
    venv.enable_image_policy(cfg, bc.cnn_params_from_state_dict(sd, image_size=FRAME))
    venv.reset()
    venv.step(n_steps=8)
    frames = venv.camera()
    got = torch.empty(N, device=venv.device)
    out = {"cnn_act_us": timed_us(lambda: venv.image_act(frames), reps, calls)}
    for name, stage in (("conv_kernel_us", capi.CNN_STAGE_CONV), ("head_kernel_us", capi.CNN_STAGE_HEAD)):
        out[name] = timed_us(lambda: venv.env.cnn_act(frames, None, stages=stage), reps, calls)
    venv.image_act(frames, {"out": got})
    result = [None]

    def torch_forward():
        with torch.no_grad():
            result[0] = model(image)

    def torch_with_input():
        with torch.no_grad():
            result[0] = model(bc.frames_to_input(frames))

    with torch.no_grad():
        image = bc.frames_to_input(frames)
    out["torch_eager_us"] = timed_us(torch_forward, reps, calls)
    out["torch_eager_with_frames_to_input_us"] = timed_us(torch_with_input, reps, calls)
    out["max_abs_difference"] = float((got - result[0][:, 0]).abs().max())
    out["torch_graph_us"] = timed_us(graphed(venv, torch_forward).replay, reps, calls)
    out["torch_graph_with_frames_to_input_us"] = timed_us(graphed(venv, torch_with_input).replay, reps, calls)

    # one iteration of bc.drive's loop both ways, launched one by one and as a replayed graph of one iteration; a step alone
    frame = torch.empty_like(frames)

    def device_iteration():
        venv.step()
        venv.camera(out=frame)
        venv.image_act(frame)

    def torch_iteration():
        venv.step()
        venv.camera(out=frame)
        with torch.no_grad():
            o = model(bc.frames_to_input(frame))[:, 0]
        venv.throttle.fill_(bc.THROTTLE)
        torch.mul(o, bc.STEER_SCALE, out=venv.steering)

    for name, fn in (("drive_iteration_device_policy", device_iteration), ("drive_iteration_torch_policy", torch_iteration)):
        out[name + "_eager_us"] = timed_us(fn, reps, calls)
        out[name + "_graph_us"] = timed_us(venv.capture(fn, warmup=1).replay, reps, calls)
    out["step_us"] = timed_us(venv.step, reps, calls)
    out["camera_us"] = timed_us(lambda: venv.camera(out=frame), reps, calls)
    med, flop = out["cnn_act_us"]["median"], flop_per_frame(cfg)
    out["cnn_act_tflops"] = flop * N / (med * 1e-6) / 1e12
    out["matrix_peak_floor_us"] = flop * N / (PEAK_TFLOPS * 1e12) * 1e6
    out["fraction_of_matrix_peak"] = out["matrix_peak_floor_us"] / med
    out["torch_eager_over_cnn_act"] = out["torch_eager_with_frames_to_input_us"]["median"] / med
    out["torch_graph_over_cnn_act"] = out["torch_graph_with_frames_to_input_us"]["median"] / med
    venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "cnn", "cnn_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    cfg = capi.cnn_config(image_size=FRAME)
    res = {"device": torch.cuda.get_device_name(0), "track": "Austin",
           "network": "conv %s, k %s, stride %s -> flatten -> %d -> 1" % (tuple(cfg.channels), tuple(cfg.kernel), tuple(cfg.stride), cfg.hidden),
           "frame": FRAME, "plan": capi.cnn_plan(cfg), "lds_bytes": capi.cnn_lds_bytes(cfg), "reps": a.reps, "calls_per_region": a.calls,
           "flop_per_frame": flop_per_frame(cfg), "matrix_peak_tflops": PEAK_TFLOPS,
           "populations": {str(N): population(N, a.reps, a.calls) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
