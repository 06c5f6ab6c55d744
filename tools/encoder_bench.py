"""The flow driver's image encoder: okenv_bev_encode per call at 1024 and 4096 agents, reference shape
(128 x 128 frames, k 5/3/3, 32/64/128 channels, 128 wide), and each of its three kernels alone, against the PyTorch module with the
same weights on the same frames -- with and without frames_to_input in front of it, launched eagerly and as one replayed
torch.cuda.graph -- and one whole iteration of flow.drive's loop (step, camera, encoder, flow_act) with each encoder.

    python tools/encoder_bench.py [--out profiles/bev_encoder/encoder_bench.json] [--reps 5] [--calls 10]

Every figure is the time between two HIP events on the environment's stream around --calls calls, per call, median / min / max of
--reps repetitions after one warm-up region.  Nothing steps between the encoder's calls, so every call does the same work.
95.2 MFLOP per frame: 390 GFLOP per call at 4096 agents, 2.5 ms at the f32 matrix peak (157 TFLOP/s)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd import flow  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

FRAME, KERNEL, CHANNELS, EMBED = 128, (5, 3, 3), (32, 64, 128), 128
PEAK_TFLOPS = 157.0


def flop_per_frame():
    total, cin, side = 0.0, 3, FRAME
    for k, c in zip(KERNEL, CHANNELS):
        side //= 2
        total += 2.0 * side * side * c * cin * k * k
        cin = c
    return total + 2.0 * CHANNELS[2] * EMBED


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
    torch.manual_seed(0)
    model = flow.ConditionalFlowMatchingPolicy().to(venv.device).eval()
    sd = model.state_dict()
    venv.enable_flow_policy(flow.flow_config_from_state_dict(sd, steps=32), flow.flow_params_from_state_dict(sd))
    venv.enable_bev_encoder(flow.bev_config_from_state_dict(sd, image_size=FRAME), flow.bev_params_from_state_dict(sd))
    venv.reset()
    venv.step(n_steps=8)
    frames = venv.camera()
    cond = torch.empty((N, EMBED), device=venv.device)
    out = {"bev_encode_us": timed_us(lambda: venv.bev_encode(frames, out=cond), reps, calls)}
    for name, stage in (("front_kernel_us", capi.BEV_STAGE_FRONT), ("back_kernel_us", capi.BEV_STAGE_BACK), ("head_kernel_us", capi.BEV_STAGE_HEAD)):
        out[name] = timed_us(lambda: venv.env.bev_encode(frames, cond, stages=stage), reps, calls)
    venv.bev_encode(frames, out=cond)
    result = [None]

    def torch_encoder():
        with torch.no_grad():
            result[0] = model.bev_encoder(image)

    def torch_with_input():
        with torch.no_grad():
            result[0] = model.bev_encoder(flow.frames_to_input(frames))

    with torch.no_grad():
        image = flow.frames_to_input(frames)
    out["torch_eager_us"] = timed_us(torch_encoder, reps, calls)
    out["torch_eager_with_frames_to_input_us"] = timed_us(torch_with_input, reps, calls)
    out["max_abs_difference"] = float((cond - result[0]).abs().max())
    out["torch_graph_us"] = timed_us(graphed(venv, torch_encoder).replay, reps, calls)
    out["torch_graph_with_frames_to_input_us"] = timed_us(graphed(venv, torch_with_input).replay, reps, calls)

    # one iteration of flow.drive's loop with each encoder, launched one by one and as a replayed graph of one iteration
    frame = torch.empty_like(frames)

    def device_iteration():
        venv.step()
        venv.camera(out=frame)
        venv.bev_encode(frame, out=cond)
        venv.flow_act(cond)

    def torch_iteration():
        venv.step()
        venv.camera(out=frame)
        with torch.no_grad():
            c = model.bev_encoder(flow.frames_to_input(frame))
        venv.flow_act(c.contiguous())

    for name, fn in (("drive_iteration_device_encoder", device_iteration), ("drive_iteration_torch_encoder", torch_iteration)):
        out[name + "_eager_us"] = timed_us(fn, reps, calls)
        out[name + "_graph_us"] = timed_us(venv.capture(fn, warmup=1).replay, reps, calls)
    med = out["bev_encode_us"]["median"]
    out["bev_encode_tflops"] = flop_per_frame() * N / (med * 1e-6) / 1e12
    out["matrix_peak_floor_us"] = flop_per_frame() * N / (PEAK_TFLOPS * 1e12) * 1e6
    out["torch_eager_over_bev_encode"] = out["torch_eager_with_frames_to_input_us"]["median"] / med
    out["torch_graph_over_bev_encode"] = out["torch_graph_with_frames_to_input_us"]["median"] / med
    venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "bev_encoder", "encoder_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    cfg = capi.bev_config(image_size=FRAME, kernel=KERNEL, channels=CHANNELS, embed_dim=EMBED)
    res = {"device": torch.cuda.get_device_name(0), "track": "Austin", "network": "conv %s, k %s, stride 2 -> pool -> %d" % (CHANNELS, KERNEL, EMBED),
           "frame": FRAME, "tiles": capi.bev_tiles(cfg), "lds_bytes": capi.bev_lds_bytes(cfg), "reps": a.reps, "calls_per_region": a.calls,
           "flop_per_frame": flop_per_frame(), "matrix_peak_tflops": PEAK_TFLOPS,
           "populations": {str(N): population(N, a.reps, a.calls) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
