"""The flow-matching driver: okenv_flow_act per call at 1024 and 4096 agents, reference shape (C 128, H 256,
32 Euler steps), against flow.sample -- the PyTorch loop over the trunk with the same weights, from the same noise and condition --
launched eagerly and as one replayed torch.cuda.graph.  The conv encoder is in neither; one forward of it and a step launch are timed
beside them, for scale.

    python tools/flow_bench.py [--out profiles/flow/flow_bench.json] [--reps 5] [--calls 20]

Every figure is the time between two HIP events on the environment's stream around --calls calls, per call, median / min / max of
--reps repetitions after one warm-up region.  Nothing steps between the calls, so every call does the same work.  4.3 MFLOP per
agent: 17.6 GFLOP per act at 4096 agents, 0.11 ms at the f32 matrix peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd import flow  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

C, H, S, FRAME = 128, 256, 32, 128
FLOP_PER_AGENT = 2.0 * (C * H + S * (3 * H + H * H + 2 * H))


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
    venv = VectorEnvironment("Austin", N, auto_reset=True, randomize_lane=True, randomize_heading=True, seed=0)
    venv.enable_camera(width=FRAME, height=FRAME, fmt="rgba")
    torch.manual_seed(0)
    model = flow.ConditionalFlowMatchingPolicy(bev_dim=C, hidden_dim=H).to(venv.device).eval()
    sd = model.action_flow_trunk.state_dict()
    venv.enable_flow_policy(flow.flow_config_from_state_dict(sd, steps=S), flow.flow_params_from_state_dict(sd))
    venv.reset()
    venv.step(n_steps=8)
    frames = venv.camera()
    with torch.no_grad():
        image = flow.frames_to_input(frames)
        cond = model.bev_encoder(image).contiguous()
    rec = {"x0": torch.empty((N, 2), device=venv.device), "x": torch.empty((N, 2), device=venv.device),
           "action": torch.empty((N, 2), device=venv.device), "alive": torch.empty(N, dtype=torch.uint8, device=venv.device)}
    out = {"flow_act_us": timed_us(lambda: venv.flow_act(cond), reps, calls),
           "flow_act_recording_us": timed_us(lambda: venv.flow_act(cond, rec), reps, calls)}
    # the PyTorch sampler on the trunk alone, from the noise the device drew
    venv.flow_act(cond, rec)
    torch.cuda.synchronize()
    x0 = rec["x0"].clone()
    sampled = [None]

    def torch_sample():
        sampled[0] = flow.sample(model, cond, x0, S)

    out["torch_eager_fp32_us"] = timed_us(torch_sample, reps, calls)
    out["max_abs_sample_difference"] = float((rec["x"] - sampled[0]).abs().max())
    side = torch.cuda.Stream(device=venv.device)
    side.wait_stream(torch.cuda.current_stream(venv.device))
    with torch.cuda.stream(side):
        torch_sample()
    torch.cuda.current_stream(venv.device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        torch_sample()
    torch.cuda.synchronize()
    out["torch_graph_fp32_us"] = timed_us(graph.replay, reps, calls)
    out["max_abs_sample_difference_graph"] = float((rec["x"] - sampled[0]).abs().max())

    def encoder():
        with torch.no_grad():
            model.bev_encoder(image)

    out["encoder_forward_us"] = timed_us(encoder, reps, calls)
    out["step_us"] = timed_us(venv.step, reps, calls)
    out["flow_act_tflops"] = FLOP_PER_AGENT * N / (out["flow_act_us"]["median"] * 1e-6) / 1e12
    out["torch_graph_over_flow_act"] = out["torch_graph_fp32_us"]["median"] / out["flow_act_us"]["median"]
    out["torch_eager_over_flow_act"] = out["torch_eager_fp32_us"]["median"] / out["flow_act_us"]["median"]
    venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "flow", "flow_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    cfg = capi.flow_config(cond_dim=C, hidden=H, steps=S)
    res = {"device": torch.cuda.get_device_name(0), "track": "Austin", "network": "trunk %d -> %d -> %d -> 2, %d Euler steps" % (3 + C, H, H, S),
           "agents_per_workgroup": capi.FLOW_AGENTS, "lds_bytes": capi.flow_lds_bytes(cfg), "encoder_frame": FRAME, "reps": a.reps,
           "calls_per_region": a.calls, "flop_per_agent": FLOP_PER_AGENT,
           "populations": {str(N): population(N, a.reps, a.calls) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
