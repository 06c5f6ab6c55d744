"""The Deep-Q image racers: okenv_qcnn_act per call at 1024 and 4096 agents, reference shape (96 x 96 frames,
k 8/4/3, stride 4/2/1, padding 2/1/1, 32/64/64 channels, 512 hidden, 5 actions), each of its two kernels alone and the head with 32
agents a workgroup instead of the act's 16 (the tiling that was measured and not chosen), against dqn_cnn.QCNN behind dqn_cnn.gray with the same weights on the same frames -- launched
eagerly and as one replayed torch.cuda.graph; the push beside a step launch; the batch gather at B = 256 and 4096; and one whole
iteration of dqn_cnn.run_episode's loop (act, step, camera, push) with either policy.

    python tools/qcnn_bench.py [--out profiles/qcnn/qcnn_bench.json] [--reps 5] [--calls 10]

Every figure is the time between two HIP events on the environment's stream around --calls calls, per call, median / min / max of
--reps repetitions after one warm-up region.  Nothing steps between the act's calls, so every call does the same work.  The floors
printed beside the measurements are derived from the shape, not measured: the FLOP of a frame at the f32 matrix peak, and fc1's
weights read once per workgroup of the head (what its L2 traffic is)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd import dqn_cnn  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

FRAME = 96
PEAK_TFLOPS = 157.3
CAPACITY = 16384


def flop_per_frame(cfg):
    total, cin = 0.0, 1
    for k, c, side in zip(cfg.kernel, cfg.channels, capi.qcnn_sides(cfg)):
        total += 2.0 * side * side * c * cin * k * k
        cin = c
    F = cfg.channels[2] * capi.qcnn_sides(cfg)[2] ** 2
    return total + 2.0 * F * cfg.hidden + 2.0 * cfg.hidden * cfg.num_actions


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
    model = dqn_cnn.QCNN(FRAME).to(venv.device).eval()
    sd = model.state_dict()
    cfg = dqn_cnn.qcnn_config_from_state_dict(sd, image_size=FRAME, mode="eps_greedy", epsilon=0.5, seed=1)
    venv.enable_image_dqn(cfg, dqn_cnn.qcnn_params_from_state_dict(sd, image_size=FRAME), capacity=CAPACITY)
    venv.reset()
    venv.step(n_steps=8)
    frames = venv.camera()
    A = cfg.num_actions
    rec = {"q": torch.empty((N, A), device=venv.device), "action": torch.empty(N, dtype=torch.int64, device=venv.device),
           "value": torch.empty(N, device=venv.device), "alive": torch.empty(N, dtype=torch.uint8, device=venv.device)}
    out = {"qcnn_act_us": timed_us(lambda: venv.image_dqn_act(frames, rec), reps, calls)}
    for name, stage in (("conv_kernel_us", capi.QCNN_STAGE_CONV), ("head_kernel_us", capi.QCNN_STAGE_HEAD),
                        ("head_kernel_32_agents_us", capi.QCNN_STAGE_HEAD_32)):
        out[name] = timed_us(lambda: venv.env.qcnn_act(frames, None, stages=stage), reps, calls)
    out["head_agents_per_workgroup"] = capi.QCNN_AGENTS
    venv.image_dqn_act(frames, rec)
    result = [None]

    def torch_forward():
        with torch.no_grad():
            result[0] = model(planes)

    def torch_with_gray():
        with torch.no_grad():
            result[0] = model(dqn_cnn.gray(frames))

    with torch.no_grad():
        planes = dqn_cnn.gray(frames).unsqueeze(1).contiguous()
    out["torch_eager_us"] = timed_us(torch_forward, reps, calls)
    out["torch_eager_with_gray_us"] = timed_us(torch_with_gray, reps, calls)
    out["max_abs_difference"] = float((rec["q"] - result[0]).abs().max())
    out["torch_graph_us"] = timed_us(graphed(venv, torch_forward).replay, reps, calls)
    out["torch_graph_with_gray_us"] = timed_us(graphed(venv, torch_with_gray).replay, reps, calls)

    # the push beside a step launch, and the gather
    nxt = torch.empty_like(frames)
    venv.camera(out=nxt)
    out["push_us"] = timed_us(lambda: venv.image_dqn_push(rec, frames, nxt), reps, calls)
    out["step_us"] = timed_us(venv.step, reps, calls)
    out["camera_us"] = timed_us(lambda: venv.camera(out=nxt), reps, calls)
    for B in (256, 4096):
        batch = venv.image_dqn_batch(B)
        for mode in ("sequential", "uniform"):
            out["batch_%s_%d_us" % (mode, B)] = timed_us(lambda: venv.image_dqn_batch(B, mode, 3, out=batch), reps, calls)
    out["batch_bytes_4096"] = 2 * 2 * 4096 * FRAME * FRAME * 4  # both planes read and written

    # one iteration of run_episode's loop both ways, launched one by one and as a replayed graph of one iteration
    table = torch.tensor(capi.QCNN_ACTION_MAP, dtype=torch.float32, device=venv.device)

    def device_iteration():
        venv.image_dqn_act(frames, rec)
        venv.step()
        venv.camera(out=nxt)
        venv.image_dqn_push(rec, frames, nxt)

    def torch_iteration():
        with torch.no_grad():
            q = model(dqn_cnn.gray(frames))
            explore = torch.rand(N, device=venv.device) < 0.5
            action = torch.where(explore, torch.randint(0, A, (N,), device=venv.device), q.argmax(1))
            rec["action"].copy_(action)
            rec["alive"].copy_(~venv.done)
            venv.throttle.copy_(table[action, 0])
            venv.steering.copy_(table[action, 1])
        venv.step()
        venv.camera(out=nxt)
        venv.image_dqn_push(rec, frames, nxt)

    for name, fn in (("loop_iteration_device_policy", device_iteration), ("loop_iteration_torch_policy", torch_iteration)):
        out[name + "_eager_us"] = timed_us(fn, reps, calls)
        try:
            out[name + "_graph_us"] = timed_us(venv.capture(fn, warmup=1).replay, reps, calls)
        except RuntimeError as e:  # (torch's random draws inside a capture: reported, not hidden)
            out[name + "_graph_us"] = "capture failed: %s" % str(e).splitlines()[0]
            venv.use_stream(torch.cuda.current_stream(venv.device))
    med, flop = out["qcnn_act_us"]["median"], flop_per_frame(cfg)
    fc1_bytes = 4.0 * cfg.hidden * cfg.channels[2] * capi.qcnn_sides(cfg)[2] ** 2
    out["qcnn_act_tflops"] = flop * N / (med * 1e-6) / 1e12
    out["matrix_peak_floor_us"] = flop * N / (PEAK_TFLOPS * 1e12) * 1e6
    out["fraction_of_matrix_peak"] = out["matrix_peak_floor_us"] / med
    out["head_fc1_l2_bytes"] = {str(t): fc1_bytes * -(-N // t) for t in (16, 32)}
    out["torch_eager_over_qcnn_act"] = out["torch_eager_with_gray_us"]["median"] / med
    out["torch_graph_over_qcnn_act"] = out["torch_graph_with_gray_us"]["median"] / med
    venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "qcnn", "qcnn_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    cfg = capi.qcnn_config(image_size=FRAME)
    res = {"device": torch.cuda.get_device_name(0), "track": "Austin",
           "network": "grey -> conv %s, k %s, stride %s, padding %s -> flatten -> %d -> %d" % (
               tuple(cfg.channels), tuple(cfg.kernel), tuple(cfg.stride), tuple(cfg.padding), cfg.hidden, cfg.num_actions),
           "frame": FRAME, "plan": capi.qcnn_plan(cfg), "lds_bytes": capi.qcnn_lds_bytes(cfg), "reps": a.reps, "calls_per_region": a.calls,
           "flop_per_frame": flop_per_frame(cfg), "matrix_peak_tflops": PEAK_TFLOPS, "num_params": capi.qcnn_num_params(cfg),
           "weights_read_once_bytes": 4 * capi.qcnn_num_params(cfg), "ring_capacity": CAPACITY,
           "populations": {str(N): population(N, a.reps, a.calls) for N in (1024, 4096)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
