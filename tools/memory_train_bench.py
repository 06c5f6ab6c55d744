"""The memory's training on the device: one epoch of okenv_memory_update against worldmodel.train_memory's
PyTorch minibatch loop (eager fp32: the forward, mse_loss, backward, clip_grad_norm_, AdamW and the cosine scheduler's step) on the same
windows and order, at the reference shape (Z 32, H 512, L 3, S 5, B 256) and at the example's default memory (H 64).

    python tools/memory_train_bench.py [--out profiles/memory/memory_train_bench.json] [--reps 5] [--kernel-stats FILE.csv]

Every figure is the time between two HIP events on the environment's stream around one epoch of 4 minibatches (1024 windows), per
minibatch, median / min / max of --reps repetitions after one warm-up epoch.  The forward's share is measured as okenv_memory_eval's
epoch (the gather, the forward's launches, the seeds and the loss).  worldmodel.train_memory is the same code in the parent commit,
so its figure here is the parent's.  --kernel-stats merges a kernel trace's per-kernel statistics (a CSV with Name, Calls,
TotalDurationNs columns, taken in a run of its own) into the result under "kernels".

The floors named beside the figures are DERIVED, not measured: at the reference shape a position costs 3 x 512 x (34 + 512) +
2 x 3 x 512 x 1024 + 32 x 512 = about 4.0 M multiply-adds forward and about twice that backward, 24 MFLOP forward and backward
together, 31 GFLOP for a minibatch of 1280 positions: about 0.2 ms at the 157 TFLOP/s f32 matrix peak the README uses; the parameters,
the gradient and the two moments are 5.6 M floats each, about 0.1 GB read and written per step: about 0.02 ms at 5 TB/s."""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import _capi as capi  # noqa: E402
from openkitchen_amd import worldmodel as wm  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

SHAPES = {"reference": dict(Z=32, H=512, L=3, S=5, B=256), "example": dict(Z=32, H=64, L=3, S=5, B=256)}
MINIBATCHES = 4


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


def timed_us(fn, reps, per):
    fn()
    return stats([1e3 * event_ms(fn) / per for _ in range(reps)])


def floors(Z, H, L, S, B):
    forward = 3 * H * (Z + 2 + H) + (L - 1) * 3 * H * 2 * H + Z * H  # multiply-adds of one position
    params = forward + L * 6 * H + Z
    return {"derived_not_measured": True, "multiply_adds_per_position_forward": forward, "gflop_per_minibatch": 2 * 3 * forward * B * S / 1e9,
            "ms_at_157_tflops_f32_matrix_peak": 2 * 3 * forward * B * S / 157e12 * 1e3, "parameter_and_moment_gigabytes_per_step": 7 * 4 * params / 1e9}


def one_shape(name, reps):
    Z, H, L, S, B = (SHAPES[name][k] for k in "ZHLSB")
    venv = VectorEnvironment("Austin", 2, auto_reset=False, seed=0)
    dev = venv.device
    torch.manual_seed(0)
    T, N = S + MINIBATCHES, B  # every agent alive: MINIBATCHES * B windows
    latents, actions = torch.randn(T, N, Z, device=dev), torch.randn(T, N, 2, device=dev)
    alive = torch.ones(T, N, dtype=torch.bool, device=dev)
    model = wm.GRUDynamics(Z, H, L).to(dev)
    venv.env.world_create(capi.world_config(image_size=16, channels=(16, 16, 16, 16), latent=Z, hidden=2))
    _, stats_, _ = wm.train_memory_device(venv, model, latents, actions, alive, epochs=1, batch=B, seq_len=S)  # attaches the memory and the learner
    start = wm.memory_window_starts(alive, S)
    M = int(start.numel())
    assert M == MINIBATCHES * B
    order = torch.randperm(M, device=dev)
    order32 = order.to(torch.int32)[None].contiguous()
    schedule = np.full(MINIBATCHES, 1e-3, np.float32)
    # the PyTorch loop on the same windows
    z, a = wm.memory_windows(latents, actions, alive, S)
    st = {k: v.to(dev) for k, v in stats_.items()}
    zn, an = (z - st["z_mean"]) / st["z_std"], (a - st["a_mean"]) / st["a_std"]
    x, y = torch.cat([zn[:, :-1], an[:, :-1]], dim=2), zn[:, 1:]
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=10 ** 6)
    model.train()

    def torch_epoch():  # worldmodel.train_memory's minibatch loop
        total = torch.zeros((), device=dev)
        for at in range(0, M, B):
            rows = order[at:at + B]
            loss = nn.functional.mse_loss(model(x[rows])[0], y[rows])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            sched.step()
            total += loss.detach() * rows.numel()

    res = {"shape": SHAPES[name], "windows": M, "minibatches_per_epoch": MINIBATCHES, "positions_per_minibatch": B * S,
           "device_update_us_per_minibatch": timed_us(lambda: venv.memory_update(latents, actions, start, B, stride=N, order=order32, lr_schedule=schedule),
                                                      reps, MINIBATCHES),
           "device_forward_us_per_minibatch": timed_us(lambda: venv.memory_eval(latents, actions, start, B, stride=N), reps, MINIBATCHES),
           "torch_eager_fp32_us_per_minibatch": timed_us(torch_epoch, reps, MINIBATCHES),
           "parent_commit_loop": "worldmodel.train_memory is unchanged: torch_eager_fp32_us_per_minibatch is the parent's figure",
           "floors": floors(Z, H, L, S, B)}
    res["device_backward_and_step_us_per_minibatch"] = res["device_update_us_per_minibatch"]["median"] - res["device_forward_us_per_minibatch"]["median"]
    res["torch_over_device"] = res["torch_eager_fp32_us_per_minibatch"]["median"] / res["device_update_us_per_minibatch"]["median"]
    venv.close()
    return res


def kernel_stats(path):
    """Name, calls and total microseconds of the learner's kernels from a kernel trace's statistics."""
    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "okMemTrain" in row.get("Name", "") or "okMemoryPack" in row.get("Name", ""):
                out.append({"kernel": row["Name"].split("(")[0], "calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3,
                            "percent_of_all_kernels": float(row.get("Percentage", "nan"))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "memory", "memory_train_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="reference,example")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    for name in a.shapes.split(","):
        res[name] = one_shape(name, a.reps)
    if a.kernel_stats:
        res["kernels"] = {"source": "a kernel trace of this tool at --shapes reference --reps 1, a run of its own", "rows": kernel_stats(a.kernel_stats)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
