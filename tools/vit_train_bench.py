"""DinoControl's training on the device: one epoch of the head's minibatch loop over 4096 cached embeddings at
the reference head shape (384-128-64-1), batch 64 (dino.train's default) and 512 (the reference's), okenv_vit_head_update against
dino.train's own PyTorch loop (eager fp32, the same embeddings and order); and okenv_vit_embed against model.embed behind
frames_to_input at 64 frames of the reference backbone.

    python tools/vit_train_bench.py [--out profiles/vit/vit_train_bench.json] [--reps 5] [--epochs 10]

Every figure is the time between two HIP events on the environment's stream around --epochs epochs (or --embed-calls embeds), per
minibatch, median / min / max of --reps repetitions after one warm-up region; ten epochs make the shortest region 80 minibatches.
The device loop is two launches per minibatch: the forward kernel's share is measured as okenv_vit_head_eval's epochs (the forward
kernel and the one wave that sums the loss), the gradient + Adam kernel's as the rest."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openkitchen_amd import dino  # noqa: E402
from openkitchen_amd.torch_env import VectorEnvironment  # noqa: E402

M = 4096
HEAD_BACKBONE = dict(image_size=8, patch=8, dim=384, heads=6, depth=1, dim_feedforward=16, head_hidden1=128, head_hidden2=64)  # two tokens: only the head matters


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


def attach(venv, model, heads):
    sd = model.state_dict()
    venv.enable_vit_policy(dino.vit_config_from_state_dict(sd, heads=heads), dino.vit_params_from_state_dict(sd, heads=heads))


def head_loop(reps, epochs):
    venv = VectorEnvironment("Austin", 2, auto_reset=False, seed=0)
    torch.manual_seed(0)
    model = dino.ViT(**HEAD_BACKBONE).to(venv.device).eval()
    attach(venv, model, 6)
    venv.enable_vit_head_learner()
    emb = torch.randn((M, 384), device=venv.device)
    steer = (torch.rand(M, device=venv.device) * 2 - 1) * dino.STEER_SCALE
    label = (steer[:, None] / dino.STEER_SCALE).clamp(-1.0, 1.0)
    order = torch.randperm(M, device=venv.device)
    order32 = order.to(torch.int32)[None, :].repeat(epochs, 1).contiguous()
    opt = torch.optim.Adam(model.head.parameters(), lr=1e-4)
    out = {}
    for B in (64, 512):
        K = M // B

        def torch_epochs():  # dino.train's minibatch loop
            for _ in range(epochs):
                total = torch.zeros((), device=venv.device)
                for at in range(0, M, B):
                    idx = order[at:at + B]
                    loss = dino.weighted_mse(model.head(emb[idx]), label[idx])
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    opt.step()
                    total += loss.detach() * idx.numel()

        def eval_epochs():
            for _ in range(epochs):
                venv.vit_head_eval(emb, steer, B)

        res = {"minibatches_per_epoch": K, "epochs_per_region": epochs,
               "device_update_us_per_minibatch": timed_us(lambda: venv.vit_head_update(emb, steer, B, epochs, order32), reps, K * epochs),
               "device_forward_us_per_minibatch": timed_us(eval_epochs, reps, K * epochs),
               "torch_eager_fp32_us_per_minibatch": timed_us(torch_epochs, reps, K * epochs)}
        res["device_grad_adam_us_per_minibatch"] = res["device_update_us_per_minibatch"]["median"] - res["device_forward_us_per_minibatch"]["median"]
        res["torch_over_device"] = res["torch_eager_fp32_us_per_minibatch"]["median"] / res["device_update_us_per_minibatch"]["median"]
        out[str(B)] = res
    venv.close()
    return out


def embed(reps, calls, frames_n=64):
    venv = VectorEnvironment("Austin", frames_n, auto_reset=False, seed=0)  # (a pass holds at most the population: one pass of 64 here)
    torch.manual_seed(0)
    model = dino.ViT().to(venv.device).eval()
    attach(venv, model, 6)
    frames = torch.randint(0, 256, (frames_n, 224, 224, 4), dtype=torch.uint8, device=venv.device)
    got = torch.empty((frames_n, 384), device=venv.device)

    def device_embed():
        for _ in range(calls):
            venv.vit_embed(frames, out=got)

    def torch_embed():
        with torch.no_grad():
            for _ in range(calls):
                model.embed(dino.frames_to_input(frames))

    res = {"frames": frames_n, "vit_embed_us": timed_us(device_embed, reps, calls),
           "torch_eager_fp32_us": timed_us(torch_embed, reps, calls)}
    with torch.no_grad():
        res["max_abs_difference"] = float((got - model.embed(dino.frames_to_input(frames))).abs().max())
    res["device_over_torch"] = res["vit_embed_us"]["median"] / res["torch_eager_fp32_us"]["median"]
    venv.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "vit", "vit_train_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--embed-calls", type=int, default=1)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "samples": M, "head": "384-128-64-1", "reps": a.reps, "head_loop": head_loop(a.reps, a.epochs),
           "embed": embed(a.reps, a.embed_calls)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
