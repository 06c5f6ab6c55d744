"""The behavioural-cloning driver of BehavioralCloning/ on the device environment: the network (env_train_bc.py: PolicyCNN) as a PyTorch
module for training, the hand-over of its weights to the device act (okenv_cnn_*) and the driving loop of
main.cpp for N agents.

Training stays in PyTorch.  The forward, once per environment step, runs in PyTorch or, handed over, as the device act
(drive(policy="device")).
"""
import torch
from torch import nn

from . import _capi as capi
from .flow import frames_to_input
from .rollout import _Chunk, _run_episode

THROTTLE, STEER_SCALE = 100.0, 10.0  # main.cpp: the constant throttle and the steering per unit of the output
KEYS = ("encoder.0.weight", "encoder.0.bias", "encoder.2.weight", "encoder.2.bias", "encoder.4.weight", "encoder.4.bias",
        "steering_head.0.weight", "steering_head.0.bias", "steering_head.2.weight", "steering_head.2.bias")


class PolicyCNN(nn.Module):
    """The reference's policy and its parameter names: three valid convolutions with ReLU, the flatten, a hidden layer with ReLU,
    one output and its tanh.  The flatten's width follows from image_size."""

    def __init__(self, image_size=96):
        super().__init__()
        self.image_size = int(image_size)
        self.encoder = nn.Sequential(nn.Conv2d(3, 32, kernel_size=8, stride=4), nn.ReLU(), nn.Conv2d(32, 64, kernel_size=4, stride=2), nn.ReLU(),
                                     nn.Conv2d(64, 64, kernel_size=3, stride=1), nn.ReLU(), nn.Flatten())
        side = capi.cnn_sides(capi.cnn_config(image_size=image_size))[2]
        assert side >= 1, "image_size %d is too small for the three convolutions" % image_size
        self.steering_head = nn.Sequential(nn.Linear(64 * side * side, 256), nn.ReLU(), nn.Linear(256, 1))

    def forward(self, image):
        return torch.tanh(self.steering_head(self.encoder(image)))


def _tensors(sd):
    return [sd[k] for k in KEYS]


def cnn_config_from_state_dict(sd, image_size=96, stride=(4, 2, 1), throttle=THROTTLE, steer_scale=STEER_SCALE):
    """The capi.cnn_config of the shape a state dict of the policy has, for frames of image_size (the strides are not in a state
    dict: the reference's by default)."""
    t = _tensors(sd)
    return capi.cnn_config(image_size=image_size, kernel=[w.shape[2] for w in t[0:6:2]], stride=stride, channels=[w.shape[0] for w in t[0:6:2]],
                           hidden=t[6].shape[0], throttle=throttle, steer_scale=steer_scale)


def cnn_params_from_state_dict(sd, image_size=96, stride=(4, 2, 1), dtype=torch.float32):
    """The flat parameter vector of okenv_cnn_set_params: the pieces of capi.cnn_layout in order."""
    cfg = cnn_config_from_state_dict(sd, image_size, stride)
    pieces = []
    for t, (name, _, shape) in zip(_tensors(sd), capi.cnn_layout(cfg)):
        assert tuple(t.shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape))
        pieces.append(t.detach().to(dtype=dtype).reshape(-1))
    return torch.cat(pieces).contiguous()


def train(model, frames, actions, epochs=1, batch=256, lr=3e-4, seed=0, steer_scale=STEER_SCALE):
    """The reference's recipe (env_train_bc.py) on device tensors: frames [M, S, S, 4] uint8, actions [M, 2] (throttle, steering);
    MSE of the tanh output against clamp(steering / steer_scale, -1, 1), Adam.  Returns the mean loss of every epoch."""
    target = (actions[:, 1:2] / steer_scale).clamp(-1.0, 1.0)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    gen = torch.Generator(device=frames.device).manual_seed(seed)
    M, losses = frames.shape[0], []
    model.train()
    for _ in range(epochs):
        order = torch.randperm(M, device=frames.device, generator=gen)
        total = torch.zeros((), device=frames.device)
        for at in range(0, M, batch):
            idx = order[at:at + batch]
            loss = nn.functional.mse_loss(model(frames_to_input(frames[idx])), target[idx])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += loss.detach() * idx.numel()
        losses.append(float(total) / M)
    model.eval()
    return losses


def drive(venv, model, steps, graph_chunk=0, policy="torch", throttle=THROTTLE, steer_scale=STEER_SCALE):
    """The loop of main.cpp for every agent: `step`, the agents' frames (venv.camera()), the forward, the action (the constant
    throttle, steer_scale times the output), `steps` times; the environment's auto-reset stands in for resetAgent (without it the
    loop ends once nobody is alive).  policy="torch": `model` in PyTorch behind frames_to_input; policy="device": the one given to
    venv.enable_image_policy, no PyTorch op in the iteration (model is not used and may be None) -- the camera must render at the
    policy's image_size, the device path does not resize.  graph_chunk = K > 0 replays a HIP graph of K iterations.  Returns the
    steps taken."""
    assert policy in ("torch", "device"), 'policy is "torch" or "device"'
    assert hasattr(venv, "camera_shape") and len(venv.camera_shape) == 4, 'call venv.enable_camera(..., fmt="rgba") first'
    frame = torch.empty(venv.camera_shape, dtype=torch.uint8, device=venv.device)
    if policy == "device":
        assert getattr(venv, "cnn_config", None) is not None, "call venv.enable_image_policy(config, params) first"
        S = venv.cnn_config.image_size
        if tuple(venv.camera_shape[1:3]) != (S, S):
            raise ValueError('drive(policy="device") needs the camera at the policy\'s size: venv.enable_camera(width=%d, height=%d, fmt="rgba"); '
                             "it renders %dx%d (the device policy does not resize)" % (S, S, venv.camera_shape[2], venv.camera_shape[1]))
        graphs = venv._cnn_graphs

        def iteration(_):
            venv.step()
            venv.camera(out=frame)
            venv.image_act(frame)

        def build():
            return iteration, (frame,)

        key = ("device",)
    else:
        S = model.image_size
        if tuple(venv.camera_shape[1:3]) != (S, S):
            raise ValueError("drive needs the camera at the policy's size %dx%d; it renders %dx%d" % (S, S, venv.camera_shape[2], venv.camera_shape[1]))
        if not hasattr(venv, "_bc_graphs"):
            venv._bc_graphs = {}
        graphs = venv._bc_graphs

        def iteration(_):
            venv.step()
            venv.camera(out=frame)
            with torch.no_grad():
                out = model(frames_to_input(frame))[:, 0]
            venv.throttle.fill_(throttle)
            torch.mul(out, steer_scale, out=venv.steering)

        def build():
            venv.camera(out=frame)
            with torch.no_grad():  # the convolutions choose their kernels on the first call of a shape: not inside a capture
                model(frames_to_input(frame))
            return iteration, (frame, model)

        key = (id(model), float(throttle), float(steer_scale))

    K = int(graph_chunk)
    chunk = None
    if K > 0:  # (the act draws nothing: there is no draw-offset word to hand over)
        chunk = _Chunk(K=K, graphs=graphs, key=(K,) + key, set_draw_offset=lambda word: None, build=build, after_replay=None)
    _, taken = _run_episode(venv, iteration, int(steps), 8, chunk)
    return taken


__all__ = ["PolicyCNN", "cnn_config_from_state_dict", "cnn_params_from_state_dict", "train", "drive", "frames_to_input", "THROTTLE", "STEER_SCALE"]
