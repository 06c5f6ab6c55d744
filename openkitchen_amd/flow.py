"""The flow-matching driver of FlowMatching/ on the device environment: the networks (flow_matching_model.py: BEVEncoder,
ActionFlowTrunk, ConditionalFlowMatchingPolicy) as PyTorch modules for training, the hand-over of the trunk's weights to the device
sampler (okenv_flow_*) and the driving loop of main_flow_control.cpp:157-170 for N agents.

Training stays in PyTorch.  The 32 evaluations of the trunk per action run as one HIP kernel; the conv encoder, once per environment
step, runs in PyTorch or, handed over like the trunk, as the device encoder (okenv_bev_*, DESIGN.md section 25: drive(encoder="device")).
"""
import torch
from torch import nn

from . import _capi as capi
from .imitation import denormalize_controls, normalize_controls
from .rollout import _Chunk, _run_episode

ACTION_LO, ACTION_HI = (0.0, -10.0), (100.0, 10.0)  # flow_matching_model.py: ActionNormalizer
TRUNK_KEYS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")
TRUNK_PREFIX = "action_flow_trunk."
ENCODER_KEYS = ("conv.0.weight", "conv.0.bias", "conv.2.weight", "conv.2.bias", "conv.4.weight", "conv.4.bias", "proj.weight", "proj.bias")
ENCODER_PREFIX = "bev_encoder."


class BEVEncoder(nn.Module):
    """The reference's image encoder and its parameter names: three strided convolutions with ReLU, a global average and a
    projection to `embed_dim`."""

    def __init__(self, in_channels=3, embed_dim=128):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channels, 32, kernel_size=5, stride=2, padding=2), nn.ReLU(inplace=True),
                                  nn.Conv2d(32, 64, kernel_size=3, stride=2, padding=1), nn.ReLU(inplace=True),
                                  nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1), nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d(1))
        self.proj = nn.Linear(128, embed_dim)

    def forward(self, image):
        return self.proj(self.conv(image).flatten(1))


class ActionFlowTrunk(nn.Module):
    """The velocity field v(x_t, t, embedding): Linear(2 + 1 + bev_dim, hidden) - ReLU - Linear(hidden, hidden) - ReLU -
    Linear(hidden, 2) on cat([x_t, t, embedding])."""

    def __init__(self, bev_dim=128, hidden_dim=256, action_dim=2):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(action_dim + 1 + bev_dim, hidden_dim), nn.ReLU(inplace=True), nn.Linear(hidden_dim, hidden_dim),
                                 nn.ReLU(inplace=True), nn.Linear(hidden_dim, action_dim))

    def forward(self, x_t, t, bev_embedding):
        return self.net(torch.cat([x_t, t, bev_embedding], dim=1))


class ConditionalFlowMatchingPolicy(nn.Module):
    """Encoder and trunk under the reference's names (a checkpoint's model_state_dict of its train_flow_matching.py loads)."""

    def __init__(self, bev_dim=128, hidden_dim=256, action_dim=2):
        super().__init__()
        self.bev_encoder = BEVEncoder(embed_dim=bev_dim)
        self.action_flow_trunk = ActionFlowTrunk(bev_dim=bev_dim, hidden_dim=hidden_dim, action_dim=action_dim)

    def forward(self, x_t, t, image):
        return self.action_flow_trunk(x_t, t, self.bev_encoder(image))


def _trunk_tensors(sd):
    """The trunk's six tensors from its own state dict or from the whole policy's."""
    prefix = TRUNK_PREFIX if TRUNK_PREFIX + TRUNK_KEYS[0] in sd else ""
    return [sd[prefix + k] for k in TRUNK_KEYS]


def flow_config_from_state_dict(sd, **members):
    """The capi.flow_config of the shape a state dict of the trunk (or of the whole policy) has; members: steps, noise, action_lo,
    action_hi, seed, agent_base."""
    w1, _, w2 = _trunk_tensors(sd)[:3]
    return capi.flow_config(cond_dim=w1.shape[1] - 3, hidden=w2.shape[0], **members)


def flow_params_from_state_dict(sd, dtype=torch.float32):
    """The flat parameter vector of okenv_flow_set_params: the pieces of capi.flow_layout in order."""
    cfg = flow_config_from_state_dict(sd)
    pieces = []
    for t, (name, _, shape) in zip(_trunk_tensors(sd), capi.flow_layout(cfg)):
        assert tuple(t.shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape))
        pieces.append(t.detach().to(dtype=dtype).reshape(-1))
    return torch.cat(pieces).contiguous()


def _encoder_tensors(sd):
    """The encoder's eight tensors from its own state dict or from the whole policy's."""
    prefix = ENCODER_PREFIX if ENCODER_PREFIX + ENCODER_KEYS[0] in sd else ""
    return [sd[prefix + k] for k in ENCODER_KEYS]


def bev_config_from_state_dict(sd, image_size=128):
    """The capi.bev_config of the shape a state dict of the encoder (or of the whole policy) has, for frames of image_size."""
    t = _encoder_tensors(sd)
    return capi.bev_config(image_size=image_size, kernel=[w.shape[2] for w in t[0:6:2]], channels=[w.shape[0] for w in t[0:6:2]],
                           embed_dim=t[6].shape[0])


def bev_params_from_state_dict(sd, dtype=torch.float32):
    """The flat parameter vector of okenv_bev_set_params: the pieces of capi.bev_layout in order."""
    cfg = bev_config_from_state_dict(sd)
    pieces = []
    for t, (name, _, shape) in zip(_encoder_tensors(sd), capi.bev_layout(cfg)):
        assert tuple(t.shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape))
        pieces.append(t.detach().to(dtype=dtype).reshape(-1))
    return torch.cat(pieces).contiguous()


def frames_to_input(frames, image_size=None):
    """venv.camera()'s RGBA frames [N, H, W, 4] uint8 -> the encoder's input [N, 3, S, S] float in 0 .. 1 (main_flow_control.cpp:40-66:
    drop alpha, to float, NCHW, bilinear resize with align_corners=False -- only when the size differs).  The camera's row 0 is already
    the applications' flipped frame."""
    x = frames[..., :3].permute(0, 3, 1, 2).to(torch.float32).div_(255.0)
    if image_size is not None and (x.shape[2] != image_size or x.shape[3] != image_size):
        x = nn.functional.interpolate(x, size=(image_size, image_size), mode="bilinear", align_corners=False)
    return x.contiguous()


def sample(model_or_trunk, cond, x0, steps):
    """The reference's sampler (main_flow_control.cpp:68-85) in PyTorch from a given x0 [N, 2] and the encoder's output cond [N, C]:
    `steps` evaluations of the trunk, x += dt * v, clamped to [-1, 1].  The comparison path of the device act."""
    trunk = getattr(model_or_trunk, "action_flow_trunk", model_or_trunk)
    x, dt = x0, 1.0 / steps
    with torch.no_grad():
        for i in range(steps):
            t = torch.full((x.shape[0], 1), i / steps, dtype=x.dtype, device=x.device)
            x = x + dt * trunk(x, t, cond)
    return x.clamp(-1.0, 1.0)


def train(model, frames, actions, epochs=1, batch=64, lr=1e-3, seed=0, image_size=None, action_lo=ACTION_LO, action_hi=ACTION_HI):
    """The reference's recipe (train_flow_matching.py:16-43) on device tensors: frames [M, H, W, 4] uint8, actions [M, 2]; per batch
    x0 ~ N(0, I), t ~ U[0, 1), the straight path x_t = (1 - t) x0 + t x1 to the normalised action x1, target x1 - x0, MSE, Adam.
    Returns the mean loss of every epoch."""
    x1_all = normalize_controls(actions, action_lo, action_hi)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    gen = torch.Generator(device=frames.device).manual_seed(seed)
    M, losses = frames.shape[0], []
    model.train()
    for _ in range(epochs):
        order = torch.randperm(M, device=frames.device, generator=gen)
        total = torch.zeros((), device=frames.device)
        for at in range(0, M, batch):
            idx = order[at:at + batch]
            x1 = x1_all[idx]
            x0 = torch.randn(x1.shape, device=x1.device, generator=gen)
            t = torch.rand((x1.shape[0], 1), device=x1.device, generator=gen)
            pred = model((1.0 - t) * x0 + t * x1, t, frames_to_input(frames[idx], image_size))
            loss = nn.functional.mse_loss(pred, x1 - x0)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += loss.detach() * idx.numel()
        losses.append(float(total) / M)
    model.eval()
    return losses


def demonstration_rows(demonstrations):
    """(frames [M, H, W, 4], actions [M, 2]) of the alive rows of what demonstrations.collect_demonstrations(images=True) returns."""
    alive = demonstrations["alive"].reshape(-1).bool()
    frames = demonstrations["frames"]
    return frames.reshape((-1,) + tuple(frames.shape[2:]))[alive], demonstrations["actions"].reshape(-1, 2)[alive]


def drive(venv, model, steps, graph_chunk=0, image_size=None, encoder="torch"):
    """The loop of main_flow_control.cpp:157-170 for every agent: `step`, the agents' frames (venv.camera()), the encoder and the
    device sampler from its output, `steps` times; the environment's auto-reset stands in for resetAgent (without it the loop ends
    once nobody is alive).  The trunk is the one given to venv.enable_flow_policy.  encoder="torch": model.bev_encoder in PyTorch
    behind frames_to_input; encoder="device": the one given to venv.enable_bev_encoder, no PyTorch op in the iteration (model is not
    used and may be None) -- the camera must render at the encoder's image_size, the device path does not resize.
    graph_chunk = K > 0 replays a HIP graph of K iterations.  Returns the steps taken."""
    assert encoder in ("torch", "device"), 'encoder is "torch" or "device"'
    assert getattr(venv, "flow_config", None) is not None, "call venv.enable_flow_policy(config, params) first"
    assert hasattr(venv, "camera_shape") and len(venv.camera_shape) == 4, 'call venv.enable_camera(..., fmt="rgba") first'
    frame = torch.empty(venv.camera_shape, dtype=torch.uint8, device=venv.device)
    if encoder == "device":
        assert getattr(venv, "bev_config", None) is not None, "call venv.enable_bev_encoder(config, params) first"
        S = venv.bev_config.image_size
        if tuple(venv.camera_shape[1:3]) != (S, S):
            raise ValueError('drive(encoder="device") needs the camera at the encoder\'s size: venv.enable_camera(width=%d, height=%d, fmt="rgba"); '
                             "it renders %dx%d (the device encoder does not resize; encoder=\"torch\" does)" % (S, S, venv.camera_shape[2], venv.camera_shape[1]))
        assert venv.bev_config.embed_dim == venv.flow_config.cond_dim, "the encoder's embed_dim is not the trunk's cond_dim"
        cond = torch.empty((venv.num_envs, venv.bev_config.embed_dim), dtype=torch.float32, device=venv.device)

        def iteration(_):
            venv.step()
            venv.camera(out=frame)
            venv.bev_encode(frame, out=cond)
            venv.flow_act(cond)

        def build():
            return iteration, (frame, cond)

        key = ("device",)
    else:
        module = model.bev_encoder

        def iteration(_):
            venv.step()
            venv.camera(out=frame)
            with torch.no_grad():
                cond = module(frames_to_input(frame, image_size))
            venv.flow_act(cond.contiguous())

        def build():
            venv.camera(out=frame)
            with torch.no_grad():  # the convolutions choose their kernels on the first call of a shape: not inside a capture
                module(frames_to_input(frame, image_size))
            return iteration, (frame, module)

        key = (id(module), image_size)

    K = int(graph_chunk)
    chunk = None
    if K > 0:
        chunk = _Chunk(K=K, graphs=venv._flow_graphs, key=(K,) + key, set_draw_offset=venv.env.flow_set_draw_offset, build=build, after_replay=None)
    _, taken = _run_episode(venv, iteration, int(steps), 8, chunk)
    return taken


__all__ = ["BEVEncoder", "ActionFlowTrunk", "ConditionalFlowMatchingPolicy", "flow_config_from_state_dict", "flow_params_from_state_dict",
           "bev_config_from_state_dict", "bev_params_from_state_dict", "frames_to_input", "sample", "train", "demonstration_rows", "drive", "normalize_controls", "denormalize_controls", "ACTION_LO",
           "ACTION_HI"]
