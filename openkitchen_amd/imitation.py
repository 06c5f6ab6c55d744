"""The imitation learner of ImitationLearningTransformer/ on the device environment: the network (laser_transformer.py:
LidarTransformer) as a PyTorch module for training, the hand-over of its weights to the device driver (okenv_lidar_*, DESIGN.md
section 22) and the driving loop of infer_torch_traced_main.cpp:138-148 for N agents.

Training stays in PyTorch, as in the reference's train.py; only acting runs as a HIP kernel.
"""
import math

import torch
from torch import nn

from . import _capi as capi
from .rollout import _Chunk, _run_episode


def sinusoid_table(rows, d_model, dtype=torch.float32):
    """pe[p][2i] = sin(p / 10000^(2i/d)), pe[p][2i+1] = cos(the same): the table of the reference's PositionalEncoding."""
    position = torch.arange(rows, dtype=dtype).unsqueeze(1)
    freq = torch.exp(torch.arange(0, d_model, 2, dtype=dtype) * (-math.log(10000.0) / d_model))
    pe = torch.zeros(rows, d_model, dtype=dtype)
    pe[:, 0::2] = torch.sin(position * freq)
    pe[:, 1::2] = torch.cos(position * freq)
    return pe


class _BatchIndexedEncoding(nn.Module):
    """The reference's positional module, bug for bug: its table pe [max_len, 1, d] is indexed by the FIRST dimension of the input,
    which is the batch of a batch-first tensor: sample b receives pe[b] on every token."""

    def __init__(self, d_model, max_len=1000):
        super().__init__()
        self.register_buffer("pe", sinusoid_table(max_len, d_model).unsqueeze(1))

    def forward(self, x):
        return x + self.pe[: x.size(0)]


class LidarTransformer(nn.Module):
    """The reference's architecture and parameter names (a best_model.pth of its train.py loads): Linear(2, d) per point, the
    positional term, `num_layers` post-norm nn.TransformerEncoderLayer (batch_first, ReLU, dropout 0.1), and the control head
    Linear(n_points d, head_hidden1) - ReLU - Linear(head_hidden1, head_hidden2) - ReLU - Linear(head_hidden2, 2).

    positional: "reference" adds what the reference adds (see _BatchIndexedEncoding); "token" adds pe[t] to token t."""

    def __init__(self, n_points=7, d_model=128, nhead=8, num_layers=3, dim_feedforward=512, head_hidden1=256, head_hidden2=64,
                 positional="reference"):
        super().__init__()
        assert positional in ("reference", "token")
        self.n_points, self.d_model, self.nhead, self.positional = n_points, d_model, nhead, positional
        self.point_embedding = nn.Linear(2, d_model)
        self.pos_encoder = _BatchIndexedEncoding(d_model)
        layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward, batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False)
        self.control_head = nn.Sequential(nn.Linear(d_model * n_points, head_hidden1), nn.ReLU(), nn.Linear(head_hidden1, head_hidden2),
                                          nn.ReLU(), nn.Linear(head_hidden2, 2))

    def forward(self, x):
        """x [B, n_points, 2], normalised points -> [B, 2], normalised controls."""
        x = self.point_embedding(x)
        x = self.pos_encoder(x) if self.positional == "reference" else x + self.pos_encoder.pe[: x.size(1), 0]
        x = self.transformer_encoder(x)
        return self.control_head(x.reshape(x.size(0), -1))

    def driven(self, x):
        """The forward the device driver computes from this module's weights: as forward(), but with the positional table of
        lidar_params_from_state_dict(positional=self.positional) -- "reference": row 0 on every token, whatever the batch."""
        x = self.point_embedding(x)
        x = x + (self.pos_encoder.pe[0, 0] if self.positional == "reference" else self.pos_encoder.pe[: x.size(1), 0])
        x = self.transformer_encoder(x)
        return self.control_head(x.reshape(x.size(0), -1))

    def lidar_config(self, **ranges):
        """The capi.lidar_config of this module's shape; ranges: action_lo, action_hi, sensor_range."""
        return lidar_config_from_state_dict(self.state_dict(), self.nhead, **ranges)


def normalize_points(rel_xy, sensor_range=200.0):
    """infer_torch_traced_main.cpp:19-29 on a tensor of points."""
    lo, hi = -sensor_range, sensor_range
    return 2 * (rel_xy - lo) / (hi - lo) - 1


def normalize_controls(actions, lo=(0.0, -2.0), hi=(100.0, 2.0)):
    """laser_transformer.py's normalize_controls on a tensor [..., 2] of (throttle, steering)."""
    lo, hi = actions.new_tensor(lo), actions.new_tensor(hi)
    return 2 * (actions - lo) / (hi - lo) - 1


def denormalize_controls(o, lo=(0.0, -2.0), hi=(100.0, 2.0)):
    lo, hi = o.new_tensor(lo), o.new_tensor(hi)
    return (o + 1) / 2 * (hi - lo) + lo


def lidar_config_from_state_dict(sd, nhead, **ranges):
    """The shape a state dict of the reference module has (nhead is not recoverable from the weights)."""
    d = sd["point_embedding.weight"].shape[0]
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer_encoder.layers."))
    return capi.lidar_config(num_points=sd["control_head.0.weight"].shape[1] // d, d_model=d, nhead=nhead, num_layers=layers,
                             dim_feedforward=sd["transformer_encoder.layers.0.linear1.weight"].shape[0],
                             head_hidden1=sd["control_head.0.weight"].shape[0], head_hidden2=sd["control_head.2.weight"].shape[0], **ranges)


def lidar_params_from_state_dict(sd, positional="reference", dtype=torch.float32):
    """The flat parameter vector of okenv_lidar_set_params from a state dict of the reference module: the pieces of capi.lidar_layout
    in order, then the positional table pos [R][d].

    positional="reference": what the reference's C++ driver adds.  Its PositionalEncoding indexes its table by the batch dimension,
    and the driver's batch is one, so every token receives row 0 = (0, 1, 0, 1, ...).  positional="token": pos[t] = pe[t].  The table
    is the state dict's "pos_encoder.pe" when it carries one, else the sinusoid table."""
    assert positional in ("reference", "token")
    cfg = lidar_config_from_state_dict(sd, 1)
    R, d = cfg.num_points, cfg.d_model
    pe = sd["pos_encoder.pe"].reshape(-1, d)[:R] if "pos_encoder.pe" in sd else sinusoid_table(R, d, torch.float64)
    pos = pe[:1].expand(R, d) if positional == "reference" else pe
    pieces = []
    for name, _, shape in capi.lidar_layout(cfg):
        t = pos if name == "pos" else sd[name]
        assert tuple(t.shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape))
        pieces.append(t.detach().to(dtype=dtype).reshape(-1))
    return torch.cat(pieces).contiguous()


def drive(venv, steps, graph_chunk=0):
    """The loop of infer_torch_traced_main.cpp:138-148 for every agent: `step`, then the policy's action from the new hit points,
    `steps` times; the environment's auto-reset stands in for resetAgent (without it the loop ends once nobody is alive).  The policy
    is the one given to venv.enable_lidar_policy.  graph_chunk = K > 0 replays a HIP graph of K iterations.  Returns the steps
    taken."""
    assert getattr(venv, "lidar_config", None) is not None, "call venv.enable_lidar_policy(config, params) first"

    def iteration(_):
        venv.step()
        venv.lidar_act()

    K = int(graph_chunk)
    chunk = None
    if K > 0:  # (the act draws nothing: there is no draw-offset word to hand over)
        chunk = _Chunk(K=K, graphs=venv._lidar_graphs, key=K, set_draw_offset=lambda word: None, build=lambda: (iteration, None),
                       after_replay=None)
    _, taken = _run_episode(venv, iteration, int(steps), 8, chunk)
    return taken


def demonstration_rows(demonstrations):
    """(points [M, R, 2], actions [M, 2]) of the alive rows of what demonstrations.collect_demonstrations returns."""
    alive = demonstrations["alive"].reshape(-1).bool()
    R = demonstrations["rel_xy"].shape[-2]
    return demonstrations["rel_xy"].reshape(-1, R, 2)[alive], demonstrations["actions"].reshape(-1, 2)[alive]


def train(model, points, actions, epochs=1, batch=128, lr=1e-4, seed=0, sensor_range=200.0, action_lo=(0.0, -2.0), action_hi=(100.0, 2.0)):
    """The reference's recipe (train.py) on device tensors: MSE on the normalised controls, Adam, shuffled batches.  Returns the mean
    loss of every epoch."""
    x, y = normalize_points(points, sensor_range), normalize_controls(actions, action_lo, action_hi)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    gen = torch.Generator(device=x.device).manual_seed(seed)
    losses = []
    model.train()
    for _ in range(epochs):
        order = torch.randperm(x.shape[0], device=x.device, generator=gen)
        total = torch.zeros((), device=x.device)
        for at in range(0, x.shape[0], batch):
            idx = order[at:at + batch]
            loss = nn.functional.mse_loss(model(x[idx]), y[idx])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += loss.detach() * idx.numel()
        losses.append(float(total) / x.shape[0])
    model.eval()
    return losses


__all__ = ["LidarTransformer", "lidar_params_from_state_dict", "lidar_config_from_state_dict", "drive", "train", "demonstration_rows",
           "normalize_points", "normalize_controls", "denormalize_controls", "sinusoid_table"]
