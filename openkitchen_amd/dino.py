"""The image transformer driver of DinoControl/ on the device environment: the frozen vision transformer (timm's
vit_small_patch8_224.dino) and the 384-128-64-1 policy head as PyTorch modules written anew with timm's parameter names, the hand-over
of their weights to the device act (okenv_vit_*) and the driving loop of main_dino_control.cpp for N agents.

timm is not needed: a checkpoint of timm's model loads into ViT by name (load_backbone).  Training trains the head only: in PyTorch
(train), or on the device driver's own parameter vector (train_device: okenv_vit_embed and okenv_vit_head_update, DESIGN.md section
31).  The forward, once per environment step, runs in PyTorch or, handed over, as the device act (drive(policy="device")).
"""
import torch
from torch import nn

from . import _capi as capi
from .rollout import _Chunk, _run_episode

THROTTLE, STEER_SCALE = 100.0, 10.0  # main_dino_control.cpp:80-89: the constant throttle, the steering per unit of the output and its clamp
SMALL = dict(image_size=32, patch=8, dim=32, heads=2, depth=2, dim_feedforward=64, head_hidden1=32, head_hidden2=16)  # examples' --small


class Attention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, T, D = x.shape
        q, k, v = self.qkv(x).reshape(B, T, 3, self.heads, D // self.heads).permute(2, 0, 3, 1, 4)
        attn = (q @ k.transpose(-2, -1) * (D // self.heads) ** -0.5).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, T, D))


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(nn.functional.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim, heads, hidden, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, heads)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, hidden)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class PatchEmbed(nn.Module):
    def __init__(self, patch, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class PolicyHead(nn.Module):
    """The reference's head on the class token: dim -> hidden1 -> hidden2 -> 1 with ReLU between."""

    def __init__(self, dim=384, hidden1=128, hidden2=64):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden1), nn.ReLU(), nn.Linear(hidden1, hidden2), nn.ReLU())
        self.output_layer = nn.Linear(hidden2, 1)

    def forward(self, x):
        return self.output_layer(self.net(x))


class ViT(nn.Module):
    """timm's VisionTransformer as the dino checkpoints use it (class token, learned positions, pre-norm blocks, GELU, LayerNorm eps
    1e-6, no dropout), under timm's parameter names, with the policy head where timm keeps its classifier: `head`.  parameters()
    is the device's parameter vector (capi.vit_layout).  forward: input [N, 3, S, S] -> the head's output [N, 1]."""

    def __init__(self, image_size=224, patch=8, dim=384, heads=6, depth=12, dim_feedforward=1536, head_hidden1=128, head_hidden2=64, ln_eps=1e-6):
        super().__init__()
        assert image_size % patch == 0
        self.image_size, self.patch = int(image_size), int(patch)
        tokens = (image_size // patch) ** 2 + 1
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, tokens, dim))
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.patch_embed = PatchEmbed(patch, dim)
        self.blocks = nn.Sequential(*[Block(dim, heads, dim_feedforward, ln_eps) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=ln_eps)
        self.head = PolicyHead(dim, head_hidden1, head_hidden2)

    def embed(self, x):
        """The class token behind the final LayerNorm, [N, dim]."""
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], dim=1) + self.pos_embed
        return self.norm(self.blocks(x))[:, 0]

    def forward(self, x):
        return self.head(self.embed(x))

    def backbone_parameters(self):
        return [p for n, p in self.named_parameters() if not n.startswith("head.")]


def load_backbone(model, state_dict):
    """A timm checkpoint of the backbone (no `head.*` of ours) into `model`; its own classifier entries, if any, are ignored."""
    own = {k: v for k, v in state_dict.items() if not k.startswith("head.") and not k.startswith("fc_norm.")}
    missing, unexpected = model.load_state_dict(own, strict=False)
    assert all(k.startswith("head.") for k in missing) and not unexpected, (missing, unexpected)
    return model


def vit_config_from_state_dict(sd, heads=6, mean=capi.IMAGENET_MEAN, std=capi.IMAGENET_STD, ln_eps=1e-6, throttle=THROTTLE, steer_scale=STEER_SCALE,
                               agents_per_pass=0, workspace_bytes=0):
    """The capi.vit_config of the shape a state dict of ViT has (the head count is not in a state dict: the reference's by default)."""
    w = sd["patch_embed.proj.weight"]
    dim, patch = int(w.shape[0]), int(w.shape[2])
    side = int(round((sd["pos_embed"].shape[1] - 1) ** 0.5))
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    return capi.vit_config(image_size=side * patch, patch=patch, dim=dim, heads=heads, depth=depth, dim_feedforward=int(sd["blocks.0.mlp.fc1.weight"].shape[0]),
                           head_hidden1=int(sd["head.net.0.weight"].shape[0]), head_hidden2=int(sd["head.net.2.weight"].shape[0]), mean=mean, std=std,
                           ln_eps=ln_eps, throttle=throttle, steer_scale=steer_scale, agents_per_pass=agents_per_pass, workspace_bytes=workspace_bytes)


def vit_params_from_state_dict(sd, heads=6, dtype=torch.float32):
    """The flat parameter vector of okenv_vit_set_params: the pieces of capi.vit_layout in order."""
    pieces = []
    for name, _, shape in capi.vit_layout(vit_config_from_state_dict(sd, heads)):
        t = sd[name]
        assert tuple(t.shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape))
        pieces.append(t.detach().to(dtype=dtype).reshape(-1))
    return torch.cat(pieces).contiguous()


def frames_to_input(frames, mean=capi.IMAGENET_MEAN, std=capi.IMAGENET_STD, dtype=torch.float32):
    """venv.camera()'s RGBA frames [N, S, S, 4] uint8 -> the transformer's input [N, 3, S, S]: drop alpha, / 255, (x - mean) / std per
    channel, NCHW.  No resize: the camera renders at the network's size.  mean and std: three numbers each, or tensors [3] on the
    frames' device (inside a graph capture nothing may be copied from the host)."""
    x = frames[..., :3].to(dtype).div(255.0)
    mean, std = (v if torch.is_tensor(v) else torch.tensor(v, dtype=dtype, device=frames.device) for v in (mean, std))
    return ((x - mean) / std).permute(0, 3, 1, 2).contiguous()


def weighted_mse(pred, label, weight=5.0, threshold=0.1):
    """The reference's loss: squared error, `weight` times where |label| > threshold."""
    w = torch.where(label.abs() > threshold, torch.full_like(label, weight), torch.ones_like(label))
    return (w * (pred - label) ** 2).mean()


def train(model, frames, actions, epochs=1, batch=64, lr=1e-4, seed=0, steer_scale=STEER_SCALE, mean=capi.IMAGENET_MEAN, std=capi.IMAGENET_STD):
    """The reference's recipe on device tensors: frames [M, S, S, 4] uint8, actions [M, 2] (throttle, steering).  The backbone is
    frozen (its embeddings are computed once, without gradients); the head alone is trained with weighted_mse against
    steering / steer_scale, Adam 1e-4.  Returns the mean loss of every epoch."""
    label = (actions[:, 1:2] / steer_scale).clamp(-1.0, 1.0)
    model.eval()
    with torch.no_grad():
        emb = torch.cat([model.embed(frames_to_input(frames[at:at + batch], mean, std)) for at in range(0, frames.shape[0], batch)])
    opt = torch.optim.Adam(model.head.parameters(), lr=lr)
    gen = torch.Generator(device=frames.device).manual_seed(seed)
    M, losses = frames.shape[0], []
    for _ in range(epochs):
        order = torch.randperm(M, device=frames.device, generator=gen)
        total = torch.zeros((), device=frames.device)
        for at in range(0, M, batch):
            idx = order[at:at + batch]
            loss = weighted_mse(model.head(emb[idx]), label[idx])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += loss.detach() * idx.numel()
        losses.append(float(total) / M)
    return losses


def epoch_means(losses, M, batch):
    """Per-minibatch mean losses [epochs * ceil(M / batch)] (a tensor) -> the mean loss of every epoch as train forms it: each
    minibatch's loss times its size, summed, over M."""
    K = (M + batch - 1) // batch
    sizes = torch.full((K,), float(batch), device=losses.device)
    sizes[-1] = float(M - (K - 1) * batch)
    return [float(v) for v in (losses.reshape(-1, K) * sizes).sum(dim=1) / M]


def train_device(venv, frames, actions, epochs=1, batch=64, lr=1e-4, seed=0, val_split=0.0, embed_chunk=256):
    """train's recipe on the device driver venv.enable_vit_policy attached: frames [M, S, S, 4] uint8 and actions [M, 2] on the device.
    The frozen backbone's embeddings are computed once (venv.vit_embed, `embed_chunk` frames a call), then the head alone is trained in
    the handle's parameter vector (venv.vit_head_update: a fresh Adam of `lr`, the weighted squared error against steering /
    steer_scale), in the orders train draws (torch.randperm of the same generator).  The next venv.vit_act acts with the new head.
    val_split > 0 keeps the last floor(M val_split) samples out of the training and evaluates them behind every epoch
    (venv.vit_head_eval).  Returns the mean loss of every epoch, formed as train forms it; with val_split > 0 the pair (training
    losses, validation losses)."""
    assert getattr(venv, "vit_config", None) is not None, "call venv.enable_vit_policy(config, params) first"
    total = int(frames.shape[0])
    held = int(total * float(val_split))
    M = total - held
    assert M >= 1 and epochs >= 1 and batch >= 1
    emb = torch.empty((total, venv.vit_config.dim), dtype=torch.float32, device=venv.device)
    for at in range(0, total, embed_chunk):
        venv.vit_embed(frames[at:at + embed_chunk], out=emb[at:at + embed_chunk])
    steer = actions[:, 1].to(torch.float32).contiguous()
    venv.enable_vit_head_learner(lr=lr)
    gen = torch.Generator(device=frames.device).manual_seed(seed)
    order = torch.stack([torch.randperm(M, device=frames.device, generator=gen) for _ in range(epochs)]).to(torch.int32)
    if held == 0:
        return epoch_means(venv.vit_head_update(emb[:M], steer[:M], batch, epochs, order), M, batch)
    losses, val = [], []
    for e in range(epochs):
        losses.append(venv.vit_head_update(emb[:M], steer[:M], batch, 1, order[e:e + 1]))
        val.append(venv.vit_head_eval(emb[M:], steer[M:], batch))
    return epoch_means(torch.cat(losses), M, batch), epoch_means(torch.cat(val), held, batch)


def head_from_device(venv, model):
    """Copies the head the device holds (trained by train_device) into model.head, so that the PyTorch module follows the driver."""
    cfg = venv.vit_config
    flat = torch.empty(capi.vit_num_params(cfg), dtype=torch.float32, device=venv.device)
    venv.env.vit_get_params(out=flat)
    own = dict(model.named_parameters())
    with torch.no_grad():
        for name, at, shape in capi.vit_layout(cfg):
            if name.startswith("head."):
                n = 1
                for s in shape:
                    n *= int(s)
                own[name].copy_(flat[at:at + n].reshape(shape))
    return model


def drive(venv, model, steps, policy="torch", graph_chunk=0, throttle=THROTTLE, steer_scale=STEER_SCALE, mean=capi.IMAGENET_MEAN, std=capi.IMAGENET_STD):
    """The loop of main_dino_control.cpp for every agent: `step`, the agents' frames (venv.camera()), the forward, the action (the
    constant throttle, the clamped steer_scale times the output), `steps` times; the environment's auto-reset stands in for
    resetAgent.  policy="torch": `model` in PyTorch behind frames_to_input; policy="device": the one given to
    venv.enable_vit_policy, no PyTorch op in the iteration (model may be None).  The camera must render at the network's image_size.
    graph_chunk = K > 0 replays a HIP graph of K iterations.  Returns the steps taken."""
    assert policy in ("torch", "device"), 'policy is "torch" or "device"'
    assert hasattr(venv, "camera_shape") and len(venv.camera_shape) == 4, 'call venv.enable_camera(..., fmt="rgba") first'
    frame = torch.empty(venv.camera_shape, dtype=torch.uint8, device=venv.device)
    if policy == "device":
        assert getattr(venv, "vit_config", None) is not None, "call venv.enable_vit_policy(config, params) first"
        S = venv.vit_config.image_size
    else:
        S = model.image_size
    if tuple(venv.camera_shape[1:3]) != (S, S):
        raise ValueError("drive needs the camera at the policy's size: venv.enable_camera(width=%d, height=%d, fmt=\"rgba\"); it renders %dx%d "
                         "(there is no resize)" % (S, S, venv.camera_shape[2], venv.camera_shape[1]))
    if policy == "device":
        graphs = venv._vit_graphs

        def iteration(_):
            venv.step()
            venv.camera(out=frame)
            venv.vit_act(frames=frame)

        def build():
            return iteration, (frame,)

        key = ("device",)
    else:
        if not hasattr(venv, "_dino_graphs"):
            venv._dino_graphs = {}
        graphs = venv._dino_graphs
        mean, std = (torch.tensor(v, dtype=torch.float32, device=venv.device) for v in (mean, std))

        def iteration(_):
            venv.step()
            venv.camera(out=frame)
            with torch.no_grad():
                out = model(frames_to_input(frame, mean, std))[:, 0]
            venv.throttle.fill_(throttle)
            torch.clamp(out * steer_scale, -steer_scale, steer_scale, out=venv.steering)

        def build():
            venv.camera(out=frame)
            with torch.no_grad():  # the library chooses its kernels on the first call of a shape: not inside a capture
                model(frames_to_input(frame, mean, std))
            return iteration, (frame, model, mean, std)

        key = (id(model), float(throttle), float(steer_scale))

    K = int(graph_chunk)
    chunk = None
    if K > 0:  # (the act draws nothing: there is no draw-offset word to hand over)
        chunk = _Chunk(K=K, graphs=graphs, key=(K,) + key, set_draw_offset=lambda word: None, build=build, after_replay=None)
    _, taken = _run_episode(venv, iteration, int(steps), 8, chunk)
    return taken


__all__ = ["ViT", "PolicyHead", "load_backbone", "vit_config_from_state_dict", "vit_params_from_state_dict", "frames_to_input", "weighted_mse", "train",
           "train_device", "epoch_means", "head_from_device", "drive", "THROTTLE", "STEER_SCALE", "SMALL"]
