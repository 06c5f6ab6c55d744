"""The world-model racers of WorldModelVaeRnn/ on the device environment: the conv VAE (train_vae.py: Encoder, Decoder, VAE) as PyTorch
modules for training, the hand-over of the encoder to the device act (okenv_world_*) and the CMA-ES loop of
main.cpp with every candidate an agent of one handle.

Training the VAE stays in PyTorch.  A generation is one batched rollout: camera -> act (the shared encoder, then each candidate's own
controller on [mu | sin(rot), cos(rot)]) -> step -> score, replayed as graph chunks until nobody is alive.  The reference evaluates its
candidates one after another, one frame at a time; its GRU dynamics model and decoder are not called by its driver and are not here.
"""
import numpy as np
import torch
from torch import nn

from . import _capi as capi
from .cmaes import BatchedController, CmaEsSolver
from .flow import frames_to_input
from .rollout import _Chunk, _run_episode
from .torch_env import VectorEnvironment

THROTTLE, STEER_SCALE = 100.0, 5.0  # main.cpp:249-252
Z_DIM, HIDDEN = 32, 16              # main.cpp:72 and the controller's hidden width
CONVS = (0, 2, 5, 8)                # the convolutions' places in Encoder.net; a BatchNorm follows each but the first


class Encoder(nn.Module):
    """The reference's encoder and its parameter names: four stride-2 convolutions of kernel 4 and padding 1, BatchNorm behind all but
    the first, ReLU behind each, the flatten, fc_mu and fc_logvar.  channels: the four widths (the reference: ch, 2 ch, 4 ch, 8 ch)."""

    def __init__(self, image_size=128, latent=Z_DIM, channels=(64, 128, 256, 512)):
        super().__init__()
        assert image_size % 16 == 0, "image_size must be a multiple of 16"
        self.image_size, self.latent, self.channels = int(image_size), int(latent), tuple(int(c) for c in channels)
        layers, cin = [], 3
        for l, c in enumerate(self.channels):
            layers.append(nn.Conv2d(cin, c, 4, 2, 1))
            if l > 0:
                layers.append(nn.BatchNorm2d(c))
            layers.append(nn.ReLU(True))
            cin = c
        self.net = nn.Sequential(*layers)
        self.flatten_dim = cin * (image_size // 16) ** 2
        self.fc_mu = nn.Linear(self.flatten_dim, latent)
        self.fc_logvar = nn.Linear(self.flatten_dim, latent)

    def forward(self, x):
        flat = self.net(x).flatten(1)
        return self.fc_mu(flat), self.fc_logvar(flat)


class Decoder(nn.Module):
    """The encoder mirrored: a linear layer, four transposed convolutions, a sigmoid.  Only training uses it."""

    def __init__(self, image_size=128, latent=Z_DIM, channels=(64, 128, 256, 512)):
        super().__init__()
        self.side, c = image_size // 16, [int(v) for v in channels]
        self.fc = nn.Linear(latent, c[3] * self.side ** 2)
        layers = []
        for a, b in ((c[3], c[2]), (c[2], c[1]), (c[1], c[0])):
            layers += [nn.ConvTranspose2d(a, b, 4, 2, 1), nn.BatchNorm2d(b), nn.ReLU(True)]
        self.deconv = nn.Sequential(*layers, nn.ConvTranspose2d(c[0], 3, 4, 2, 1), nn.Sigmoid())

    def forward(self, z):
        return self.deconv(self.fc(z).view(z.size(0), -1, self.side, self.side))


class VAE(nn.Module):
    def __init__(self, image_size=128, latent=Z_DIM, channels=(64, 128, 256, 512)):
        super().__init__()
        self.enc = Encoder(image_size, latent, channels)
        self.dec = Decoder(image_size, latent, channels)

    def forward(self, x):
        mu, logvar = self.enc(x)
        z = mu + torch.randn_like(mu) * torch.exp(0.5 * logvar)
        return self.dec(z), mu, logvar


def fold_batchnorm(sd, eps=1e-5):
    """The encoder's convolutions with their eval-mode BatchNorm folded in, from a state dict of Encoder: {name: float64 tensor} under
    the names of capi.world_layout.  w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta, in float64."""
    out = {}
    for l, at in enumerate(CONVS):
        w, b = sd["net.%d.weight" % at].detach().double().cpu(), sd["net.%d.bias" % at].detach().double().cpu()
        if l > 0:
            bn = "net.%d." % (at + 1)
            scale = sd[bn + "weight"].detach().double().cpu() / torch.sqrt(sd[bn + "running_var"].detach().double().cpu() + eps)
            w = w * scale[:, None, None, None]
            b = (b - sd[bn + "running_mean"].detach().double().cpu()) * scale + sd[bn + "bias"].detach().double().cpu()
        out["net.%d.weight" % at], out["net.%d.bias" % at] = w, b
    out["fc_mu.weight"], out["fc_mu.bias"] = sd["fc_mu.weight"].detach().double().cpu(), sd["fc_mu.bias"].detach().double().cpu()
    return out


def world_config_from_state_dict(sd, image_size=128, hidden=HIDDEN, throttle=THROTTLE, steer_scale=STEER_SCALE, skip_crashed=0):
    """The capi.world_config of the shape a state dict of Encoder has, for frames of image_size."""
    return capi.world_config(image_size=image_size, channels=[sd["net.%d.weight" % at].shape[0] for at in CONVS],
                             latent=sd["fc_mu.weight"].shape[0], hidden=hidden, throttle=throttle, steer_scale=steer_scale,
                             skip_crashed=skip_crashed)


def world_params_from_state_dict(sd, image_size=128, eps=1e-5):
    """The encoder vector of okenv_world_set_params: the pieces of capi.world_layout in order, BatchNorm folded in float64 and rounded
    once to float32."""
    folded = fold_batchnorm(sd, eps)
    pieces = []
    for name, _, shape in capi.world_layout(world_config_from_state_dict(sd, image_size)):
        assert tuple(folded[name].shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(folded[name].shape), tuple(shape))
        pieces.append(folded[name].reshape(-1))
    return torch.cat(pieces).to(torch.float32).contiguous()


def train_vae(model, frames, epochs=1, batch=64, lr=2e-4, beta=1.0, seed=0):
    """The reference's recipe (train_vae.py) on a device tensor of frames [M, S, S, 4] uint8: binary cross-entropy of the reconstruction
    plus beta times the KL term, summed, Adam.  Returns the mean loss per frame of every epoch; leaves the model in eval mode."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    gen = torch.Generator(device=frames.device).manual_seed(seed)
    M, losses = frames.shape[0], []
    model.train()
    for _ in range(epochs):
        order = torch.randperm(M, device=frames.device, generator=gen)
        total = torch.zeros((), device=frames.device)
        for at in range(0, M, batch):
            x = frames_to_input(frames[order[at:at + batch]])
            recon, mu, logvar = model(x)
            loss = nn.functional.binary_cross_entropy(recon, x, reduction="sum") - 0.5 * beta * torch.sum(1 + logvar - mu.pow(2) - logvar.exp())
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += loss.detach()
        losses.append(float(total) / M)
    model.eval()
    return losses


class WorldModelRacers:
    """main.cpp:284-369 for `population` candidates at once, after cmaes.CmaEsRacers.  encoder_model: an Encoder (eval mode is set
    here).  encoder="device": okenv_world_act, no PyTorch op in the iteration; "torch": the module behind frames_to_input plus
    cmaes.BatchedController.  The fitness is the device's score kernel either way."""

    RAYS = (-70.0, -30.0, 0.0, 30.0, 70.0)  # the agents still cast rays for the collision check's neighbourhood; nobody reads them

    def __init__(self, track, population, encoder_model, device=0, seed=0, encoder="device", hidden=HIDDEN, sigma=0.5, reset_randomly=False,
                 max_steps=1000, graph_chunk=8, skip_crashed=True):
        assert encoder in ("device", "torch"), 'encoder is "device" or "torch"'
        self.encoder, self.max_steps, self.graph_chunk = encoder, int(max_steps), int(graph_chunk)
        self.venv = VectorEnvironment(track, population, ray_angles_deg=np.array(self.RAYS, dtype=np.float32), device=device,
                                      movement_mode=capi.MODE_VELOCITY, auto_reset=False, pick_random_point=reset_randomly, seed=seed)
        self.model = encoder_model.to(self.venv.device).eval()
        S = self.model.image_size
        self.venv.enable_camera(width=S, height=S, fmt="rgba")
        sd = self.model.state_dict()
        self.config = world_config_from_state_dict(sd, S, hidden=hidden, skip_crashed=int(bool(skip_crashed)))
        env = self.venv.env
        _, self.num_params = env.world_create(self.config)
        self._encoder_flat = world_params_from_state_dict(sd, S).to(self.venv.device)
        env.world_set_params("encoder", self._encoder_flat)
        env.world_set_lane_widths(self.venv.track.wl, self.venv.track.wr)
        self.controller = BatchedController(self.config.latent + 2, hidden, 1, self.venv.device, population)
        assert self.controller.count_params() == self.num_params
        self.solver = CmaEsSolver(self.num_params, population, seed=seed, sigma=sigma, device=self.venv.device)
        self.frame = torch.empty(self.venv.camera_shape, dtype=torch.uint8, device=self.venv.device)
        self.generation = 0
        self._graphs = {}

    def set_params(self, population):
        """Controller::set_params for every candidate (main.cpp:316-317): one copy."""
        self.controller.set_params(population)
        if self.encoder == "device":
            self.venv.env.world_set_params("controllers", self.controller.flat)

    def _iteration(self, _=None):
        venv = self.venv
        venv.camera(out=self.frame)
        if self.encoder == "device":
            venv.env.world_act(self.frame)
        else:
            with torch.no_grad():
                mu = self.model(frames_to_input(self.frame))[0]
                # the reference passes rot_, degrees, to std::sin / std::cos (main.cpp:231)
                state = torch.cat([mu, torch.sin(venv.rot)[:, None], torch.cos(venv.rot)[:, None]], dim=1)
                out = self.controller.forward(state)
            venv.throttle.fill_(THROTTLE)
            torch.mul(out[:, 0], STEER_SCALE, out=venv.steering)
        venv.step()
        venv.env.world_score()

    def _build(self):
        if self.encoder == "torch":  # the convolutions choose their kernels on the first call of a shape: not inside a capture
            with torch.no_grad():
                self.model(frames_to_input(self.frame))
        return self._iteration, (self.frame,)

    def run_generation(self):
        """One pass of main.cpp:306-369: sample, resetAgent and the observation step, the loop, tell.  Returns (best fitness, steps)."""
        population = self.solver.sample()
        self.set_params(population)
        self.venv.env.world_score_begin()
        chunk = None
        if self.graph_chunk > 0:
            chunk = _Chunk(K=self.graph_chunk, graphs=self._graphs, key=(self.graph_chunk, self.encoder), set_draw_offset=lambda word: None,
                           build=self._build, after_replay=None)
        _, steps = _run_episode(self.venv, self._iteration, self.max_steps, 8, chunk)
        self.fitness = self.venv.env.world_fitness().astype(np.float64)
        self.solver.tell(population, self.fitness)
        self.generation += 1
        return float(self.fitness.max()), steps


__all__ = ["Encoder", "Decoder", "VAE", "fold_batchnorm", "world_config_from_state_dict", "world_params_from_state_dict", "frames_to_input",
           "train_vae", "WorldModelRacers", "THROTTLE", "STEER_SCALE", "Z_DIM", "HIDDEN"]
