"""The world-model racers of WorldModelVaeRnn/ on the device environment: the conv VAE (train_vae.py: Encoder, Decoder, VAE) as PyTorch
modules for training, the hand-over of the encoder to the device act (okenv_world_*) and the CMA-ES loop of
main.cpp with every candidate an agent of one handle.

Training the VAE stays in PyTorch.  A generation is one batched rollout: camera -> act (the shared encoder, then each candidate's own
controller on [mu | sin(rot), cos(rot)]) -> step -> score, replayed as graph chunks until nobody is alive.  The reference evaluates its
candidates one after another, one frame at a time.

The memory (train_rnn.py's GRUDynamics) is optional: with it, the controllers read [mu | h_top] and the act is
okenv_memory_act.  Its training follows the reference's recipe in PyTorch; the decoder is only the VAE's training partner.
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


MEMORY_HIDDEN, MEMORY_LAYERS, SEQ_LEN = 512, 3, 5  # train_rnn.py's defaults
STATS = ("z_mean", "z_std", "a_mean", "a_std")   # stats.npz of train_rnn.py, behind the state dict in the network vector


class GRUDynamics(nn.Module):
    """The reference's dynamics model and its parameter names: a stacked GRU (batch first) on the normalised [z | a] and a linear head
    that predicts the normalised next latent.  forward(x [B, T, Z + 2], h [L, B, H] or None) -> (prediction [B, T, Z], h)."""

    def __init__(self, latent=Z_DIM, hidden=MEMORY_HIDDEN, layers=MEMORY_LAYERS, actions=2):
        super().__init__()
        assert actions == 2, "the device rule has two action values"
        self.latent, self.hidden, self.layers = int(latent), int(hidden), int(layers)
        self.gru = nn.GRU(self.latent + actions, self.hidden, num_layers=self.layers, batch_first=True)
        self.head = nn.Linear(self.hidden, self.latent)

    def forward(self, x, h=None):
        y, h = self.gru(x, h)
        return self.head(y), h


def memory_config_from_state_dict(sd, ctrl_hidden=HIDDEN, carry=True, throttle=THROTTLE, steer_scale=STEER_SCALE):
    """The capi.memory_config of the shape a state dict of GRUDynamics has."""
    layers = sum(1 for k in sd if k.startswith("gru.weight_hh_l"))
    return capi.memory_config(hidden=sd["gru.weight_hh_l0"].shape[1], layers=layers, ctrl_hidden=ctrl_hidden, carry=int(bool(carry)),
                              throttle=throttle, steer_scale=steer_scale)


def identity_stats(latent):
    """Statistics that normalise nothing: mean 0, std 1."""
    return {"z_mean": torch.zeros(latent), "z_std": torch.ones(latent), "a_mean": torch.zeros(2), "a_std": torch.ones(2)}


def memory_params_from_state_dict(sd, stats=None):
    """The network vector of okenv_memory_set_params: the state dict's tensors in their own order (capi.memory_layout), then the
    statistics z_mean, z_std, a_mean, a_std (a dict of tensors or arrays; None: identity_stats), float32."""
    latent = sd["head.weight"].shape[0]
    stats = identity_stats(latent) if stats is None else stats
    world = capi.world_config(latent=latent)
    given = {k: sd[k] for k in sd}
    given.update({k: torch.as_tensor(stats[k]) for k in STATS})
    pieces = []
    for name, _, shape in capi.memory_layout(world, memory_config_from_state_dict(sd)):
        assert tuple(given[name].shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(given[name].shape), tuple(shape))
        pieces.append(given[name].detach().to(dtype=torch.float32, device="cpu").reshape(-1))
    flat = torch.cat(pieces).contiguous()
    assert bool(torch.isfinite(flat).all()) and all(bool((torch.as_tensor(stats[k]) > 0).all()) for k in ("z_std", "a_std")), \
        "every value must be finite and every std > 0"
    return flat


def collect_latents(venv, steps, drive=None):
    """Rollouts for the memory's training through the device encoder: venv has its camera and world racers enabled (enable_camera,
    enable_world_racers with controllers set).  Every step records the stored action (the one the last step ran with), renders, takes
    mu from okenv_world_act's record, lets drive(venv) -- an expert, say -- overwrite the act's action, and steps.  Returns device
    tensors latents [T, N, Z], actions [T, N, 2] (the stored action in front of latent t, as the device rule pairs them) and alive
    [T, N] bool."""
    N, Z = venv.num_envs, venv.world_config.latent
    latents = torch.empty(steps, N, Z, device=venv.device)
    actions = torch.empty(steps, N, 2, device=venv.device)
    alive = torch.empty(steps, N, dtype=torch.bool, device=venv.device)
    frame = torch.empty(venv.camera_shape, dtype=torch.uint8, device=venv.device)
    venv.reset()
    for t in range(steps):
        actions[t, :, 0], actions[t, :, 1] = venv.throttle, venv.steering
        alive[t] = ~venv.done
        venv.camera(out=frame)
        venv.world_act(frame, {"mu": latents[t]})
        if drive is not None:
            drive(venv)
        venv.step()
    torch.cuda.synchronize(venv.device)
    return latents, actions, alive


def memory_windows(latents, actions, alive, seq_len=SEQ_LEN):
    """Every window of seq_len + 1 consecutive steps inside one agent's life: (z [M, seq_len + 1, Z], a [M, seq_len + 1, 2])."""
    T = latents.shape[0]
    if T <= seq_len:
        return latents.new_zeros(0, seq_len + 1, latents.shape[2]), actions.new_zeros(0, seq_len + 1, 2)
    ok = torch.stack([alive[k:T - seq_len + k] for k in range(seq_len + 1)]).all(0)  # [T - seq_len, N]
    t0, n = ok.nonzero(as_tuple=True)
    at = t0[:, None] + torch.arange(seq_len + 1, device=latents.device)[None]
    return latents[at, n[:, None]], actions[at, n[:, None]]


def train_memory(model, latents, actions, alive, epochs=1, batch=64, lr=1e-3, weight_decay=1e-4, seq_len=SEQ_LEN, seed=0):
    """The reference's recipe (train_rnn.py) on collect_latents' tensors: windows of seq_len inside one agent's life, teacher forcing
    (the input at every step is the recorded [z_t | a_t], normalised; the target the normalised z_{t+1}), mean squared error, AdamW,
    a cosine schedule over all steps, gradient clipping at 1.0; the normalisation statistics come from the training windows.  Returns
    (the mean loss of every epoch, the statistics as a dict of CPU tensors); leaves the model in eval mode."""
    z, a = memory_windows(latents, actions, alive, seq_len)
    assert z.shape[0] > 0, "no window of %d steps inside one agent's life" % (seq_len + 1)
    stats = {"z_mean": z.mean((0, 1)), "z_std": z.std((0, 1)).clamp_min(1e-6), "a_mean": a.mean((0, 1)), "a_std": a.std((0, 1)).clamp_min(1e-6)}
    zn, an = (z - stats["z_mean"]) / stats["z_std"], (a - stats["a_mean"]) / stats["a_std"]
    x, y = torch.cat([zn[:, :-1], an[:, :-1]], dim=2), zn[:, 1:]
    M = x.shape[0]
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max(1, epochs * -(-M // batch)))
    gen = torch.Generator(device=x.device).manual_seed(seed)
    losses = []
    model.train()
    for _ in range(epochs):
        order = torch.randperm(M, device=x.device, generator=gen)
        total = torch.zeros((), device=x.device)
        for at in range(0, M, batch):
            rows = order[at:at + batch]
            loss = nn.functional.mse_loss(model(x[rows])[0], y[rows])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            sched.step()
            total += loss.detach() * rows.numel()
        losses.append(float(total) / M)
    model.eval()
    return losses, {k: v.detach().cpu() for k, v in stats.items()}


def memory_window_starts(alive, seq_len=SEQ_LEN):
    """The flat first rows t0 * N + n of memory_windows' windows, in its order, as an int32 tensor [M], without materialising them: with
    row stride N, step s of window w is row start[w] + s * N of latents.reshape(T * N, Z)."""
    T, N = alive.shape
    if T <= seq_len:
        return torch.zeros(0, dtype=torch.int32, device=alive.device)
    ok = torch.stack([alive[k:T - seq_len + k] for k in range(seq_len + 1)]).all(0)
    t0, n = ok.nonzero(as_tuple=True)
    return (t0 * N + n).to(torch.int32)


def memory_from_params(vector, latent, hidden, layers):
    """A GRUDynamics and the statistics (train_memory's form) from a network vector (capi.memory_layout): the inverse of
    memory_params_from_state_dict."""
    model = GRUDynamics(latent=latent, hidden=hidden, layers=layers)
    flat = torch.as_tensor(vector).detach().to(dtype=torch.float32, device="cpu").reshape(-1)
    sd, stats = {}, {}
    for name, at, shape in capi.memory_layout(capi.world_config(latent=latent), capi.memory_config(hidden=hidden, layers=layers)):
        piece = flat[at:at + int(np.prod(shape))].reshape(tuple(shape)).clone()
        (stats if name in STATS else sd)[name] = piece
    model.load_state_dict(sd)
    return model.eval(), stats


def train_memory_device(venv, model, latents, actions, alive, epochs=1, batch=64, lr=1e-3, weight_decay=1e-4, seq_len=SEQ_LEN, seed=0, ctrl_hidden=HIDDEN,
                        carry=True):
    """train_memory's recipe on the device (okenv_memory_update): venv has its world racers enabled; model, a
    GRUDynamics, supplies the shape and the initial weights and is not changed.  The statistics come from the training windows as
    train_memory forms them and are written with the initial weights; the epochs' orders come from torch.randperm with train_memory's
    generator; the cosine schedule is a host array.  Attaches a memory of the model's shape and its learner to venv's handle.  Returns
    (the mean loss of every epoch, the statistics as a dict of CPU tensors, the trained network vector, a float32 device tensor)."""
    z, a = memory_windows(latents, actions, alive, seq_len)
    assert z.shape[0] > 0, "no window of %d steps inside one agent's life" % (seq_len + 1)
    stats = {"z_mean": z.mean((0, 1)), "z_std": z.std((0, 1)).clamp_min(1e-6), "a_mean": a.mean((0, 1)), "a_std": a.std((0, 1)).clamp_min(1e-6)}
    stats = {k: v.detach().cpu() for k, v in stats.items()}
    start = memory_window_starts(alive, seq_len)
    M, N = int(start.numel()), int(alive.shape[1])
    steps_per_epoch = -(-M // batch)
    sd = model.state_dict()
    env = venv.env
    env.memory_create(memory_config_from_state_dict(sd, ctrl_hidden=ctrl_hidden, carry=carry))
    flat = memory_params_from_state_dict(sd, stats).to(venv.device)
    env.memory_set_params("network", flat)
    venv.enable_memory_learner(lr=lr, weight_decay=weight_decay, seq_len=seq_len, max_batch=min(batch, M))
    gen = torch.Generator(device=latents.device).manual_seed(seed)
    order = torch.stack([torch.randperm(M, device=latents.device, generator=gen) for _ in range(epochs)]).to(torch.int32).contiguous()
    total = max(1, epochs * steps_per_epoch)  # CosineAnnealingLR with eta_min 0: the rate of step i
    schedule = np.array([lr * 0.5 * (1.0 + np.cos(np.pi * i / total)) for i in range(epochs * steps_per_epoch)], np.float32)
    loss, _ = venv.memory_update(latents.contiguous(), actions.contiguous(), start, batch, stride=N, epochs=epochs, order=order, lr_schedule=schedule)
    sizes = torch.tensor([min(batch, M - k * batch) for k in range(steps_per_epoch)], dtype=torch.float32, device=loss.device)
    losses = ((loss.reshape(epochs, steps_per_epoch) * sizes).sum(1) / M).tolist()
    vector = torch.empty_like(flat)
    env.memory_get_params("network", vector)
    return losses, stats, vector


class WorldModelRacers:
    """main.cpp:284-369 for `population` candidates at once, after cmaes.CmaEsRacers.  encoder_model: an Encoder (eval mode is set
    here).  encoder="device": okenv_world_act, no PyTorch op in the iteration; "torch": the module behind frames_to_input plus
    cmaes.BatchedController.  The fitness is the device's score kernel either way.

    memory: None, or a GRUDynamics (with memory_stats, train_memory's statistics): the controllers are Z + H wide and read
    [mu | h_top] (main.cpp's runVaeRnn); carry=False is the reference as written, whose hidden state starts from zero at every act.
    "device" acts through okenv_memory_act; "torch" runs the same state through the PyTorch modules."""

    RAYS = (-70.0, -30.0, 0.0, 30.0, 70.0)  # the agents still cast rays for the collision check's neighbourhood; nobody reads them

    def __init__(self, track, population, encoder_model, device=0, seed=0, encoder="device", hidden=HIDDEN, sigma=0.5, reset_randomly=False,
                 max_steps=1000, graph_chunk=8, skip_crashed=True, memory=None, memory_stats=None, carry=True, memory_shape=None):
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
        if torch.is_tensor(memory):  # train_memory_device's network vector, with memory_shape = (hidden, layers): its statistics are inside
            assert memory_shape is not None, "a network vector needs memory_shape=(hidden, layers)"
            memory, memory_stats = memory_from_params(memory, self.config.latent, *memory_shape)
        self.memory, self.carry = memory, bool(carry)
        width = self.config.latent + 2
        if memory is not None:
            assert memory.latent == self.config.latent, "the memory's latent width is not the encoder's"
            self.memory = memory.to(self.venv.device).eval()
            msd = self.memory.state_dict()
            self.memory_config = memory_config_from_state_dict(msd, ctrl_hidden=hidden, carry=carry)
            _, self.num_params = env.memory_create(self.memory_config)
            self._memory_flat = memory_params_from_state_dict(msd, memory_stats).to(self.venv.device)
            env.memory_set_params("network", self._memory_flat)
            stats = identity_stats(self.config.latent) if memory_stats is None else memory_stats
            self._stats = {k: torch.as_tensor(stats[k]).to(device=self.venv.device, dtype=torch.float32) for k in STATS}
            self._h = torch.zeros(memory.layers, population, memory.hidden, device=self.venv.device)
            width = self.config.latent + memory.hidden
        self.controller = BatchedController(width, hidden, 1, self.venv.device, population)
        assert self.controller.count_params() == self.num_params
        self.solver = CmaEsSolver(self.num_params, population, seed=seed, sigma=sigma, device=self.venv.device)
        self.frame = torch.empty(self.venv.camera_shape, dtype=torch.uint8, device=self.venv.device)
        self.generation = 0
        self._graphs = {}

    def set_params(self, population):
        """Controller::set_params for every candidate (main.cpp:316-317): one copy."""
        self.controller.set_params(population)
        if self.encoder == "device":
            if self.memory is not None:
                self.venv.env.memory_set_params("controllers", self.controller.flat)
            else:
                self.venv.env.world_set_params("controllers", self.controller.flat)

    def _memory_iteration(self):
        """The memory's act in PyTorch: the device rule's state, the alive agents' only where the device skips the crashed."""
        venv, st = self.venv, self._stats
        with torch.no_grad():
            mu = self.model(frames_to_input(self.frame))[0]
            a = torch.stack([venv.throttle, venv.steering], dim=1)
            x = torch.cat([(mu - st["z_mean"]) / st["z_std"], (a - st["a_mean"]) / st["a_std"]], dim=1)
            _, h = self.memory.gru(x[:, None], self._h if self.carry else None)
            out = self.controller.forward(torch.cat([mu, h[-1]], dim=1))
            if self.config.skip_crashed:
                keep = ~venv.done
                self._h.copy_(torch.where(keep[None, :, None], h, self._h))
                venv.throttle.copy_(torch.where(keep, torch.full_like(venv.throttle, THROTTLE), venv.throttle))
                venv.steering.copy_(torch.where(keep, out[:, 0] * STEER_SCALE, venv.steering))
            else:
                self._h.copy_(h)
                venv.throttle.fill_(THROTTLE)
                torch.mul(out[:, 0], STEER_SCALE, out=venv.steering)

    def _iteration(self, _=None):
        venv = self.venv
        venv.camera(out=self.frame)
        if self.encoder == "device":
            if self.memory is not None:
                venv.env.memory_act(self.frame)
            else:
                venv.env.world_act(self.frame)
        elif self.memory is not None:
            self._memory_iteration()
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
                mu = self.model(frames_to_input(self.frame))[0]
                if self.memory is not None:
                    self.memory.gru(torch.zeros(mu.shape[0], 1, mu.shape[1] + 2, device=mu.device), torch.zeros_like(self._h))
        return self._iteration, (self.frame,)

    def evaluate(self, population):
        """One batched rollout of given candidates [population, num_params]: resetAgent and the observation step, then the loop until
        nobody is alive.  Leaves their fitness in self.fitness and returns the steps taken."""
        self.set_params(population)
        self.venv.env.world_score_begin()
        chunk = None
        if self.graph_chunk > 0:
            chunk = _Chunk(K=self.graph_chunk, graphs=self._graphs, key=(self.graph_chunk, self.encoder), set_draw_offset=lambda word: None,
                           build=self._build, after_replay=None)
        if self.memory is not None:  # a new generation remembers nothing (the episode's own reset does not act, so the order is free)
            self.venv.env.memory_reset()
            self._h.zero_()
        _, steps = _run_episode(self.venv, self._iteration, self.max_steps, 8, chunk)
        self.fitness = self.venv.env.world_fitness().astype(np.float64)
        return steps

    def run_generation(self):
        """One pass of main.cpp:306-369: sample, evaluate, tell.  Returns (best fitness, steps)."""
        population = self.solver.sample()
        steps = self.evaluate(population)
        self.solver.tell(population, self.fitness)
        self.generation += 1
        return float(self.fitness.max()), steps


__all__ = ["Encoder", "Decoder", "VAE", "fold_batchnorm", "world_config_from_state_dict", "world_params_from_state_dict", "frames_to_input",
           "train_vae", "WorldModelRacers", "THROTTLE", "STEER_SCALE", "Z_DIM", "HIDDEN", "GRUDynamics", "memory_config_from_state_dict",
           "memory_params_from_state_dict", "identity_stats", "collect_latents", "memory_windows", "train_memory", "memory_window_starts",
           "memory_from_params", "train_memory_device", "MEMORY_HIDDEN",
           "MEMORY_LAYERS", "SEQ_LEN"]
