"""The reference's Deep-Q learner on bird's-eye frames (RLRacers/DQN_CNN: CNN.hpp, DQCNNAgent.hpp, dq_cnn_racer_sim.cpp) on the host
side: the PyTorch module for the update, the rule's grey in torch, the hand-over of its weights to the device act (okenv_qcnn_*,
DESIGN.md section 29), the temporal-difference step and the episode loop for every agent of a VectorEnvironment.  The act, the grey
conversion, the replay ring and the batch gather run on the device; the update stays in PyTorch."""
import torch
from torch import nn

from . import _capi as capi

KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
KERNEL, STRIDE, PADDING, CHANNELS, HIDDEN, ACTIONS = (8, 4, 3), (4, 2, 1), (2, 1, 1), (32, 64, 64), 512, 5  # CNN.hpp
EPSILON, EPSILON_DISCOUNT, GAMMA, LEARNING_RATE = 0.99, 0.01, 0.99, 1e-4                                   # DQCNNAgent.hpp
ACTION_MAP = capi.QCNN_ACTION_MAP


class QCNN(nn.Module):
    """The reference's Q-network and its parameter names: three padded convolutions with ReLU on ONE grey channel, the flatten, fc1
    with ReLU, fc2 to the Q-values.  The flatten's width follows from image_size (the reference's 43 x 50 is its quarter-scale screen
    grab; the frames here are rendered at the network's own size)."""

    def __init__(self, image_size=96):
        super().__init__()
        self.image_size = int(image_size)
        self.conv1 = nn.Conv2d(1, CHANNELS[0], KERNEL[0], stride=STRIDE[0], padding=PADDING[0])
        self.conv2 = nn.Conv2d(CHANNELS[0], CHANNELS[1], KERNEL[1], stride=STRIDE[1], padding=PADDING[1])
        self.conv3 = nn.Conv2d(CHANNELS[1], CHANNELS[2], KERNEL[2], stride=STRIDE[2], padding=PADDING[2])
        side = capi.qcnn_sides(capi.qcnn_config(image_size=image_size))[2]
        assert side >= 1, "image_size %d is too small for the three convolutions" % image_size
        self.fc1 = nn.Linear(CHANNELS[2] * side * side, HIDDEN)
        self.fc2 = nn.Linear(HIDDEN, ACTIONS)

    def forward(self, x):
        """x [B, 1, S, S] grey planes (or [B, S, S]) -> Q-values [B, 5]."""
        if x.dim() == 3:
            x = x.unsqueeze(1)
        x = torch.relu(self.conv1(x))
        x = torch.relu(self.conv2(x))
        x = torch.relu(self.conv3(x))
        x = torch.relu(self.fc1(x.flatten(1)))
        return self.fc2(x)


def gray(frames):
    """The rule's grey of frames [N, S, S, 4] uint8 as [N, S, S] float32, operation by operation as DQCNNAgent::imageToTensor: the
    division by 255 (by a tensor: the division itself, not a multiplication by the reciprocal), then 0.2989 r + 0.5870 g + 0.1140 b with
    separate multiplications and additions.  Alpha is not an input."""
    x = frames[..., :3].to(torch.float32) / torch.full((1,), 255.0, dtype=torch.float32, device=frames.device)
    t = x[..., 0] * 0.2989
    t = t + x[..., 1] * 0.5870
    t = t + x[..., 2] * 0.1140
    return t


def _tensors(sd):
    return [sd[k] for k in KEYS]


def qcnn_config_from_state_dict(sd, image_size=96, stride=STRIDE, padding=PADDING, **members):
    """The capi.qcnn_config of the shape a state dict of the Q-network has, for frames of image_size (strides and paddings are not in
    a state dict: the reference's by default); members: mode, epsilon, seed, agent_base, action_table."""
    t = _tensors(sd)
    return capi.qcnn_config(image_size=image_size, kernel=[w.shape[2] for w in t[0:6:2]], stride=stride, padding=padding,
                            channels=[w.shape[0] for w in t[0:6:2]], hidden=t[6].shape[0], num_actions=t[8].shape[0], **members)


def qcnn_params_from_state_dict(sd, image_size=96, stride=STRIDE, padding=PADDING, dtype=torch.float32):
    """The flat parameter vector of okenv_qcnn_set_params: the pieces of capi.qcnn_layout in order."""
    cfg = qcnn_config_from_state_dict(sd, image_size, stride, padding)
    pieces = []
    for t, (name, _, shape) in zip(_tensors(sd), capi.qcnn_layout(cfg)):
        assert tuple(t.shape) == tuple(shape), "%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape))
        pieces.append(t.detach().to(dtype=dtype).reshape(-1))
    return torch.cat(pieces).contiguous()


def update(model, optimizer, batch, gamma=GAMMA, mask_done=False):
    """One step of DQCNNAgent::updateDQN on a batch (a dict of state, next_state [B, S, S], action [B] int64, reward, done [B], as
    venv.image_dqn_batch gives it): target = q.detach().clone() with r + gamma amax(q') written at the action (mask_done: (1 - done)
    in front of gamma, the reference's commented alternative), mse_loss, one optimiser step (the reference: Adam, lr 1e-4).  Returns
    the loss as a device tensor."""
    q = model(batch["state"])
    with torch.no_grad():
        best = torch.amax(model(batch["next_state"]), 1)
        g = (1.0 - batch["done"]) * gamma if mask_done else gamma
        target = q.detach().clone()
        target.scatter_(1, batch["action"].reshape(-1, 1), (batch["reward"] + g * best).reshape(-1, 1))
    loss = nn.functional.mse_loss(q, target)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss.detach()


def _record(venv):
    A = venv.qcnn_config.num_actions
    return {"q": torch.empty((venv.num_envs, A), dtype=torch.float32, device=venv.device),
            "action": torch.empty(venv.num_envs, dtype=torch.int64, device=venv.device),
            "value": torch.empty(venv.num_envs, dtype=torch.float32, device=venv.device),
            "alive": torch.empty(venv.num_envs, dtype=torch.uint8, device=venv.device)}


def run_episode(venv, model=None, max_steps=None, check_every=8, graph_chunk=0, policy="torch", reward=None):
    """One episode of dq_cnn_racer_sim.cpp's loop for every agent: reset and the initial frame, then `act -> step -> camera -> push`
    until every agent has crashed (tested every `check_every` steps) or `max_steps` steps have run.  ONE camera call per step: the
    frame rendered after the step is the push's next_frames and the next act's frames (two buffers that swap roles).  The transitions
    go straight into the frame ring of venv.enable_image_dqn(..., capacity=...).

    policy="device": the act of venv.enable_image_dqn (its mode and epsilon), no PyTorch op in the iteration (model is not used).
    policy="torch": `model` in PyTorch behind gray(), epsilon-greedy with torch's generator at the config's epsilon; the grey
    conversion of the push and the ring stay on the device.  reward: None for the clearance reward, "tracker" for the environment's
    `reward` tensor, or a device tensor [N] the caller keeps up to date.  graph_chunk = K > 0 (even) replays a HIP graph of K
    iterations; the test for the episode's end runs once per chunk.  Returns {"steps": steps taken}."""
    assert policy in ("torch", "device"), 'policy is "torch" or "device"'
    cfg = getattr(venv, "qcnn_config", None)
    assert cfg is not None and getattr(venv, "qcnn_push_all", None) is not None, "call venv.enable_image_dqn(config, params, capacity=...) first"
    assert hasattr(venv, "camera_shape") and len(venv.camera_shape) == 4, 'call venv.enable_camera(..., fmt="rgba") first'
    assert not venv.auto_reset or max_steps is not None, "with auto-reset on the episode never ends: pass max_steps"
    S, K = cfg.image_size, int(graph_chunk)
    if tuple(venv.camera_shape[1:3]) != (S, S):
        raise ValueError("run_episode needs the camera at the network's size: venv.enable_camera(width=%d, height=%d, fmt=\"rgba\"); "
                         "it renders %dx%d (the device path does not resize)" % (S, S, venv.camera_shape[2], venv.camera_shape[1]))
    assert K % 2 == 0, "graph_chunk must be even: the two frame buffers swap roles every step"
    if isinstance(reward, str):
        assert reward == "tracker" and venv.reward_kind is not None, 'reward="tracker" needs a VectorEnvironment with a reward'
        reward = venv.reward
    table = torch.tensor([tuple(row) for row in cfg.action_table][:cfg.num_actions], dtype=torch.float32, device=venv.device)

    def make():
        return [torch.empty(venv.camera_shape, dtype=torch.uint8, device=venv.device) for _ in range(2)], _record(venv)

    def iteration_on(bufs, rec):
        def iteration(t):
            cur, nxt = bufs[t % 2], bufs[(t + 1) % 2]
            if policy == "device":
                venv.image_dqn_act(cur, rec)
            else:
                with torch.no_grad():
                    q = model(gray(cur))
                    explore = torch.rand(venv.num_envs, device=venv.device) < cfg.epsilon
                    action = torch.where(explore, torch.randint(0, cfg.num_actions, (venv.num_envs,), device=venv.device), q.argmax(1))
                    rec["action"].copy_(action)
                    rec["alive"].copy_(~venv.done)
                    venv.throttle.copy_(table[action, 0])
                    venv.steering.copy_(table[action, 1])
            venv.step()
            venv.camera(out=nxt)
            venv.image_dqn_push(rec, cur, nxt, reward)
        return iteration

    key = (K, policy, None if policy == "device" else id(model), None if reward is None else reward.data_ptr())
    if K <= 0:
        if getattr(venv, "_qcnn_eager", None) is None or venv._qcnn_eager[0][0].shape != tuple(venv.camera_shape):
            venv._qcnn_eager = make()
        bufs, rec = venv._qcnn_eager
    elif key in venv._qcnn_graphs:
        bufs, rec = venv._qcnn_graphs[key][3][:2]
    else:
        bufs, rec = make()
    iteration = iteration_on(bufs, rec)

    venv.reset()  # resetAgent for every agent + the initial-observation step
    start = venv.env.step_count
    venv.camera(out=bufs[0])
    steps, offset = 0, None
    if K > 0:
        if key not in venv._qcnn_graphs:
            if policy == "torch":
                with torch.no_grad():  # the convolutions choose their kernels on the first call of a shape: not inside a capture
                    model(gray(bufs[0]))
            # (rollout._run_episode's scheme) without auto-reset a captured act carries the host's step count of the moment of
            # capture: the graph's last node advances a word of ours by K instead, which the act kernel adds to its draw index
            offset = None if venv.auto_reset else torch.zeros(1, dtype=torch.int32, device=venv.device)

            def body():
                for k in range(K):
                    iteration(k)
                if offset is not None:
                    offset.add_(K)

            if offset is not None:
                offset.add_(0)
            venv.env.qcnn_set_draw_offset(offset)
            try:
                graph = venv.capture(body, warmup=0)
            finally:
                venv.env.qcnn_set_draw_offset(None)
            venv._qcnn_graphs[key] = (graph, offset, venv.env.step_count, (bufs, rec, reward, model))
        graph, offset, base, _ = venv._qcnn_graphs[key]
        if offset is not None:
            offset.fill_(((start - base + 2 ** 31) % 2 ** 32) - 2 ** 31)
        check_every = K
    try:
        while True:
            if K > 0:
                graph.replay()
                steps += K
            else:
                iteration(steps)
                steps += 1
            if steps % check_every == 0 and venv.env.alive_count() == 0:
                break
            if max_steps is not None and steps >= max_steps:
                break
    finally:
        if offset is not None:
            venv.env.step_count = start + steps  # (replays do not advance the host's count)
    return {"steps": steps}


__all__ = ["QCNN", "gray", "qcnn_config_from_state_dict", "qcnn_params_from_state_dict", "update", "run_episode", "ACTION_MAP", "EPSILON",
           "EPSILON_DISCOUNT", "GAMMA", "LEARNING_RATE"]
