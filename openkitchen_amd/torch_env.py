"""Batched Python binding on device tensors: `step(actions) -> obs, done`.

The reference's Python surface is `open_kitchen_pybind.Environment(race_track_path, draw_rays, hidden_window)` with
`set_action(throttle, steering)` and `step()` for ONE agent behind a window (Pybind/bindings.cpp:19-79,
Pybind/example.py:10-20).  `VectorEnvironment` keeps those names and meanings for N agents and hands out the
library-owned struct-of-arrays state as zero-copy torch tensors (okenv_field_device_ptr), so a PyTorch-ROCm policy
reads observations and writes actions without a host round trip; everything is enqueued on torch's current stream.
The tensors also speak DLPack (`torch.Tensor.__dlpack__`) for other consumers.

PyTorch is plumbing here (device memory, streams); the step itself is the HIP kernel behind okenv_step.
"""
import torch

from . import _capi as capi
from .env import BatchedEnvironment, Track, default_ray_fan

_TYPESTR = {torch.float32: "<f4", torch.uint8: "|u1", torch.uint32: "<u4", torch.int32: "<i4"}


class _DeviceArray:
    """`__cuda_array_interface__` view of memory the okenv handle owns (kept alive through `owner`)."""

    def __init__(self, address, shape, dtype, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": _TYPESTR[dtype], "data": (address, False),
                                         "version": 2, "strides": None}


class VectorEnvironment:
    """N single-agent environments of the reference, stepped by one kernel launch.

    Field tensors (views, no copies): `distances` [N, R] = sensor_hits_[r].norm(), `rel_x/rel_y` [N, R] =
    sensor_hits_, `hit_x/hit_y`, `pos_x, pos_y, rot, speed, acceleration, throttle, steering` [N] f32,
    `crashed, timed_out, mode` [N] u8.  `done` is `crashed` viewed as bool (Agent::crashed_ covers wall hits and
    standstill timeouts).  With `reward="step"` (+1 per step, RLRacers/PPO/ppo_sim.cpp:77-80)
    or `reward="progress"` (centre-line index progress, CovarianceMatrixAdaptationEvolution/main_eigen.cpp:147-158)
    also `reward, fitness, episode_return` [N] f32, `episode_steps` [N] u32, `track_idx` [N] i32, updated by `step`.
    """

    FIELDS = {"pos_x": capi.F_POS_X, "pos_y": capi.F_POS_Y, "rot": capi.F_ROT, "speed": capi.F_SPEED,
              "acceleration": capi.F_ACC, "throttle": capi.F_THROTTLE, "steering": capi.F_STEER, "mode": capi.F_MODE,
              "crashed": capi.F_CRASHED, "timed_out": capi.F_TIMED_OUT, "hit_x": capi.F_HIT_X, "hit_y": capi.F_HIT_Y,
              "rel_x": capi.F_REL_X, "rel_y": capi.F_REL_Y, "distances": capi.F_DIST,
              # DisplacementStats (the standstill bookkeeping, Environment.h:17-27)
              "disp_ctr": capi.F_DISP_CTR, "disp_x": capi.F_DISP_X, "disp_y": capi.F_DISP_Y, "disp_timed_out": capi.F_DISP_TO}
    TRACKER_FIELDS = {"reward": capi.F_REWARD, "fitness": capi.F_FITNESS, "track_idx": capi.F_TRACK_IDX,
                      "episode_steps": capi.F_EPISODE_STEPS, "episode_return": capi.F_EPISODE_RETURN,
                      # the tracker's memory of crashed_ at its last update: part of the state capture() saves and restores
                      "prev_crashed": capi.F_PREV_CRASHED}
    SENSOR_RANGE = 200.0  # Agent::kSensorRange (Environment/Agent.h:10)

    def __init__(self, race_track_path, num_envs, num_rays=15, ray_angles_deg=None, device=0,
                 movement_mode=capi.MODE_VELOCITY, auto_reset=True, pick_random_point=True, randomize_lane=False,
                 randomize_heading=False, seed=0, agent_base=0, reward=None, draw_rays=False, hidden_window=True):
        # draw_rays / hidden_window: accepted for signature compatibility; there is no window (image observations come from
        # enable_camera / camera: every agent's bird's-eye view rendered on the device)
        del draw_rays, hidden_window
        if not torch.cuda.is_available():
            raise capi.OkenvError(-3, "VectorEnvironment needs a GPU; there is no CPU path")
        self.device = torch.device("cuda", int(device))
        self.track = race_track_path if isinstance(race_track_path, Track) else Track(race_track_path)
        rays = default_ray_fan(num_rays) if ray_angles_deg is None else ray_angles_deg
        self.env = BatchedEnvironment.from_track(self.track, num_envs, ray_angles_deg=rays, device=int(device))
        self.num_envs, self.num_rays = self.env.N, self.env.R
        self.seed, self.agent_base = int(seed), int(agent_base)
        self.reset_flags = ((capi.RESET_RANDOM_POINT if pick_random_point else 0) |
                            (capi.RESET_RANDOM_LANE if randomize_lane else 0) |
                            (capi.RESET_RANDOM_HEADING if randomize_heading else 0))
        with torch.cuda.device(self.device):
            self.env.set_stream(torch.cuda.current_stream().cuda_stream)
            for name, f in self.FIELDS.items():
                setattr(self, name, self._view(f))
            self.done = self.crashed.view(torch.bool)
            self.mode.fill_(int(movement_mode))
            # rollout bookkeeping on the device: reward / fitness / episode length (okenv_tracker_*)
            self.reward_kind = {None: None, "step": capi.REWARD_STEP, "progress": capi.REWARD_PROGRESS}[reward]
            if self.reward_kind is not None:
                self.env.tracker_create(self.reward_kind)
                for name, f in self.TRACKER_FIELDS.items():
                    setattr(self, name, self._view(f))
        self.auto_reset = bool(auto_reset)
        self.env.set_auto_reset(self.auto_reset, self.reset_flags, self.seed, self.agent_base)
        # Pybind/bindings.cpp:27-33: the agent starts on a (random) centre-line point with the track heading
        self.env.reset_random(None, capi.RESET_RANDOM_POINT if pick_random_point else 0, self.seed, 0xFFFFFFFF,
                              self.agent_base)

    def _view(self, field):
        address, nbytes = self.env.field_device_ptr(field)
        dtype = torch.from_numpy(capi.FIELD_DTYPE[field](0).reshape(1)).dtype
        shape = (self.num_envs, self.num_rays) if field in capi.PER_RAY else (self.num_envs,)
        t = torch.as_tensor(_DeviceArray(address, shape, dtype, self.env), device=self.device)
        assert t.data_ptr() == address and t.numel() * t.element_size() == nbytes
        return t

    def use_stream(self, stream):
        """Enqueue the environment's kernels on `stream` (a torch.cuda.Stream) from now on."""
        self.env.set_stream(stream.cuda_stream)

    def _state_tensors(self):
        names = list(self.FIELDS) + (list(self.TRACKER_FIELDS) if self.reward_kind is not None else [])
        return {n: getattr(self, n) for n in names}

    def capture(self, body, warmup=3):
        """Capture `body()` -- typically policy forward + `self.step(actions)` -- into a HIP graph and return it
        (`graph.replay()` runs one iteration).  A loop of one Environment step per policy evaluation is launch-bound
        (a dozen small kernels per iteration); replaying it as a graph removes the per-launch host cost.  The step
        counter that seeds the auto-reset draws lives on the device, so replays keep advancing it.  `body` must not
        synchronise or touch the host.  The `warmup` eager iterations that precede the capture (library and allocator
        initialisation) run on a copy: the environment's state and step count are restored afterwards, so capturing
        has no side effect on the simulation."""
        torch.cuda.synchronize(self.device)
        saved = {n: t.clone() for n, t in self._state_tensors().items()}
        count = self.env.step_count
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            self.use_stream(side)
            for _ in range(warmup):
                body()
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            body()
        self.use_stream(torch.cuda.current_stream(self.device))
        for n, t in self._state_tensors().items():
            t.copy_(saved[n])
        self.env.step_count = count
        torch.cuda.synchronize(self.device)
        return graph

    # ---- the reference binding's two methods, batched -------------------------------------------------------------
    def set_action(self, throttle_delta, steering_delta):
        """Agent::current_action_ of every agent; scalars or [N] tensors (Pybind/bindings.cpp:36-40)."""
        if torch.is_tensor(throttle_delta):
            self.throttle.copy_(throttle_delta, non_blocking=True)
        else:
            self.throttle.fill_(float(throttle_delta))
        if torch.is_tensor(steering_delta):
            self.steering.copy_(steering_delta, non_blocking=True)
        else:
            self.steering.fill_(float(steering_delta))

    def step(self, actions=None, n_steps=1):
        """Environment::step() for all agents.  `actions`: optional [N, 2] (throttle, steering) tensor.
        Returns (distances [N, R], done [N]) -- views that the next step overwrites."""
        if actions is not None:
            self.set_action(actions[:, 0], actions[:, 1])
        self.env.step(n_steps)
        if self.reward_kind is not None:
            self.env.tracker_update()
        return self.distances, self.done

    # ---- conveniences for learners ----------------------------------------------------------------------------------
    def observation(self):
        """sensor_hits_[i].norm() / kSensorRange, the network input of the reference's learners
        (RLRacers/PPO/PPOAgent.hpp:66-74, CovarianceMatrixAdaptationEvolution/main_eigen.cpp:45-56)."""
        return self.distances / self.SENSOR_RANGE

    def reset(self, mask=None, epoch=None):
        """Environment::resetAgent for all agents (or those in the bool/index tensor `mask`) with this environment's
        flags, then one step with the zeroed action for the initial observation (RLRacers/PPO/ppo_sim.cpp:53-60)."""
        epoch = self.env.step_count if epoch is None else int(epoch)
        if mask is None:
            self.env.reset_random(None, self.reset_flags, self.seed, epoch, self.agent_base)
        else:
            idx = mask.nonzero().flatten() if mask.dtype == torch.bool else mask
            idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
            if idx.numel():
                self.env.reset_random(idx, self.reset_flags, self.seed, epoch, self.agent_base)
        self.env.step(1)
        if self.reward_kind is not None:
            if mask is None:
                self.env.tracker_begin()
            else:
                self.env.tracker_update()  # re-placed agents restart their episode, the others take a normal step
        return self.distances, self.done

    # ---- bird's-eye camera views (include/okenv.h) ---------------------------------------------------
    def enable_camera(self, width=96, height=96, samples=1, fmt="rgba", heading_up=False, draw_agent=True, draw_heading=True,
                      view=None):
        """Sets up `camera()`: each agent's follow-camera frame of the track bands and its own disc, width x height pixels
        (samples x samples box-filtered samples each), `view` = (view_w, view_h) world px, default the reference's follow
        camera (1600 x 1400 at zoom 15).  fmt "rgba" gives [N, H, W, 4] uint8, "class" [N, H, W] band / agent classes."""
        fmt_code = {"rgba": capi.VIEW_RGBA8, "class": capi.VIEW_CLASS8}[fmt]
        flags = ((capi.VIEW_DRAW_AGENT if draw_agent else 0) | (capi.VIEW_DRAW_HEADING if draw_heading else 0) |
                 (capi.VIEW_HEADING_UP if heading_up else 0))
        self.env.render_create(self.track, width, height, samples, fmt_code, flags, view)
        self.camera_shape = self.env.render_shape

    def camera(self, out=None):
        """Every agent's view of the current state, rendered by one kernel on the environment's stream (torch's current stream
        unless use_stream chose another), without a synchronisation.
        `out`: a contiguous uint8 tensor of camera_shape on this device to fill in place; otherwise a new tensor."""
        if out is None:
            out = torch.empty(self.camera_shape, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != self.camera_shape or not out.is_contiguous() or out.device != self.device:
            raise ValueError("camera(out=...) needs a contiguous uint8 tensor of shape %s on %s" % (self.camera_shape, self.device))
        return self.env.render_views(out)

    # ---- expert drivers (include/okenv.h) --------------------------------------------------------------
    def enable_expert(self, kind="potfield", **params):
        """Attaches the reference's potential-field ("potfield") or vector-field-histogram ("vfh") driver
        (FieldNavigators/); params as in capi.expert_params (lookahead, goal_wrap, clamp_deg, ...)."""
        self.expert_params = self.env.expert_create(kind, **params)

    def expert_act(self, record=None):
        """The expert's updateAction for every agent from the last observation, written into `throttle` / `steering`: one
        kernel on the environment's stream, no synchronisation, usable inside capture(body).  record: optional dict of
        device tensors ("action" [N,2], "dist" [N,R], "rel_xy" [N,R,2] float32, "alive" [N] uint8) that receive the sample."""
        self.env.expert_act(record)

    # ---- shared-network actors (include/okenv.h) -------------------------------------------------------
    @staticmethod
    def _network_tensors(net, what):
        """[l1.weight, l1.bias, l2.weight, l2.bias] of Sequential(Linear, ReLU, Linear[, Softmax]) or of four raw tensors."""
        if isinstance(net, torch.nn.Module):
            mods = list(net.children()) if isinstance(net, torch.nn.Sequential) else None
            if mods is not None and len(mods) == 4 and isinstance(mods[3], torch.nn.Softmax):
                mods = mods[:3]
            if (mods is None or len(mods) != 3 or not isinstance(mods[0], torch.nn.Linear) or not isinstance(mods[1], torch.nn.ReLU)
                    or not isinstance(mods[2], torch.nn.Linear) or mods[0].bias is None or mods[2].bias is None):
                raise ValueError("%s: expected torch.nn.Sequential(Linear, ReLU, Linear[, Softmax]) with biases" % what)
            return [mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias]
        t = list(net)
        if len(t) != 4 or not all(torch.is_tensor(x) for x in t):
            raise ValueError("%s: expected a module or the four tensors l1.weight, l1.bias, l2.weight, l2.bias" % what)
        return t

    @staticmethod
    def _check_network(t, what, inputs, outputs=None, max_hidden=None):
        """(hidden width, outputs) of the four tensors of an inputs -> H -> outputs network (outputs None: any); ValueError otherwise."""
        w1, b1, w2, b2 = t
        hidden = w1.shape[0] if w1.dim() == 2 else -1
        out = w2.shape[0] if w2.dim() == 2 else -1
        if (tuple(w1.shape) != (hidden, inputs) or tuple(b1.shape) != (hidden,) or tuple(w2.shape) != (out, hidden)
                or tuple(b2.shape) != (out,) or (outputs is not None and out != outputs)):
            raise ValueError("%s: shapes %s do not form a %d -> H -> %s network" % (what, [tuple(x.shape) for x in t], inputs,
                                                                                 "A" if outputs is None else outputs))
        if max_hidden is not None and not 1 <= hidden <= max_hidden:
            raise ValueError("%s: hidden width %d outside 1 .. %d" % (what, hidden, max_hidden))
        return hidden, out

    def _flatten(self, tensors):
        """The tensors of one network as one float32 vector on the device, in parameters() order; None stays None."""
        if tensors is None:
            return None
        return torch.cat([x.detach().reshape(-1) for x in tensors]).to(device=self.device, dtype=torch.float32).contiguous()

    @staticmethod
    def _unflatten(tensors, vec):
        """_flatten's inverse: copies the vector's pieces back into the tensors."""
        at = 0
        with torch.no_grad():
            for x in tensors or ():
                x.copy_(vec[at:at + x.numel()].reshape(x.shape))
                at += x.numel()

    def enable_actor(self, actor, critic=None, mode="sample", actions=None, epsilon=0.0):
        """Attaches the reference's shared-network agent (RLRacers/PPO, Reinforce, Deep_Q_Learning): `actor` is
        torch.nn.Sequential(Linear(R, H), ReLU, Linear(H, A)[, Softmax]) or its four parameter tensors, `critic` optionally the
        same with one output; mode "sample" (PPO, REINFORCE), "greedy" or "eps_greedy" (Deep-Q, with `epsilon`); `actions` the
        table [(throttle, steering), ...] of A rows, default PPOAgent::kActionMap.  The modules are remembered: sync_actor() hands
        their current parameters to the device actor (call it after every optimiser step)."""
        from .rollout import PPO_ACTIONS
        actions = PPO_ACTIONS if actions is None else actions
        self._actor_nets = (self._network_tensors(actor, "actor"), None if critic is None else self._network_tensors(critic, "critic"))
        hidden, n_actions = self._check_network(self._actor_nets[0], "actor", self.num_rays, max_hidden=capi.ACTOR_MAX_HIDDEN)
        if n_actions != len(actions) or not 2 <= n_actions <= capi.ACTOR_MAX_ACTIONS:
            raise ValueError("actor: %d outputs for a table of %d actions (2 .. %d)" % (n_actions, len(actions), capi.ACTOR_MAX_ACTIONS))
        value_hidden = 0 if critic is None else self._check_network(self._actor_nets[1], "critic", self.num_rays, 1, capi.ACTOR_MAX_HIDDEN)[0]
        self.env.actor_create(hidden, actions, value_hidden, mode, epsilon, self.seed, self.agent_base)
        self.actor_has_value = critic is not None
        self.actor_dropout = 0.0  # (a new device actor starts without dropout)
        self._actor_graphs = {}
        self.sync_actor()

    def sync_actor(self):
        """The current parameters of the networks given to enable_actor, flattened in parameters() order and copied device to
        device on the environment's stream: no host hop, no synchronisation."""
        flat = [self._flatten(t) for t in self._actor_nets]
        self.env.actor_set_params(flat[0], flat[1])
        self._actor_flat = flat  # alive until the next hand-over: the copy is asynchronous

    def enable_learner(self, lr=3e-4, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8):
        """Attaches PPO's update to the device actor: Adam state for the networks given to enable_actor, with
        the reference's learning rate and clip and torch.optim.Adam's defaults.  rollout.ppo_update then steps the DEVICE parameters in
        place: the next actor_act uses them without sync_actor(), and pull_actor() copies them back into the modules."""
        assert getattr(self, "_actor_nets", None) is not None, "call enable_actor(actor, critic) first"
        self.env.learner_create(lr, clip, beta1, beta2, eps)
        self.learner_enabled = True

    def pull_actor(self):
        """Copies the device actor's parameters back into the modules (or tensors) given to enable_actor."""
        n_policy, n_value = self.env.actor_num_params()
        flat = [torch.empty(n, dtype=torch.float32, device=self.device) if t is not None else None
                for t, n in zip(self._actor_nets, (n_policy, n_value))]
        self.env.actor_get_params(out=flat)
        for tensors, vec in zip(self._actor_nets, flat):
            self._unflatten(tensors, vec)

    def set_actor_epsilon(self, epsilon):
        self.env.actor_set_epsilon(epsilon)
        self._actor_graphs = {}  # a captured launch carries the old value

    def set_actor_dropout(self, p, seed=None):
        """Dropout with probability p in [0, 1) on the hidden layer of the device actor's policy network, as the reference's REINFORCE
        network has it while acting and in the update (Reinforce/Policy.hpp:22-29); 0 switches it off.  The masks
        are keyed by `seed` (default: the environment's), the global agent id and the draw index, so rollout.reinforce_update regenerates
        them.  While it is on, rollout.ppo_update and rollout.dqn_update refuse."""
        self.env.actor_set_dropout(p, self.seed if seed is None else seed)
        self.actor_dropout = float(p)
        self._actor_graphs = {}  # a captured launch carries the old value

    def actor_act(self, record=None):
        """updateAction of the shared-network agents for every agent from the last observation, written into `throttle` /
        `steering`: one kernel on the environment's stream, no synchronisation, usable inside capture(body).  record: optional
        dict of device tensors ("state" [N,R] float32, "action" [N] int64, "prob" [N] float32, "value" [N] float32, "alive" [N]
        uint8 or bool) that receive the sample."""
        self.env.actor_act(record)

    # ---- Deep-Q learning (include/okenv.h) --------------------------------------------------------------
    def enable_replay(self, capacity, push_all=False, gamma=0.99, mask_done=False, target_network=False, seed=None):
        """Attaches a replay ring of `capacity` transitions that persists across episodes on the device, and sets the constants of
        rollout.dqn_update: the reference's discount, its target r + gamma max q' (mask_done: (1 - done) in front of gamma), no
        target network (target_network=True: q' comes from a copy that sync_target() refreshes).  push_all: push crashed agents' frozen
        observations too, as the reference's loop does; the default pushes the agents that entered the step alive."""
        self.env.replay_create(capacity, push_all)
        self.env.dqn_params(gamma, mask_done, target_network, self.seed if seed is None else seed)
        self.replay_push_all = bool(push_all)
        self._dqn_draw = 0
        self._actor_graphs = {}  # a captured push carries the old ring's pointers, capacity and flags

    def replay_push(self, record, reward=None):
        """Appends the transitions of the step that has just run to the ring: `record` is the dict the preceding actor_act filled
        ("state", "action", "alive"); reward: None for the reference's clearance reward, or a device float32 tensor [N] (the tracker's
        `reward`, say).  Two kernels on the environment's stream, no synchronisation, usable inside capture(body)."""
        self.env.replay_push(record, reward)

    def sync_target(self):
        """Copies the online Q network into the target network (device to device, no synchronisation)."""
        self.env.dqn_sync_target()

    # ---- DDPG (include/okenv.h) ---------------------------------------------------------------------------
    def enable_ddpg(self, actor, critic, **config):
        """Attaches the reference's DDPG agent (RLRacers/DDPG) with one hidden layer per network: `actor` is
        torch.nn.Sequential(Linear(R, H), ReLU, Linear(H, 2)) -- the device applies tanh * scale + bias to its output -- and `critic`
        Sequential(Linear(R + 2, Hc), ReLU, Linear(Hc, 1)) on torch.cat([state, action], 1), or their four parameter tensors each.
        config: the members of okenv_ddpg_config but the widths (capi.ddpg_config: scale, bias, noise, gamma, tau, lr_actor, lr_critic,
        beta1, beta2, eps, sample_seed).  The online and the target networks on the device start from the modules' parameters;
        rollout.ddpg_update steps them in place, and pull_ddpg() copies the online ones back into the modules."""
        nets = (self._network_tensors(actor, "actor"), self._network_tensors(critic, "critic"))
        widths = (self._check_network(nets[0], "actor", self.num_rays, 2)[0], self._check_network(nets[1], "critic", self.num_rays + 2, 1)[0])
        config.setdefault("seed", self.seed)
        config.setdefault("agent_base", self.agent_base)
        config.setdefault("sample_seed", self.seed)
        self.env.ddpg_create(widths[0], widths[1], **config)
        self._ddpg_nets = nets
        self._ddpg_graphs = {}
        flat = [self._flatten(t) for t in nets]
        self.env.ddpg_set_params(flat[0], flat[1])
        self._ddpg_flat = flat  # alive until the next hand-over: the copy is asynchronous

    def pull_ddpg(self):
        """Copies the device's online actor and critic back into the modules (or tensors) given to enable_ddpg."""
        names = ("actor", "critic")
        self._pull(dict(zip(names, self._ddpg_nets)), dict(zip(names, self.env.ddpg_num_params())), lambda flat: self.env.ddpg_state(out=flat))

    def ddpg_act(self, record=None):
        """The continuous action of every agent from the last observation, written into `throttle` / `steering`: one kernel on the
        environment's stream, no synchronisation, usable inside capture(body).  record: optional dict of device tensors ("state"
        [N,R] float32, "action" [N,2] float32, "alive" [N] uint8) that receive the sample."""
        self.env.ddpg_act(record)

    def enable_ddpg_replay(self, capacity, push_all=False):
        """Attaches DDPG's replay ring of `capacity` transitions that persists across episodes on the device."""
        self.env.ddpg_replay_create(capacity, push_all)
        self.ddpg_push_all = bool(push_all)
        self._ddpg_draw = 0
        self._ddpg_graphs = {}  # a captured push carries the old ring's pointers, capacity and flags

    def ddpg_replay_push(self, record, reward=None):
        """Appends the transitions of the step that has just run to DDPG's ring: `record` is the dict the preceding ddpg_act filled;
        reward: None for the reference's +1 per step, or a device float32 tensor [N].  Usable inside capture(body)."""
        self.env.ddpg_replay_push(record, reward)

    # ---- continuous REINFORCE (include/okenv.h) --------------------------------------------------------
    @staticmethod
    def _layer_tensors(module, what, layers, log_std):
        """[log_std,] then weight and bias of each Linear layer named in `layers`, of a module built like the reference's
        (RLRacers/ReinforceContinuous/Policy.hpp:17-30, RLRacers/GuidedCostLearning/Networks.hpp): parameters() order, a policy's own
        log_std first."""
        listed = "%s and %s" % (", ".join(layers[:-1]), layers[-1])
        try:
            t = [module.log_std] if log_std else []
            for name in layers:
                t += [getattr(module, name).weight, getattr(module, name).bias]
        except AttributeError:
            raise ValueError("%s: expected a module with %s%s (Linear layers with biases)" % (what, "log_std, " if log_std else "", listed))
        if any(x is None for x in t):
            raise ValueError("%s: %s need their biases" % (what, listed))
        return t

    def _pull(self, nets, counts, read):
        """Copies vectors of the device back into the tensors they were flattened from.  nets: {name: tensors}; counts: {name: floats};
        read(flat): fills the dict of device vectors `flat` (an env.*_state(out=flat))."""
        flat = {k: torch.empty(counts[k], dtype=torch.float32, device=self.device) for k in nets}
        read(flat)
        for k, tensors in nets.items():
            self._unflatten(tensors, flat[k])

    def enable_gauss_actor(self, policy_module, **config):
        """Attaches the reference's continuous REINFORCE agent (RLRacers/ReinforceContinuous): `policy_module` has log_std [2],
        fc1 = Linear(R, H1), fc2 = Linear(H1, H2) and mean = Linear(H2, 2); the device applies ReLU behind fc1 and fc2 and samples
        tanh(mu + exp(log_std) * eps) * scale + bias.  config: the members of okenv_gauss_config but the widths (capi.gauss_config:
        scale, bias, greedy, seed, agent_base).  The device's parameters start from the module's; rollout's update steps them in
        place, and pull_gauss() copies them back."""
        t = self._layer_tensors(policy_module, "policy", ("fc1", "fc2", "mean"), True)
        H1, H2 = t[1].shape[0], t[3].shape[0]
        shapes = [(2,), (H1, self.num_rays), (H1,), (H2, H1), (H2,), (2, H2), (2,)]
        if [tuple(x.shape) for x in t] != shapes:
            raise ValueError("policy: shapes %s do not form a %d -> H1 -> H2 -> 2 network with log_std [2]" % ([tuple(x.shape) for x in t], self.num_rays))
        config.setdefault("seed", self.seed)
        config.setdefault("agent_base", self.agent_base)
        self.env.gauss_create(H1, H2, **config)
        self._gauss_nets = t
        self._gauss_graphs = {}
        self.gauss_learner_enabled = False
        self.sync_gauss()

    def sync_gauss(self):
        """The module's current parameters to the device actor, device to device on the environment's stream."""
        self._gauss_flat = self._flatten(self._gauss_nets)  # alive until the next hand-over: the copy is asynchronous
        self.env.gauss_set_params(self._gauss_flat)

    def enable_gauss_learner(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        """Adam for the device's Gaussian actor (the reference's learning rate, torch.optim.Adam's defaults)."""
        assert getattr(self, "_gauss_nets", None) is not None, "call enable_gauss_actor(policy) first"
        self.env.gauss_learner_create(lr, beta1, beta2, eps)
        self.gauss_learner_enabled = True

    def pull_gauss(self):
        """Copies the device's parameters back into the module given to enable_gauss_actor."""
        self._pull({"params": self._gauss_nets}, {"params": self.env.gauss_num_params()}, lambda flat: self.env.gauss_state(out=flat))

    def set_gauss_greedy(self, greedy):
        self.env.gauss_set_greedy(greedy)
        self._gauss_graphs = {}  # a captured launch carries the old value

    def gauss_act(self, record=None):
        """The sampled (or greedy) action of every agent from the last observation, written into `throttle` / `steering`: one kernel
        on the environment's stream, no synchronisation, usable inside capture(body).  record: optional dict of device tensors
        ("state" [N,R], "eps", "pre", "action" [N,2], "logp" [N] float32, "alive" [N] uint8) that receive the sample."""
        self.env.gauss_act(record)

    # ---- guided cost learning (include/okenv.h) ----------------------------------------------------------
    def enable_gcl(self, policy_module, value_module, cost_module, **config):
        """Attaches the reference's guided-cost-learning agent (RLRacers/GuidedCostLearning): `policy_module` has log_std [2] and
        fc1 = Linear(R, H1), fc2 = Linear(H1, H2), fc3 = Linear(H2, 2) -- the device applies ReLU twice, tanh to the mean and samples
        tanh(mu + exp(log_std) * eps) * scale + bias; `value_module` has fc1, fc2, fc3 = Linear(H2, 1) of the same widths;
        `cost_module` fc1 = Linear(R + 2, C1), fc2 = Linear(C1, C2), fc3 = Linear(C2, 1), tanh twice, on torch.cat([state, action], 1).
        The state is the squared hit distance over the squared sensor range, not observation().  config: the members of okenv_gcl_config
        but the widths (capi.gcl_config: scale, bias, greedy, seed, agent_base).  The device's parameters start from the modules';
        rollout's updates step them in place, and pull_gcl() copies them back."""
        nets = {name: self._layer_tensors(module, name, ("fc1", "fc2", "fc3"), name == "policy")
                for name, module in (("policy", policy_module), ("value", value_module), ("cost", cost_module))}
        R = self.num_rays
        H1, H2 = nets["policy"][1].shape[0], nets["policy"][3].shape[0]
        C1, C2 = nets["cost"][0].shape[0], nets["cost"][2].shape[0]

        def shapes(n_in, a, b, out):
            return [(a, n_in), (a,), (b, a), (b,), (out, b), (out,)]

        want = {"policy": [(2,)] + shapes(R, H1, H2, 2), "value": shapes(R, H1, H2, 1), "cost": shapes(R + 2, C1, C2, 1)}
        for name, t in nets.items():
            if [tuple(x.shape) for x in t] != want[name]:
                raise ValueError("%s: shapes %s, expected %s" % (name, [tuple(x.shape) for x in t], want[name]))
        config.setdefault("seed", self.seed)
        config.setdefault("agent_base", self.agent_base)
        self.env.gcl_create(hidden1=H1, hidden2=H2, cost_hidden1=C1, cost_hidden2=C2, **config)
        self._gcl_nets = nets
        self._gcl_graphs = {}
        self.gcl_learner_enabled = False
        self.sync_gcl()

    def sync_gcl(self):
        """The modules' current parameters to the device's three networks, device to device on the environment's stream."""
        self._gcl_flat = {name: self._flatten(t) for name, t in self._gcl_nets.items()}  # alive until the next hand-over
        for name, flat in self._gcl_flat.items():
            self.env.gcl_set_params(name, flat)

    def enable_gcl_learner(self, lr=3e-4, clip=0.2, cost_lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
        """Adam for the device's three networks (the reference's learning rate and clip, torch.optim.Adam's defaults)."""
        assert getattr(self, "_gcl_nets", None) is not None, "call enable_gcl(policy, value, cost) first"
        self.env.gcl_learner_create(lr, clip, cost_lr, beta1, beta2, eps)
        self.gcl_learner_enabled = True

    def set_gcl_expert(self, demonstrations):
        """The expert bank from the dict demonstrations.collect_demonstrations returns: the alive rows, as rollout.gcl_expert_rows
        makes them.  Returns the number of rows."""
        from .rollout import gcl_expert_rows
        self._gcl_bank = gcl_expert_rows(demonstrations)  # alive until the next bank: the copy is asynchronous
        self.env.gcl_set_expert(*self._gcl_bank)
        return int(self._gcl_bank[0].shape[0])

    def pull_gcl(self):
        """Copies the device's parameters back into the modules given to enable_gcl."""
        for name, tensors in self._gcl_nets.items():
            self._pull({"params": tensors}, {"params": self.env.gcl_num_params(name)}, lambda flat: self.env.gcl_state(name, out=flat))

    def set_gcl_greedy(self, greedy):
        self.env.gcl_set_greedy(greedy)
        self._gcl_graphs = {}  # a captured launch carries the old value

    def gcl_act(self, record=None):
        """The sampled (or greedy) action of every agent from the last observation, written into `throttle` / `steering`: one kernel
        on the environment's stream, no synchronisation, usable inside capture(body).  record: optional dict of device tensors
        ("state" [N,R], "eps", "pre", "squashed", "action" [N,2], "logp" [N] float32, "alive" [N] uint8) that receive the sample."""
        self.env.gcl_act(record)

    # ---- lidar transformer driver (include/okenv.h) ----------------------------------------------------------
    def _attach_flat(self, family, config, params):
        """enable_lidar_policy's, enable_flow_policy's and enable_bev_encoder's hand-over: env.<family>_create(config), then the flat vector `params` (a tensor
        is brought to this device as float32).  Returns what was handed over, for the caller to keep until the next hand-over."""
        getattr(self.env, family + "_create")(config)
        if torch.is_tensor(params):
            params = params.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        getattr(self.env, family + "_set_params")(params)
        return params

    def enable_lidar_policy(self, config, params):
        """Attaches the reference's imitation policy (ImitationLearningTransformer: LidarTransformer) as a device driver.  config:
        a capi.lidar_config(...) or a dict of its members (num_points defaults to the environment's ray count); params: the flat
        vector imitation.lidar_params_from_state_dict makes, a float32 numpy array or a tensor.  Call it again with new params after
        training on."""
        if isinstance(config, dict):
            config = capi.lidar_config(**dict({"num_points": self.num_rays}, **config))
        self._lidar_flat = self._attach_flat("lidar", config, params)  # alive until the next hand-over: a tensor's copy is asynchronous
        self.lidar_config = config
        self._lidar_graphs = {}  # a captured launch carries the old shape and vector

    def lidar_act(self, record=None):
        """The policy's action of every agent from the last observation's hit points, written into `throttle` / `steering`: one
        kernel on the environment's stream, no synchronisation, usable inside capture(body).  record: optional dict of device tensors
        ("action" [N,2], "input" [N,R,2] float32, "alive" [N] uint8) that receive the sample."""
        self.env.lidar_act(record)

    # ---- flow-matching driver (include/okenv.h) -------------------------------------------------------------
    def enable_flow_policy(self, config, params):
        """Attaches the reference's flow-matching policy (FlowMatching: the Euler sampler of ActionFlowTrunk) as a device driver.
        config: a capi.flow_config(...) or a dict of its members (seed and agent_base default to the environment's); params: the flat
        vector flow.flow_params_from_state_dict makes, a float32 numpy array or a tensor.  Call it again with new params after
        training on."""
        if isinstance(config, dict):
            config = capi.flow_config(**dict({"seed": self.seed, "agent_base": self.agent_base}, **config))
        self._flow_flat = self._attach_flat("flow", config, params)  # alive until the next hand-over: a tensor's copy is asynchronous
        self.flow_config = config
        self._flow_graphs = {}  # a captured launch carries the old shape and vector

    def flow_act(self, cond, record=None):
        """The policy's action of every agent from `cond`, a contiguous float32 tensor [N, cond_dim] on this device (the image
        encoder's output), written into `throttle` / `steering`: one kernel on the environment's stream, no synchronisation, usable
        inside capture(body).  record: optional dict of device tensors ("x0", "x", "action" [N,2] float32, "alive" [N] uint8) that
        receive the sample."""
        if (not torch.is_tensor(cond) or cond.dtype != torch.float32 or not cond.is_contiguous() or cond.device != self.device
                or tuple(cond.shape) != (self.num_envs, self.flow_config.cond_dim)):
            raise ValueError("flow_act(cond) needs a contiguous float32 tensor of shape (%d, %d) on %s" % (self.num_envs, self.flow_config.cond_dim, self.device))
        self.env.flow_act(cond, record)

    # ---- the flow driver's image encoder (include/okenv.h) --------------------------------------------------
    def enable_bev_encoder(self, config, params):
        """Attaches the reference's image encoder (FlowMatching: BEVEncoder) as a device driver.  config: a capi.bev_config(...) or a
        dict of its members; params: the flat vector flow.bev_params_from_state_dict makes, a float32 numpy array or a tensor.  Call
        it again with new params after training on."""
        if isinstance(config, dict):
            config = capi.bev_config(**config)
        self._bev_flat = self._attach_flat("bev", config, params)  # alive until the next hand-over: a tensor's copy is asynchronous
        self.bev_config = config
        self._flow_graphs = {}  # a captured launch carries the old shape and vector

    def bev_encode(self, frames, out=None):
        """The embedding [N, embed_dim] float32 of every agent's frame: `frames` a contiguous uint8 tensor [N, S, S, 4] on this device
        (camera()'s, rendered at the encoder's image_size).  Three kernels on the environment's stream, no synchronisation, usable
        inside capture(body).  `out`: a contiguous float32 tensor to fill in place; otherwise a new tensor."""
        S, E = self.bev_config.image_size, self.bev_config.embed_dim
        if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.device != self.device
                or tuple(frames.shape) != (self.num_envs, S, S, 4)):
            raise ValueError("bev_encode(frames) needs a contiguous uint8 tensor of shape (%d, %d, %d, 4) on %s" % (self.num_envs, S, S, self.device))
        if out is None:
            out = torch.empty((self.num_envs, E), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (self.num_envs, E) or not out.is_contiguous() or out.device != self.device:
            raise ValueError("bev_encode(out=...) needs a contiguous float32 tensor of shape (%d, %d) on %s" % (self.num_envs, E, self.device))
        self.env.bev_encode(frames, out)
        return out

    # ---- behavioural-cloning image policy (include/okenv.h) -------------------------------------------------
    def enable_image_policy(self, config, params):
        """Attaches the reference's behavioural-cloning policy (BehavioralCloning: PolicyCNN) as a device driver.  config: a
        capi.cnn_config(...) or a dict of its members; params: the flat vector bc.cnn_params_from_state_dict makes, a float32 numpy
        array or a tensor.  Call it again with new params after training on."""
        if isinstance(config, dict):
            config = capi.cnn_config(**config)
        self._cnn_flat = self._attach_flat("cnn", config, params)  # alive until the next hand-over: a tensor's copy is asynchronous
        self.cnn_config = config
        self._cnn_graphs = {}  # a captured launch carries the old shape and vector

    def image_act(self, frames, record=None):
        """The policy's action of every agent from `frames`, a contiguous uint8 tensor [N, S, S, 4] on this device (camera()'s,
        rendered at the policy's image_size), written into `throttle` / `steering`: two kernels on the environment's stream, no
        synchronisation, usable inside capture(body).  record: optional dict of device tensors ("out" [N], "action" [N,2] float32,
        "alive" [N] uint8) that receive the sample."""
        S = self.cnn_config.image_size
        if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.device != self.device
                or tuple(frames.shape) != (self.num_envs, S, S, 4)):
            raise ValueError("image_act(frames) needs a contiguous uint8 tensor of shape (%d, %d, %d, 4) on %s" % (self.num_envs, S, S, self.device))
        self.env.cnn_act(frames, record)

    # ---- image transformer driver (include/okenv.h) -----------------------------------------------------------
    def enable_vit_policy(self, config, params):
        """Attaches DinoControl's vision transformer and head as a device driver.  config: a capi.vit_config(...) or a dict of its
        members; params: the flat vector dino.vit_params_from_state_dict makes, a float32 numpy array or a tensor.  Call it again with
        new params after training on."""
        if isinstance(config, dict):
            config = capi.vit_config(**config)
        self._vit_flat = self._attach_flat("vit", config, params)  # alive until the next hand-over: a tensor's copy is asynchronous
        self.vit_config = config
        self._vit_graphs = {}  # a captured launch carries the old shape and vector

    def vit_act(self, record=None, frames=None):
        """The policy's action of every agent from `frames`, a contiguous uint8 tensor [N, S, S, 4] on this device (None: camera()'s,
        rendered now; the camera must render at the policy's image_size), written into `throttle` / `steering`: a fixed sequence of
        kernels on the environment's stream, no synchronisation, usable inside capture(body).  record: optional dict of device
        tensors ("action" [N,2], "output" [N], "embedding" [N,D] float32, "alive" [N] uint8) that receive the sample."""
        S = self.vit_config.image_size
        if frames is None:
            frames = self.camera()
        if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.device != self.device
                or tuple(frames.shape) != (self.num_envs, S, S, 4)):
            raise ValueError("vit_act(frames) needs a contiguous uint8 tensor of shape (%d, %d, %d, 4) on %s" % (self.num_envs, S, S, self.device))
        self.env.vit_act(frames, record)

    # ---- the image transformer driver's training (include/okenv.h) -------------------------------------------
    def vit_embed(self, frames, out=None):
        """The frozen backbone's embedding [m, D] float32 of m frames, any m >= 1: `frames` a contiguous uint8 tensor [m, S, S, 4] on
        this device.  Runs in passes through the act's workspace on the environment's stream, no synchronisation, and touches no
        agent.  `out`: a contiguous float32 tensor to fill in place; otherwise a new tensor."""
        S, D = self.vit_config.image_size, self.vit_config.dim
        if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.device != self.device
                or frames.dim() != 4 or frames.shape[0] < 1 or tuple(frames.shape[1:]) != (S, S, 4)):
            raise ValueError("vit_embed(frames) needs a contiguous uint8 tensor of shape (m, %d, %d, 4) on %s" % (S, S, self.device))
        m = int(frames.shape[0])
        if out is None:
            out = torch.empty((m, D), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (m, D) or not out.is_contiguous() or out.device != self.device:
            raise ValueError("vit_embed(out=...) needs a contiguous float32 tensor of shape (%d, %d) on %s" % (m, D, self.device))
        self.env.vit_embed(frames, m, out)
        return out

    def enable_vit_head_learner(self, **params):
        """Adam for the head of the policy enable_vit_policy attached (capi.vit_head_params: lr, beta1, beta2, eps, weight, threshold;
        the reference's by default).  enable_vit_policy drops it again."""
        self.env.vit_head_learner_create(**params)

    def _vit_head_data(self, embedding, steer):
        D = self.vit_config.dim
        for name, t, tail in (("embedding", embedding, (D,)), ("steer", steer, ())):
            if (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device
                    or tuple(t.shape[1:]) != tail or t.shape[0] != embedding.shape[0] or t.shape[0] < 1):
                raise ValueError("%s must be a contiguous float32 tensor of shape (M%s) on %s" % (name, ", %d" % D if tail else "", self.device))
        return int(embedding.shape[0])

    def vit_head_update(self, embedding, steer, batch, epochs, order=None, grad=None):
        """Trains the head on cached embeddings [M, D] and recorded steering deltas [M] (float32 tensors on this device): every minibatch
        of `epochs` passes, two kernels each on the environment's stream, no synchronisation.  order: None (sequential) or an int32
        tensor [epochs, M] of sample indices.  The next vit_act acts with the new head.  Returns the minibatches' losses, a float32
        tensor [epochs * ceil(M / batch)] on the device; grad: an optional float32 tensor for the last minibatch's gradient."""
        M = self._vit_head_data(embedding, steer)
        if order is not None and (not torch.is_tensor(order) or order.dtype != torch.int32 or not order.is_contiguous() or order.device != self.device
                                  or order.numel() != int(epochs) * M):
            raise ValueError("order must be a contiguous int32 tensor of shape (%d, %d) on %s" % (int(epochs), M, self.device))
        loss = torch.empty(max(int(epochs), 0) * ((M + int(batch) - 1) // max(int(batch), 1)), dtype=torch.float32, device=self.device)
        self.env.vit_head_update(embedding, steer, M, batch, epochs, order, {"loss": loss if loss.numel() else None, "grad": grad})
        return loss

    def vit_head_eval(self, embedding, steer, batch):
        """The loss of every minibatch of one sequential pass with no update: a float32 tensor [ceil(M / batch)] on the device."""
        M = self._vit_head_data(embedding, steer)
        loss = torch.empty((M + int(batch) - 1) // max(int(batch), 1), dtype=torch.float32, device=self.device)
        self.env.vit_head_eval(embedding, steer, M, batch, loss)
        return loss

    # ---- the memory's training (include/okenv.h) -----------------------------------------------------------
    def enable_memory_learner(self, **config):
        """AdamW and clipping for the network of the memory attached to this environment's handle (capi.memory_learner_config: lr, beta1,
        beta2, eps, weight_decay, clip_grad, seq_len, max_batch; train_rnn.py's by default).  A new memory drops it again."""
        self.env.memory_learner_create(**config)

    def _memory_data(self, latent, action, start):
        Z = self.env.world_config.latent
        for name, t, dtype, tail in (("latent", latent, torch.float32, Z), ("action", action, torch.float32, 2), ("start", start, torch.int32, None)):
            if (not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous() or t.device != self.device or t.numel() < 1
                    or (tail is not None and t.shape[-1] != tail)):
                raise ValueError("%s must be a contiguous %s tensor%s on %s" % (name, dtype, "" if tail is None else " whose last dimension is %d" % tail, self.device))
        rows = latent.numel() // Z
        if action.numel() != 2 * rows:
            raise ValueError("latent and action must hold the same rows")
        return rows, int(start.numel())

    def memory_update(self, latent, action, start, batch, stride=1, epochs=1, order=None, lr_schedule=None, grad=None):
        """Trains the memory's network on windows of recorded latents [.., Z] and actions [.., 2] (float32 tensors on this device, the
        same leading dimensions, read as flat rows): window w begins at row start[w] (int32 tensor [M]) and steps by `stride` rows.
        Every minibatch of `epochs` passes is enqueued on the environment's stream, no synchronisation.  order: None (sequential) or an
        int32 tensor [epochs, M] of window indices; lr_schedule: None or a host array, one rate per minibatch.  The next memory_act acts
        with the new network.  Returns (losses, norms), float32 tensors [epochs * ceil(M / batch)] on the device; grad: an optional
        float32 tensor for the last minibatch's clipped gradient."""
        rows, M = self._memory_data(latent, action, start)
        if order is not None and (not torch.is_tensor(order) or order.dtype != torch.int32 or not order.is_contiguous() or order.device != self.device
                                  or order.numel() != int(epochs) * M):
            raise ValueError("order must be a contiguous int32 tensor of shape (%d, %d) on %s" % (int(epochs), M, self.device))
        steps = max(int(epochs), 0) * ((M + int(batch) - 1) // max(int(batch), 1))
        loss, norm = (torch.empty(steps, dtype=torch.float32, device=self.device) for _ in range(2))
        self.env.memory_update(latent, action, rows, start, M, batch, stride, epochs, order, lr_schedule,
                               {"loss": loss if steps else None, "norm": norm if steps else None, "grad": grad})
        return loss, norm

    def memory_eval(self, latent, action, start, batch, stride=1):
        """The loss of every minibatch of one sequential pass with no step: a float32 tensor [ceil(M / batch)] on the device."""
        rows, M = self._memory_data(latent, action, start)
        loss = torch.empty((M + int(batch) - 1) // max(int(batch), 1), dtype=torch.float32, device=self.device)
        self.env.memory_eval(latent, action, rows, start, M, batch, loss, stride)
        return loss

    def memory_learner_state(self, out=None):
        """The network vector, Adam's moments and t (env.memory_learner_state).  Synchronises."""
        return self.env.memory_learner_state(out)

    # ---- Deep-Q image racers (include/okenv.h) ---------------------------------------------------------------
    def enable_image_dqn(self, config, params, capacity=None, push_all=False):
        """Attaches the reference's image Q-network (RLRacers/DQN_CNN) as a device driver and, with `capacity`, its frame ring.
        config: a capi.qcnn_config(...) or a dict of its members (seed and agent_base default to the environment's); params: the flat
        vector dqn_cnn.qcnn_params_from_state_dict makes, a float32 numpy array or a tensor.  set_image_dqn_params hands new
        parameters over after an update."""
        if isinstance(config, dict):
            config = capi.qcnn_config(**dict({"seed": self.seed, "agent_base": self.agent_base}, **config))
        self._qcnn_flat = self._attach_flat("qcnn", config, params)  # alive until the next hand-over: a tensor's copy is asynchronous
        self.qcnn_config = config
        self._qcnn_graphs = {}  # a captured launch carries the old shape, vector and ring
        if capacity is not None:
            self.env.qcnn_ring_create(capacity, push_all)
            self.qcnn_push_all = bool(push_all)

    def set_image_dqn_params(self, params):
        """New parameters of the attached Q-network: a device tensor is copied device to device on the environment's stream."""
        if torch.is_tensor(params):
            params = params.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        self.env.qcnn_set_params(params)
        self._qcnn_flat = params

    def set_image_dqn_epsilon(self, epsilon):
        self.env.qcnn_set_epsilon(epsilon)
        self._qcnn_graphs = {}  # a captured launch carries the old value

    def _check_qcnn_frames(self, what, frames):
        S = self.qcnn_config.image_size
        if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.device != self.device
                or tuple(frames.shape) != (self.num_envs, S, S, 4)):
            raise ValueError("%s needs a contiguous uint8 tensor of shape (%d, %d, %d, 4) on %s" % (what, self.num_envs, S, S, self.device))

    def image_dqn_act(self, frames, record=None):
        """The Q-network's action of every agent from `frames`, a contiguous uint8 tensor [N, S, S, 4] on this device (camera()'s,
        rendered at the network's image_size), written into `throttle` / `steering`: two kernels on the environment's stream, no
        synchronisation, usable inside capture(body).  record: optional dict of device tensors ("q" [N,A], "value" [N] float32,
        "action" [N] int64, "alive" [N] uint8) that receive the sample."""
        self._check_qcnn_frames("image_dqn_act(frames)", frames)
        self.env.qcnn_act(frames, record)

    def image_dqn_push(self, record, frames, next_frames, reward=None):
        """Appends the transitions of the step that has just run to the frame ring: `record` as the preceding image_dqn_act filled it,
        `frames` what it saw, `next_frames` the camera after the step; reward: None for the clearance reward, or a device float32
        tensor [N].  Usable inside capture(body)."""
        self._check_qcnn_frames("image_dqn_push(frames)", frames)
        self._check_qcnn_frames("image_dqn_push(next_frames)", next_frames)
        self.env.qcnn_push(record, frames, next_frames, reward)

    def image_dqn_batch(self, B, mode="sequential", start_or_draw=0, out=None):
        """B positions of the frame ring as a dict of device tensors (state, next_state [B,S,S]; action int64, reward, done, index
        int32 [B]); `out`: such a dict to fill in place."""
        S = self.qcnn_config.image_size
        if out is None:
            f = dict(dtype=torch.float32, device=self.device)
            out = dict(state=torch.empty((B, S, S), **f), next_state=torch.empty((B, S, S), **f), action=torch.empty(B, dtype=torch.int64, device=self.device),
                       reward=torch.empty(B, **f), done=torch.empty(B, **f), index=torch.empty(B, dtype=torch.int32, device=self.device))
        self.env.qcnn_batch(B, out, mode, start_or_draw)
        return out

    # ---- world-model racers (include/okenv.h) ------------------------------------------------------------------
    def enable_world_racers(self, config, encoder_params, controllers=None):
        """Attaches the reference's world-model racers (WorldModelVaeRnn: the conv-VAE encoder, one controller per agent) as a device
        driver, with the track's lane widths for the score.  config: a capi.world_config(...) or a dict of its members; encoder_params:
        the flat vector worldmodel.world_params_from_state_dict makes; controllers: [N, controller] or None (set_world_controllers
        later, once per generation)."""
        if isinstance(config, dict):
            config = capi.world_config(**config)
        self.env.world_create(config)
        if torch.is_tensor(encoder_params):
            encoder_params = encoder_params.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        self.env.world_set_params("encoder", encoder_params)
        self._world_flat = encoder_params  # alive until the next hand-over: a tensor's copy is asynchronous
        self.env.world_set_lane_widths(self.track.wl, self.track.wr)
        self.world_config = config
        if controllers is not None:
            self.set_world_controllers(controllers)

    def set_world_controllers(self, controllers):
        """Every agent's controller, [N, controller] float32 (a numpy array or a tensor): one copy on the environment's stream."""
        if torch.is_tensor(controllers):
            controllers = controllers.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.env.world_set_params("controllers", controllers)
        self._world_controllers = controllers

    def world_act(self, frames, record=None):
        """Every agent's action from `frames`, a contiguous uint8 tensor [N, S, S, 4] on this device (camera()'s, rendered at the
        encoder's image_size), written into `throttle` / `steering` on the environment's stream, no synchronisation, usable inside
        capture(body).  record: optional dict of device tensors ("mu" [N,Z], "state" [N,Z+2], "out" [N], "action" [N,2] float32,
        "alive" [N] uint8)."""
        S = self.world_config.image_size
        if (not torch.is_tensor(frames) or frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.device != self.device
                or tuple(frames.shape) != (self.num_envs, S, S, 4)):
            raise ValueError("world_act(frames) needs a contiguous uint8 tensor of shape (%d, %d, %d, 4) on %s" % (self.num_envs, S, S, self.device))
        self.env.world_act(frames, record)

    def world_fitness(self):
        """The racers' fitness [N] as a float32 device tensor (a view of the handle's buffer; world_score() adds to it)."""
        return torch.as_tensor(_DeviceArray(self.env.world_fitness_device(), (self.num_envs,), torch.float32, self.env), device=self.device)

    def nearest_track_idx(self):
        """RaceTrack::findNearestTrackIndexBruteForce for every agent, as a device tensor."""
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        capi.check(self.env._L.okenv_nearest_track_idx(self.env._h, None, None, 0, capi.ptr(out)), self.env._h)
        return out

    def synchronize(self):
        self.env.sync()

    def close(self):
        self.env.close()
