"""Python host side of the batched Environment step: thin, typed wrappers over the C ABI.

`Track` mirrors the reference's RaceTrack + TrackSegments (Environment/RaceTrack.h, TrackSegments.h) and
`BatchedEnvironment` mirrors Environment's step surface (Environment/Environment.h:31-75) for N agents at
once with device-resident state.  bench.py, the parity tests and the Python callers use these; the C++
callers use the classes in include/Environment/.  All compute happens in libokenv.so on the GPU.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _capi as capi

TRACK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tracks")

# What tells Deep-Q's replay ring from DDPG's (ringCreate ... ringGet serve both on the C side): the symbols' prefix, the two structs, the
# attribute that remembers the capacity, and the action's shape and dtype per transition.
_Ring = collections.namedtuple("_Ring", "prefix ring_struct record_struct capacity_attr action_shape action_dtype")
_DQN_RING = _Ring("okenv_replay", capi.OkenvReplayRing, capi.OkenvActorRecord, "replay_capacity", (), np.int64)
_DDPG_RING = _Ring("okenv_ddpg_replay", capi.OkenvDdpgRing, capi.OkenvDdpgRecord, "ddpg_replay_capacity", (2,), np.float32)


def track_path(name):
    """Path of a bundled TUMFTM racetrack-database CSV (Austin, Silverstone, Monza, Spa)."""
    p = name if name.endswith(".csv") else os.path.join(TRACK_DIR, name + ".csv")
    if not os.path.exists(p):
        raise FileNotFoundError(p)
    return p


def default_ray_fan(num_rays):
    """angle_i = -70 + 140*i/(R-1) degrees, fp32 (generalises Agent.cpp:11-18)."""
    if num_rays == 1:
        return np.zeros(1, dtype=np.float32)
    i = np.arange(num_rays, dtype=np.float32)
    return (np.float32(-70.0) + np.float32(140.0) * i / np.float32(num_rays - 1)).astype(np.float32)


class Track:
    """RaceTrack(csv) + TrackSegments(track): centre line, headings, four boundary polylines, 4*P segments."""

    KEYS = ["x", "y", "wr", "wl", "heading", "li", "lo", "ri", "ro"]

    def queries(self, qx, qy):
        """RaceTrack::getNearestDistanceToTrackBoundary and RaceTrack::getDistanceToLaneCenter (reference
        Environment/RaceTrack.cpp:33-72) for arrays of query points: (distance to the nearest inner-boundary point [px],
        distance to the nearest centre-line point / lane width there)."""
        L = capi.load()
        qx = np.ascontiguousarray(qx, dtype=np.float32).reshape(-1)
        qy = np.ascontiguousarray(qy, dtype=np.float32).reshape(-1)
        assert qx.size == qy.size
        boundary, lane = np.zeros(qx.size, dtype=np.float32), np.zeros(qx.size, dtype=np.float32)
        h = C.c_void_p()
        capi.check(L.okenv_track_load(C.byref(h), self.path.encode()))
        try:
            capi.check(L.okenv_track_queries(h, capi.ptr(qx), capi.ptr(qy), qx.size, capi.ptr(boundary), capi.ptr(lane)))
        finally:
            L.okenv_track_free(h)
        return boundary, lane

    def __init__(self, name_or_path):
        L = capi.load()
        self.path = track_path(name_or_path)
        h = C.c_void_p()
        capi.check(L.okenv_track_load(C.byref(h), self.path.encode()))
        try:
            self.P = L.okenv_track_num_points(h)
            self.S = L.okenv_track_num_segments(h)
            for w, k in enumerate(self.KEYS):
                a = np.zeros(self.P if w < 5 else 2 * self.P, dtype=np.float32)
                capi.check(L.okenv_track_get(h, w, capi.ptr(a)))
                setattr(self, k, a)
            seg = np.zeros((self.S, 4), dtype=np.float32)
            capi.check(L.okenv_track_segments(h, capi.ptr(seg)))
            self.segments = seg
        finally:
            L.okenv_track_free(h)

    def band_triangles(self):
        """The draw list of the track bands (okenv_track_band_triangles, host only): (xy [6P, 3, 2] float32 in DrawTriangle's vertex
        order, draw ordinal [6P] uint8)."""
        L = capi.load()
        h = C.c_void_p()
        capi.check(L.okenv_track_load(C.byref(h), self.path.encode()))
        try:
            n = L.okenv_track_band_triangles(h, None, None, 0)
            if n < 0:
                capi.check(n)
            xy, ordinal = np.zeros((n, 3, 2), dtype=np.float32), np.zeros(n, dtype=np.uint8)
            assert L.okenv_track_band_triangles(h, capi.ptr(xy), capi.ptr(ordinal), n) == n
        finally:
            L.okenv_track_free(h)
        return xy, ordinal


def _flat_params(v, n):
    """A network's n parameters as the C ABI takes them: a float32 numpy array made flat and contiguous, or a device tensor that must be
    so already; None stays None (the network is left as it is)."""
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        v = np.ascontiguousarray(v, dtype=np.float32).ravel()
        assert v.size == n, "expected %d parameters, got %d" % (n, v.size)
    else:
        assert v.is_contiguous() and v.numel() == n and v.element_size() == 4, "expected %d float32 parameters" % n
    return v


class BatchedEnvironment:
    """N agents x R rays on one GPU.  State lives on the device; see include/okenv.h for field semantics."""

    def __init__(self, segments, num_agents, ray_angles_deg, device=0, flags=0, grid_cell=0.0, centerline=None):
        L = capi.load()
        seg = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 4)
        rays = np.ascontiguousarray(ray_angles_deg, dtype=np.float32)
        self.N, self.R, self.S = int(num_agents), int(rays.size), int(seg.shape[0])
        self._h = C.c_void_p()
        capi.check(L.okenv_create(C.byref(self._h), capi.ptr(seg), self.S, self.N, self.R, capi.ptr(rays), int(device),
                                  int(flags), float(grid_cell)))
        self._L = L
        self.ray_angles_deg = rays
        if centerline is not None:
            self.set_centerline(*centerline)

    @classmethod
    def from_track(cls, track, num_agents, num_rays=None, ray_angles_deg=None, **kw):
        rays = default_ray_fan(num_rays) if ray_angles_deg is None else ray_angles_deg
        env = cls(track.segments, num_agents, rays, centerline=(track.x, track.y, track.heading), **kw)
        env.set_lane_bounds(track.li, track.ri)
        return env

    def close(self):
        if getattr(self, "_h", None):
            self._L.okenv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- configuration ---------------------------------------------------------------------------
    def info(self):
        i = capi.OkenvInfo()
        capi.check(self._L.okenv_get_info(self._h, C.byref(i)), self._h)
        return {k: getattr(i, k) for k, _ in capi.OkenvInfo._fields_}

    def set_centerline(self, x, y, heading_deg):
        x, y, hd = [np.ascontiguousarray(a, dtype=np.float32) for a in (x, y, heading_deg)]
        self.P = int(x.size)
        capi.check(self._L.okenv_set_centerline(self._h, capi.ptr(x), capi.ptr(y), capi.ptr(hd), self.P), self._h)

    def set_lane_bounds(self, left_inner_xy, right_inner_xy):
        """RaceTrack::left_bound_inner_ / right_bound_inner_ as xy pairs (resetAgent's lane randomisation)."""
        l = np.ascontiguousarray(left_inner_xy, dtype=np.float32).reshape(-1)
        r = np.ascontiguousarray(right_inner_xy, dtype=np.float32).reshape(-1)
        assert l.size == r.size and l.size % 2 == 0
        capi.check(self._L.okenv_set_lane_bounds(self._h, capi.ptr(l), capi.ptr(r), l.size // 2), self._h)

    def set_sensor_offset(self, off):
        capi.check(self._L.okenv_set_sensor_offset(self._h, float(off)), self._h)

    def set_stream(self, hip_stream_ptr):
        capi.check(self._L.okenv_set_stream(self._h, C.c_void_p(hip_stream_ptr)), self._h)

    def sync(self):
        capi.check(self._L.okenv_sync(self._h), self._h)

    # ---- state -----------------------------------------------------------------------------------
    def set(self, field, values):
        """values: numpy array (copied from host) or a torch device tensor of the field's dtype."""
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):
            values = np.ascontiguousarray(values, dtype=capi.FIELD_DTYPE[field])
            n = self.N * self.R if field in capi.PER_RAY else self.N
            assert values.size == n, (capi.FIELD_NAMES[field], values.size, n)
        capi.check(self._L.okenv_set_field(self._h, field, capi.ptr(values)), self._h)

    def get(self, field, out=None):
        n = self.N * self.R if field in capi.PER_RAY else self.N
        if out is None:
            out = np.zeros(n, dtype=capi.FIELD_DTYPE[field])
        capi.check(self._L.okenv_get_field(self._h, field, capi.ptr(out)), self._h)
        if isinstance(out, np.ndarray) and field in capi.PER_RAY:
            return out.reshape(self.N, self.R)
        return out

    def snapshot(self):
        return {capi.FIELD_NAMES[f]: self.get(f) for f in range(19)}

    def set_actions(self, throttle, steer):
        if isinstance(throttle, np.ndarray) or not hasattr(throttle, "data_ptr"):
            throttle = np.ascontiguousarray(throttle, dtype=np.float32)
            steer = np.ascontiguousarray(steer, dtype=np.float32)
        capi.check(self._L.okenv_set_actions(self._h, capi.ptr(throttle), capi.ptr(steer)), self._h)

    def reset_agents(self, idx, x, y, rot_deg):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        x, y, rot = [np.ascontiguousarray(a, dtype=np.float32) for a in (x, y, rot_deg)]
        capi.check(self._L.okenv_reset_agents(self._h, capi.ptr(idx), capi.ptr(x), capi.ptr(y), capi.ptr(rot), idx.size),
                   self._h)

    def reset_random(self, idx=None, flags=capi.RESET_RANDOM_POINT, seed=0, epoch=0, agent_base=0):
        """Environment::resetAgent on the device for agents `idx` (None: all); flags = capi.RESET_*."""
        if idx is None:
            capi.check(self._L.okenv_reset_random(self._h, None, 0, int(flags), int(seed), int(epoch), int(agent_base)),
                       self._h)
            return
        if isinstance(idx, np.ndarray) or not hasattr(idx, "data_ptr"):
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            n = idx.size
        else:
            n = idx.numel()
        capi.check(self._L.okenv_reset_random(self._h, capi.ptr(idx), int(n), int(flags), int(seed), int(epoch),
                                              int(agent_base)), self._h)

    def set_auto_reset(self, enabled, flags=capi.RESET_RANDOM_POINT, seed=0, agent_base=0):
        """While on, every step begins by re-placing the agents whose crashed_ flag is set (include/okenv.h)."""
        capi.check(self._L.okenv_set_auto_reset(self._h, int(bool(enabled)), int(flags), int(seed), int(agent_base)),
                   self._h)

    @property
    def step_count(self):
        v = C.c_uint32()
        capi.check(self._L.okenv_get_step_count(self._h, C.byref(v)), self._h)
        return v.value

    @step_count.setter
    def step_count(self, value):
        capi.check(self._L.okenv_set_step_count(self._h, int(value)), self._h)

    # ---- rollout bookkeeping of the CMA-ES / PPO style callers (include/okenv.h) -----------------------------
    def tracker_create(self, reward_kind):
        capi.check(self._L.okenv_tracker_create(self._h, int(reward_kind)), self._h)

    def tracker_begin(self):
        capi.check(self._L.okenv_tracker_begin(self._h), self._h)

    def tracker_update(self):
        capi.check(self._L.okenv_tracker_update(self._h), self._h)

    # ---- CMA-ES controllers ---------------------------------------------
    def controller_create(self, hidden=16):
        """Controller.cpp:3-23 for every agent: rays -> hidden -> hidden / 2 -> 2, tanh; returns the parameter count."""
        capi.check(self._L.okenv_controller_create(self._h, int(hidden)), self._h)
        n = C.c_int32()
        capi.check(self._L.okenv_controller_num_params(self._h, C.byref(n)), self._h)
        return int(n.value)

    def controller_set_params(self, params):
        """params [N, num_params]: numpy float32 array or a torch device tensor (torch parameters() order)."""
        if isinstance(params, np.ndarray) or not hasattr(params, "data_ptr"):
            params = np.ascontiguousarray(params, dtype=np.float32)
        capi.check(self._L.okenv_controller_set_params(self._h, capi.ptr(params)), self._h)

    def controller_act(self, throttle=100.0, steering_scale=5.0):
        """CmaEsAgent::updateAction for every agent (main_eigen.cpp:58-68)."""
        capi.check(self._L.okenv_controller_act(self._h, float(throttle), float(steering_scale)), self._h)

    def rollout_controller(self, n_steps, throttle=100.0, steering_scale=5.0):
        """n_steps iterations of the CMA-ES racers' inner loop (controller, Environment::step, fitness bookkeeping) in one launch."""
        capi.check(self._L.okenv_rollout_controller(self._h, int(n_steps), float(throttle), float(steering_scale)), self._h)

    def tracker_snapshot(self):
        return {capi.FIELD_NAMES[f]: self.get(f) for f in range(capi.F_REWARD, capi.F_EPISODE_RETURN + 1)}

    def field_device_ptr(self, field):
        """(address, bytes) of a library-owned device array; see okenv_field_device_ptr."""
        p, b = C.c_void_p(), C.c_uint64()
        capi.check(self._L.okenv_field_device_ptr(self._h, int(field), C.byref(p), C.byref(b)), self._h)
        return p.value, b.value

    def hits(self):
        out = np.zeros((self.N, self.R, 2), dtype=np.float32)
        capi.check(self._L.okenv_get_hits(self._h, capi.ptr(out)), self._h)
        return out

    def distances(self):
        out = np.zeros((self.N, self.R), dtype=np.float32)
        capi.check(self._L.okenv_get_distances(self._h, capi.ptr(out)), self._h)
        return out

    def flags(self):
        out = np.zeros(self.N, dtype=np.uint8)
        capi.check(self._L.okenv_get_flags(self._h, capi.ptr(out)), self._h)
        return out

    # ---- hot path --------------------------------------------------------------------------------
    def step(self, n_steps=1):
        capi.check(self._L.okenv_step(self._h, int(n_steps)), self._h)

    def collide(self):
        capi.check(self._L.okenv_collide(self._h), self._h)

    def rollout_random(self, n_steps, seed, agent_base=0, step_base=0):
        capi.check(self._L.okenv_rollout_random(self._h, int(n_steps), int(seed), int(agent_base), int(step_base)), self._h)

    def init_bench_state(self, agent_base=0, mode=capi.MODE_VELOCITY):
        capi.check(self._L.okenv_init_bench_state(self._h, int(agent_base), int(mode)), self._h)

    def nearest_track_idx(self, qx=None, qy=None):
        if qx is None:
            out = np.zeros(self.N, dtype=np.int32)
            capi.check(self._L.okenv_nearest_track_idx(self._h, None, None, 0, capi.ptr(out)), self._h)
            return out
        qx = np.ascontiguousarray(qx, dtype=np.float32)
        qy = np.ascontiguousarray(qy, dtype=np.float32)
        out = np.zeros(qx.size, dtype=np.int32)
        capi.check(self._L.okenv_nearest_track_idx(self._h, capi.ptr(qx), capi.ptr(qy), qx.size, capi.ptr(out)), self._h)
        return out

    # ---- EvolutionaryRacer on the device (include/okenv.h) -------------------------------------------------
    def policy_mlp_create(self, hidden=30, seed=1234, agent_base=0):
        capi.check(self._L.okenv_policy_mlp_create(self._h, int(hidden), int(seed), int(agent_base)), self._h)
        self.weights_per_agent = self._L.okenv_policy_mlp_weights_per_agent(self._h)

    def policy_weights(self):
        out = np.zeros((self.N, self.weights_per_agent), dtype=np.float32)
        capi.check(self._L.okenv_policy_mlp_get_weights(self._h, capi.ptr(out)), self._h)
        return out

    def set_policy_weights(self, w):
        if isinstance(w, np.ndarray):
            w = np.ascontiguousarray(w, dtype=np.float32)
        capi.check(self._L.okenv_policy_mlp_set_weights(self._h, capi.ptr(w)), self._h)

    def rollout_policy(self, n_steps):
        capi.check(self._L.okenv_rollout_policy(self._h, int(n_steps)), self._h)

    def alive_count(self):
        n = C.c_int32()
        capi.check(self._L.okenv_alive_count(self._h, C.byref(n)), self._h)
        return n.value

    # ---- episodes: step everybody until every agent has crashed, at the cost of the agents still alive (include/okenv.h) ----
    def episode_begin(self):
        capi.check(self._L.okenv_episode_begin(self._h), self._h)

    def episode_compact(self):
        """(agents alive, agents still stepped) -- also shrinks the grid of the next rollouts to the latter."""
        alive, listed = C.c_int32(), C.c_int32()
        capi.check(self._L.okenv_episode_compact(self._h, C.byref(alive), C.byref(listed)), self._h)
        return alive.value, listed.value

    def episode_tail_limit(self):
        """Longest list that is stepped one agent per workgroup (okenv_episode_tail_limit): from there on one rollout call may ask
        for all remaining steps."""
        n = C.c_int32()
        capi.check(self._L.okenv_episode_tail_limit(self._h, C.byref(n)), self._h)
        return n.value

    def episode_end(self):
        """(steps of the reference's loop, live agent-steps); leaves the state as that loop leaves it."""
        steps, live = C.c_int32(), C.c_uint64()
        capi.check(self._L.okenv_episode_end(self._h, C.byref(steps), C.byref(live)), self._h)
        return steps.value, live.value

    def off_grid_count(self):
        """(alive, all) agents outside the raycast grid's box: escaped through the boundaries, nothing left in sensor range."""
        a, b = C.c_int32(0), C.c_int32(0)
        capi.check(self._L.okenv_off_grid_count(self._h, C.byref(a), C.byref(b)), self._h)
        return int(a.value), int(b.value)

    def reset_all(self, x, y, rot_deg):
        capi.check(self._L.okenv_reset_all(self._h, float(x), float(y), float(rot_deg)), self._h)

    def ga_scores(self, out=None):
        if out is None:
            out = np.zeros(self.N, dtype=np.float32)
        capi.check(self._L.okenv_ga_scores(self._h, capi.ptr(out)), self._h)
        return out

    def ga_scores_into(self, device_tensor):
        """assignScores straight into a float32 CUDA tensor of N elements (device-to-device, on this handle's stream): the
        fitness vector never visits the host on its way into the per-generation all-gather."""
        assert device_tensor.is_cuda and device_tensor.is_contiguous() and device_tensor.numel() == self.N
        assert str(device_tensor.dtype) == "torch.float32"
        capi.check(self._L.okenv_ga_scores(self._h, C.c_void_p(device_tensor.data_ptr())), self._h)
        return device_tensor

    def ga_select_mate(self, seed, generation, agent_base=0):
        parents = np.zeros(5, dtype=np.int32)
        capi.check(self._L.okenv_ga_select_mate(self._h, int(seed), int(generation), int(agent_base), capi.ptr(parents)), self._h)
        return parents

    # ---- RLRacers/Q_Learning on the device (include/okenv.h) -------------------------------------------------
    def q_create(self):
        capi.check(self._L.okenv_q_create(self._h), self._h)

    def q_begin_episode(self, reset_idx):
        capi.check(self._L.okenv_q_begin_episode(self._h, int(reset_idx)), self._h)

    def rollout_q(self, n_steps, epsilon, seed, agent_base=0, step_base=0):
        capi.check(self._L.okenv_rollout_q(self._h, int(n_steps), float(epsilon), int(seed), int(agent_base), int(step_base)), self._h)

    def q_table(self):
        out = np.zeros((self.N, 243, 3), dtype=np.float32)
        capi.check(self._L.okenv_q_get_table(self._h, capi.ptr(out)), self._h)
        return out

    def set_q_table(self, table):
        t = np.ascontiguousarray(table, dtype=np.float32)
        capi.check(self._L.okenv_q_set_table(self._h, capi.ptr(t)), self._h)

    def q_state(self):
        s, a, p = (np.zeros(self.N, dtype=np.int32) for _ in range(3))
        capi.check(self._L.okenv_q_get_state(self._h, capi.ptr(s), capi.ptr(a), capi.ptr(p)), self._h)
        return s, a, p

    def q_table_sums(self):
        s, c = np.zeros(729, dtype=np.float32), np.zeros(729, dtype=np.float32)
        capi.check(self._L.okenv_q_table_sums(self._h, capi.ptr(s), capi.ptr(c)), self._h)
        return s, c

    def q_assign_mean(self, sums, counts):
        s = np.ascontiguousarray(sums, dtype=np.float32)
        c = np.ascontiguousarray(counts, dtype=np.float32)
        capi.check(self._L.okenv_q_assign_mean(self._h, capi.ptr(s), capi.ptr(c)), self._h)

    def q_share_knowledge(self):
        capi.check(self._L.okenv_q_share_knowledge(self._h), self._h)

    # ---- bird's-eye camera views (include/okenv.h) ------------------------------------------------
    def render_create(self, track, width=96, height=96, samples=1, fmt=capi.VIEW_RGBA8,
                      flags=capi.VIEW_DRAW_AGENT | capi.VIEW_DRAW_HEADING, view=None, radius=9.0, agent_rgb=(80, 80, 80)):
        """Set up okenv_render_views for the bands of `track` (a Track): every agent's view, width x height pixels of
        samples x samples samples each, over `view` = (view_w, view_h) world px (default: the reference's follow camera)."""
        d = capi.OkenvViewDesc()
        d.width, d.height, d.samples, d.format, d.flags = int(width), int(height), int(samples), int(fmt), int(flags)
        d.view_w, d.view_h = (capi.VIEW_FOLLOW_W, capi.VIEW_FOLLOW_H) if view is None else (float(view[0]), float(view[1]))
        d.radius = float(radius)
        d.agent_rgb[:] = [int(c) for c in agent_rgb]
        bounds = [np.ascontiguousarray(b, dtype=np.float32) for b in (track.li, track.lo, track.ri, track.ro)]
        capi.check(self._L.okenv_render_create(self._h, *(capi.ptr(b) for b in bounds), bounds[0].size // 2, C.byref(d)), self._h)
        self.render_shape = (self.N, int(height), int(width)) + ((4,) if fmt == capi.VIEW_RGBA8 else ())

    def render_views(self, dst):
        """Every agent's view into the device tensor `dst` (contiguous uint8, >= N*H*W*C bytes), enqueued on the handle's
        stream without a synchronisation."""
        assert dst.is_contiguous()
        capi.check(self._L.okenv_render_views(self._h, C.c_void_p(dst.data_ptr()), dst.numel() * dst.element_size()), self._h)
        return dst

    def render_info(self):
        i = capi.OkenvRenderInfo()
        capi.check(self._L.okenv_render_get_info(self._h, C.byref(i)), self._h)
        return {k: getattr(i, k) for k, _ in capi.OkenvRenderInfo._fields_}

    # ---- expert drivers (include/okenv.h) ---------------------------------------------------------
    def expert_create(self, kind="potfield", **params):
        """Attaches the reference's potential-field ("potfield") or vector-field-histogram ("vfh") driver to the handle;
        params: the members of okenv_expert_params (capi.expert_params lists them with the reference's defaults)."""
        ep = capi.expert_params(kind, **params)
        capi.check(self._L.okenv_expert_create(self._h, C.byref(ep)), self._h)
        return ep

    def expert_act(self, record=None):
        """updateAction for every agent, enqueued on the handle's stream without a synchronisation.  record: None, or a dict of
        device tensors / addresses under "action" [N,2], "dist" [N,R], "rel_xy" [N,R,2] (float32) and "alive" [N] (uint8), each
        optional, that receive this step's sample."""
        self._act("okenv_expert_act", capi.OkenvExpertRecord, record,
                  record and {"action": self.N * 8, "dist": self.N * self.R * 4, "rel_xy": self.N * self.R * 8, "alive": self.N})

    # ---- shared-network actors (include/okenv.h) ---------------------------------------------------
    def actor_create(self, hidden, actions, value_hidden=0, mode="sample", epsilon=0.0, seed=0, agent_base=0):
        """Attaches a shared-network actor (policy R -> hidden -> len(actions), optional value network R -> value_hidden -> 1)
        to the handle; actions: the table [(throttle_delta, steering_delta), ...].  Returns (policy floats, value floats)."""
        ap = capi.actor_params(hidden, actions, value_hidden, mode, epsilon, seed, agent_base)
        capi.check(self._L.okenv_actor_create(self._h, C.byref(ap)), self._h)
        self.actor_params = ap
        return self.actor_num_params()

    def actor_num_params(self):
        return self._count("okenv_actor_num_params", outs=2)

    def actor_set_params(self, policy=None, value=None):
        """New parameter vectors (torch's parameters() order, flattened) from float32 numpy arrays or device tensors; None
        leaves a network as it is.  Enqueued on the handle's stream, no synchronisation for device tensors."""
        self._set_params("okenv_actor_set_params", (policy, value), self.actor_num_params())

    # (one implementation for the families that attach a network to the handle -- actor, ddpg, gauss, gcl, lidar, flow, bev: `symbol` is
    # the family's entry, `lead` what it takes between the handle and the arguments named here)
    def _count(self, symbol, *lead, outs=1):
        """The floats an okenv_*_num_params entry reports: an int, or a tuple of `outs` of them."""
        n = [C.c_int32() for _ in range(outs)]
        capi.check(getattr(self._L, symbol)(self._h, *lead, *(C.byref(v) for v in n)), self._h)
        return n[0].value if outs == 1 else tuple(v.value for v in n)

    def _set_params(self, symbol, vectors, counts, *lead):
        """Parameter vectors to an okenv_*_set_params entry, each checked by _flat_params.  The entry only enqueues its copies and a host
        buffer must stay valid until the stream has passed them, so a call that handed over a numpy array waits for the stream."""
        keep = [_flat_params(v, n) for v, n in zip(vectors, counts)]
        capi.check(getattr(self._L, symbol)(self._h, *lead, *(capi.ptr(v) for v in keep)), self._h)
        if any(isinstance(v, np.ndarray) for v in keep):
            self.sync()  # the host arrays are temporaries

    def _get_state(self, symbol, counts, out=None, struct=None, lead=()):
        """Vectors read back through an okenv_*_get_state / _get_params entry, which waits for the stream.  counts: {name: floats}, the
        float32 numpy arrays made when `out` (a dict of device tensors, any subset) is None; struct: the entry's state struct, whose t the
        result carries, or None for an entry that takes the pointer of the one vector "params"."""
        if out is None:
            out = {k: np.empty(n, dtype=np.float32) for k, n in counts.items()}
        if struct is None:
            capi.check(getattr(self._L, symbol)(self._h, *lead, capi.ptr(out["params"])), self._h)
            return out
        st = capi.fill_pointers(struct(), out, "state")
        capi.check(getattr(self._L, symbol)(self._h, *lead, C.byref(st)), self._h)
        return dict(out, t=int(st.t))

    def _set_draw_offset(self, symbol, word):
        capi.check(getattr(self._L, symbol)(self._h, capi.ptr(word)), self._h)

    def _act(self, symbol, struct, record, sizes, *lead):
        """An okenv_*_act entry, enqueued without a synchronisation.  record: None or the dict of device tensors / addresses that fills
        `struct`; sizes: the bytes each slot must hold (callers pass `record and {...}`, which builds it only for a record)."""
        rec = None if record is None else C.byref(capi.fill_pointers(struct(), record, "record", sizes))
        capi.check(getattr(self._L, symbol)(self._h, *lead, rec), self._h)

    def actor_set_epsilon(self, epsilon):
        capi.check(self._L.okenv_actor_set_epsilon(self._h, float(epsilon)), self._h)

    def actor_set_draw_offset(self, word=None):
        """A device uint32 word (tensor or address) added to the draw index of every later actor_act; None removes it."""
        self._set_draw_offset("okenv_actor_set_draw_offset", word)

    def actor_act(self, record=None):
        """updateAction of the shared-network agents for every agent, enqueued on the handle's stream without a synchronisation.
        record: None, or a dict of device tensors / addresses under "state" [N,R] float32, "action" [N] int64, "prob" [N] float32,
        "value" [N] float32 and "alive" [N] uint8, each optional, that receive this step's sample."""
        self._act("okenv_actor_act", capi.OkenvActorRecord, record,
                  record and {"state": self.N * self.R * 4, "action": self.N * 8, "prob": self.N * 4, "value": self.N * 4, "alive": self.N})

    # ---- from a recorded episode to the learner's batch (include/okenv.h) ---------------------------
    def batch_prepare(self, num_steps, num_agents, inputs, outputs, state_width=0, record_stride=0, field_stride=0, gamma=0.99, lam=1.0,
                      normalize=0, block_threads=0):
        """okenv_batch_prepare: enqueues the five kernels on the handle's stream, no synchronisation.  inputs: dict of device tensors
        / addresses under "reward", "alive" (required), "value", "last_value", "state", "action", "prob"; outputs: likewise under
        "state", "action", "prob", "ret", "adv", "index", "ret_plane", "adv_plane", "stats" (capi.BATCH_STATS_BYTES bytes), "count".
        Strided views are passed by their first element: the strides are the caller's to state, so the slots go through the shared
        packer (capi.fill_pointers) with strided=True, which skips its contiguity check."""
        bp = capi.OkenvBatchParams(int(num_steps), int(num_agents), int(state_width), int(record_stride), int(field_stride), float(gamma),
                                   float(lam), int(normalize), int(block_threads))
        bi = capi.fill_pointers(capi.OkenvBatchInput(), inputs, "batch", strided=True)
        bo = capi.fill_pointers(capi.OkenvBatchOutput(), outputs, "batch", strided=True)
        capi.check(self._L.okenv_batch_prepare(self._h, C.byref(bp), C.byref(bi), C.byref(bo)), self._h)

    def batch_count(self):
        """M of the latest batch_prepare; waits for the stream (the one 4-byte read the caller needs to size its views)."""
        m = C.c_int32()
        capi.check(self._L.okenv_batch_count(self._h, C.byref(m)), self._h)
        return m.value

    def batch_timing(self):
        """Device microseconds of the five kernels of the latest batch_prepare that ran with set_timing(True), by capi.BATCH_KERNELS."""
        return self._timing("okenv_debug_batch_timing", capi.BATCH_KERNELS)

    def _timing(self, symbol, names):
        """One device time in microseconds per name from an okenv_debug_*_timing entry (which gives milliseconds)."""
        ms = (C.c_double * len(names))()
        capi.check(getattr(self._L, symbol)(self._h, C.cast(ms, C.c_void_p)), self._h)
        return {k: 1000.0 * v for k, v in zip(names, ms)}

    # ---- PPO's update (include/okenv.h) -------------------------------------------------------------
    def learner_create(self, lr=3e-4, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8):
        """Attaches Adam state (m = v = 0, t = 0) for the networks of the handle's actor, which must have their parameters."""
        lp = capi.learner_params(lr, clip, beta1, beta2, eps)
        capi.check(self._L.okenv_learner_create(self._h, C.byref(lp)), self._h)
        self.learner_params = lp

    def learner_reset(self):
        capi.check(self._L.okenv_learner_reset(self._h), self._h)

    def ppo_update(self, batch, M, B, epochs=1, order=None, out=None):
        """okenv_ppo_update: enqueues every minibatch of every epoch on the handle's stream (two kernels each), no synchronisation.
        batch: dict of device tensors / addresses under "state" [M,R] float32, "action" [M] int64, "prob" [M] float32 (the recorded
        probability), "ret" [M] float32 and optionally "adv" [M]; order: None or a device int32 tensor [epochs, M]; out: None or a dict
        under "actor_loss", "critic_loss" (float32), "clipped" (int32), each [epochs * ceil(M / B)], "grad_policy", "grad_value"."""
        pb = capi.fill_pointers(capi.OkenvPpoBatch(), batch, "ppo batch")
        po = capi.fill_pointers(capi.OkenvPpoOutput(), out or {}, "ppo output")
        capi.check(self._L.okenv_ppo_update(self._h, C.byref(pb), int(M), int(B), int(epochs), capi.ptr(order), C.byref(po)), self._h)

    def actor_get_params(self, policy=True, value=True, out=None):
        """The actor's current parameter vectors as float32 numpy arrays (policy, value) -- None for one that is not asked for or not
        there -- or, with out=(policy tensor or None, value tensor or None), copied into those device tensors.  Synchronises."""
        n_policy, n_value = self.actor_num_params()
        if out is None:
            out = (np.empty(n_policy, dtype=np.float32) if policy else None, np.empty(n_value, dtype=np.float32) if value and n_value else None)
        capi.check(self._L.okenv_actor_get_params(self._h, capi.ptr(out[0]), capi.ptr(out[1])), self._h)
        return out

    def learner_state(self):
        """Adam's moments and step number: dict of float32 numpy arrays policy_m, policy_v, value_m, value_v (empty without a critic)
        and the int t.  Synchronises."""
        n_policy, n_value = self.actor_num_params()
        arrs = [np.empty(n, dtype=np.float32) for n in (n_policy, n_policy, n_value, n_value)]
        t = C.c_int64()
        capi.check(self._L.okenv_learner_get_state(self._h, *[capi.ptr(a) if a.size else None for a in arrs], C.byref(t)), self._h)
        return dict(zip(("policy_m", "policy_v", "value_m", "value_v"), arrs), t=t.value)

    def update_timing(self):
        """Device microseconds of the latest ppo_update that ran with set_timing(True), summed over its minibatches, by
        capi.UPDATE_KERNELS."""
        return self._timing("okenv_debug_update_timing", capi.UPDATE_KERNELS)

    # ---- REINFORCE (include/okenv.h) ----------------------------------------------------------------
    def actor_set_dropout(self, p, seed=0):
        """Dropout with probability p in [0, 1) on the hidden layer of the actor's policy network, masks keyed by `seed`; 0 switches it
        off, and so does a new actor_create.  While it is on, ppo_update and dqn_update refuse."""
        capi.check(self._L.okenv_actor_set_dropout(self._h, float(p), int(seed) & 0xFFFFFFFF), self._h)

    def reinforce_update(self, batch, M, B, accumulate=True, reduce="sum", num_agents=0, draw_first=0, order=None, out=None):
        """okenv_reinforce_update: enqueues every slice on the handle's stream (two kernels each), no synchronisation.  batch: dict of
        device tensors / addresses under "state" [M,R] float32, "action" [M] int64, "ret" [M] float32 and "index" [M] int32 (needed
        with dropout on, together with num_agents and draw_first); order: None or a device int32 tensor [M]; out: None or a dict under
        "loss" (float32, one per optimiser step) and "grad_policy"."""
        cfg = capi.reinforce_config(accumulate, reduce, num_agents, draw_first)
        rb = capi.fill_pointers(capi.OkenvReinforceBatch(), batch, "reinforce batch")
        ro = capi.fill_pointers(capi.OkenvReinforceOutput(), out or {}, "reinforce output")
        capi.check(self._L.okenv_reinforce_update(self._h, C.byref(cfg), C.byref(rb), int(M), int(B), capi.ptr(order), C.byref(ro)), self._h)

    def reinforce_timing(self):
        """Device microseconds of the latest reinforce_update that ran with set_timing(True), summed over its slices, by
        capi.REINFORCE_KERNELS."""
        return self._timing("okenv_debug_reinforce_timing", capi.REINFORCE_KERNELS)

    # ---- Deep-Q learning (include/okenv.h) ----------------------------------------------------------
    def replay_create(self, capacity, push_all=False):
        """Attaches a replay ring of `capacity` transitions (state, next_state [C,R], action, reward, done [C]) to the handle; an
        earlier one is dropped and its memory freed: a HIP graph that captured replay_push before this call must not be replayed again
        (VectorEnvironment.enable_replay drops the ones it keeps).  push_all: push every agent, not only those that entered the step
        alive."""
        self._ring_create(_DQN_RING, capacity, push_all)

    def replay_reset(self):
        self._ring_call(_DQN_RING, "reset")

    def replay_push(self, record, reward=None):
        """Appends the transitions of the step that has just run: `record` is the dict the preceding actor_act was given ("state",
        "action" and, unless push_all, "alive"); reward: None (the clearance rule) or a device float32 tensor [N].  Two kernels on
        the handle's stream, no synchronisation."""
        self._ring_push(_DQN_RING, record, reward)

    def replay_size(self):
        """(transitions in the ring, transitions ever pushed); waits for the stream."""
        return self._ring_size(_DQN_RING)

    def replay_get(self, out=None):
        """The ring's fields, all `capacity` slots: numpy arrays, or copied into the device tensors of the dict `out`.  Synchronises."""
        return self._ring_get(_DQN_RING, out)

    # (one implementation for Deep-Q's ring and DDPG's: `kind` is _DQN_RING or _DDPG_RING)
    def _ring_call(self, kind, op, *args):
        capi.check(getattr(self._L, "%s_%s" % (kind.prefix, op))(self._h, *args), self._h)

    def _ring_create(self, kind, capacity, push_all):
        self._ring_call(kind, "create", int(capacity), capi.REPLAY_PUSH_ALL if push_all else 0)
        setattr(self, kind.capacity_attr, int(capacity))

    def _ring_push(self, kind, record, reward):
        rec = capi.fill_pointers(kind.record_struct(), {k: v for k, v in record.items() if k in ("state", "action", "alive")}, "record")
        self._ring_call(kind, "push", C.byref(rec), capi.ptr(reward))

    def _ring_size(self, kind):
        size, pushed = C.c_int64(), C.c_int64()
        self._ring_call(kind, "size", C.byref(size), C.byref(pushed))
        return size.value, pushed.value

    def _ring_get(self, kind, out):
        if out is None:
            out = {k: v for k, v in _host_ring(kind, getattr(self, kind.capacity_attr), self.R, np.empty).items() if k != "pushed"}
        self._ring_call(kind, "get", C.byref(_ring_struct(kind, out)))
        return out

    def dqn_params(self, gamma=0.99, mask_done=False, target_network=False, seed=0):
        cfg = capi.dqn_config(gamma, mask_done, target_network, seed)
        capi.check(self._L.okenv_dqn_params(self._h, C.byref(cfg)), self._h)
        self.dqn_config = cfg

    def dqn_sync_target(self):
        capi.check(self._L.okenv_dqn_sync_target(self._h), self._h)

    def dqn_update(self, B, iterations, resample=False, draw_base=0, out=None):
        """okenv_dqn_update: `iterations` gradient steps on batches of B uniform samples of the ring, two kernels each on the handle's
        stream, no synchronisation.  out: None or a dict of device tensors under "loss" [iterations] float32, "grad_policy", "index"
        [B] int32."""
        po = capi.fill_pointers(capi.OkenvDqnOutput(), out or {}, "dqn output")
        capi.check(self._L.okenv_dqn_update(self._h, int(B), int(iterations), 1 if resample else 0, int(draw_base) & 0xFFFFFFFF, C.byref(po)), self._h)

    def dqn_timing(self):
        """Device microseconds of the latest dqn_update that ran with set_timing(True), summed over its iterations, by
        capi.UPDATE_KERNELS."""
        return self._timing("okenv_debug_dqn_timing", capi.UPDATE_KERNELS)

    # ---- DDPG (include/okenv.h) ----------------------------------------------------------------------
    def ddpg_create(self, hidden, critic_hidden, **config):
        """Attaches a DDPG object (actor R -> hidden -> 2 ending in tanh * scale + bias, critic (R + 2) -> critic_hidden -> 1, their
        target networks and Adam state) to the handle; config: the members of okenv_ddpg_config (capi.ddpg_config lists them with the
        reference's defaults).  Returns (actor floats, critic floats)."""
        cfg = capi.ddpg_config(hidden, critic_hidden, **config)
        capi.check(self._L.okenv_ddpg_create(self._h, C.byref(cfg)), self._h)
        self.ddpg_config = cfg
        return self.ddpg_num_params()

    def ddpg_num_params(self):
        return self._count("okenv_ddpg_num_params", outs=2)

    def ddpg_set_params(self, actor=None, critic=None):
        """New online parameters (torch's parameters() order, flattened) from float32 numpy arrays or device tensors; each network
        that arrives also replaces its target network.  None leaves a network as it is."""
        self._set_params("okenv_ddpg_set_params", (actor, critic), self.ddpg_num_params())

    def ddpg_state(self, out=None):
        """The four parameter vectors, the four Adam moments (capi.DDPG_STATE_VECTORS) and the int t: float32 numpy arrays, or copied
        into the device tensors of the dict `out` (any subset).  Synchronises."""
        na, nc = self.ddpg_num_params()
        return self._get_state("okenv_ddpg_get_state", {k: nc if "critic" in k else na for k in capi.DDPG_STATE_VECTORS}, out, capi.OkenvDdpgState)

    def ddpg_set_draw_offset(self, word=None):
        """A device uint32 word (tensor or address) added to the draw index of every later ddpg_act; None removes it."""
        self._set_draw_offset("okenv_ddpg_set_draw_offset", word)

    def ddpg_act(self, record=None):
        """The continuous action of every agent, enqueued on the handle's stream without a synchronisation.  record: None, or a dict
        of device tensors / addresses under "state" [N,R] float32, "action" [N,2] float32 and "alive" [N] uint8, each optional."""
        self._act("okenv_ddpg_act", capi.OkenvDdpgRecord, record, record and {"state": self.N * self.R * 4, "action": self.N * 8, "alive": self.N})

    def ddpg_replay_create(self, capacity, push_all=False):
        """Attaches DDPG's replay ring of `capacity` transitions (action [C,2] float32); replay_create's contract."""
        self._ring_create(_DDPG_RING, capacity, push_all)

    def ddpg_replay_reset(self):
        self._ring_call(_DDPG_RING, "reset")

    def ddpg_replay_push(self, record, reward=None):
        """Appends the transitions of the step that has just run: `record` is the dict the preceding ddpg_act was given; reward:
        None (1.0 per transition) or a device float32 tensor [N].  Two kernels on the handle's stream, no synchronisation."""
        self._ring_push(_DDPG_RING, record, reward)

    def ddpg_replay_size(self):
        """(transitions in the ring, transitions ever pushed); waits for the stream."""
        return self._ring_size(_DDPG_RING)

    def ddpg_replay_get(self, out=None):
        """The ring's fields, all `capacity` slots: numpy arrays, or copied into the device tensors of the dict `out`.  Synchronises."""
        return self._ring_get(_DDPG_RING, out)

    def ddpg_update(self, B, iterations, resample=False, draw_base=0, out=None):
        """okenv_ddpg_update: `iterations` iterations on batches of B uniform samples of the ring, four kernels each on the handle's
        stream, no synchronisation.  out: None or a dict of device tensors under "critic_loss", "actor_loss" [iterations] float32,
        "grad_critic", "grad_actor", "index" [B] int32."""
        po = capi.fill_pointers(capi.OkenvDdpgOutput(), out or {}, "ddpg output")
        capi.check(self._L.okenv_ddpg_update(self._h, int(B), int(iterations), 1 if resample else 0, int(draw_base) & 0xFFFFFFFF, C.byref(po)), self._h)

    def ddpg_timing(self):
        """Device microseconds of the latest ddpg_update that ran with set_timing(True), summed over its iterations, by
        capi.DDPG_KERNELS."""
        return self._timing("okenv_debug_ddpg_timing", capi.DDPG_KERNELS)

    # ---- continuous REINFORCE (include/okenv.h) -------------------------------------------------------
    def gauss_create(self, hidden1=128, hidden2=128, **config):
        """Attaches a Gaussian actor (R -> hidden1 -> hidden2 -> 2 with a free log_std [2]) to the handle; config: the members of
        okenv_gauss_config (capi.gauss_config lists them with the reference's defaults).  Returns the floats of its parameter vector."""
        cfg = capi.gauss_config(hidden1, hidden2, **config)
        capi.check(self._L.okenv_gauss_create(self._h, C.byref(cfg)), self._h)
        self.gauss_config = cfg
        return self.gauss_num_params()

    def gauss_num_params(self):
        return self._count("okenv_gauss_num_params")

    def gauss_set_params(self, params):
        """New parameters [log_std | fc1 | fc2 | mean] (torch's parameters() order, flattened) from a float32 numpy array or a device
        tensor.  Enqueued on the handle's stream; the call waits for the stream when it was handed a numpy
        array (which may be a temporary), not for a device tensor."""
        self._set_params("okenv_gauss_set_params", (params,), (self.gauss_num_params(),))

    def gauss_state(self, out=None):
        """The parameter vector, Adam's two moments ("params", "m", "v") and the int t: float32 numpy arrays, or copied into the
        device tensors of the dict `out` (any subset).  Synchronises."""
        return self._get_state("okenv_gauss_get_state", dict.fromkeys(("params", "m", "v"), self.gauss_num_params()), out, capi.OkenvGaussState)

    def gauss_set_draw_offset(self, word=None):
        """A device uint32 word (tensor or address) added to the draw index of every later gauss_act; None removes it."""
        self._set_draw_offset("okenv_gauss_set_draw_offset", word)

    def gauss_set_greedy(self, greedy):
        capi.check(self._L.okenv_gauss_set_greedy(self._h, 1 if greedy else 0), self._h)

    def gauss_act(self, record=None):
        """The sampled (or greedy) action of every agent, enqueued on the handle's stream without a synchronisation.  record: None,
        or a dict of device tensors / addresses under "state" [N,R], "eps", "pre", "action" [N,2], "logp" [N] float32 and "alive" [N]
        uint8, each optional."""
        self._act("okenv_gauss_act", capi.OkenvGaussRecord, record, record and
                  {"state": self.N * self.R * 4, "eps": self.N * 8, "pre": self.N * 8, "action": self.N * 8, "logp": self.N * 4, "alive": self.N})

    def gauss_learner_create(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        """Adam for the Gaussian actor (the reference's learning rate, ReinforceAgent.hpp:52): moments zeroed, t = 0."""
        lp = capi.learner_params(lr, 0.0, beta1, beta2, eps)
        capi.check(self._L.okenv_gauss_learner_create(self._h, C.byref(lp)), self._h)

    def gauss_update(self, batch, M, B, accumulate=True, reduce="sum", grad="reference", order=None, out=None):
        """okenv_gauss_update: enqueues every slice on the handle's stream (two kernels each), no synchronisation.  batch: dict of device
        tensors / addresses under "state" [M,R], "eps" [M,2] (grad="reference"), "pre" [M,2] (grad="score") and "ret" [M], float32;
        order: None or a device int32 tensor [M]; out: None or a dict under "loss" (float32, one per optimiser step) and "grad"."""
        cfg = capi.gauss_update_config(accumulate, reduce, grad)
        gb = capi.fill_pointers(capi.OkenvGaussBatch(), batch, "gauss batch")
        go = capi.fill_pointers(capi.OkenvGaussOutput(), out or {}, "gauss output")
        capi.check(self._L.okenv_gauss_update(self._h, C.byref(cfg), C.byref(gb), int(M), int(B), capi.ptr(order), C.byref(go)), self._h)

    def gauss_timing(self):
        """Device microseconds of the latest gauss_update that ran with set_timing(True), summed over its slices, by capi.GAUSS_KERNELS."""
        return self._timing("okenv_debug_gauss_timing", capi.GAUSS_KERNELS)

    # ---- lidar transformer driver (include/okenv.h) -------------------------------------------------------
    def lidar_create(self, config=None, **members):
        """Attaches a lidar transformer policy to the handle; config: a capi.lidar_config(...), or its members by name (num_points
        defaults to the handle's ray count, the rest to the reference's shape).  Returns the floats of its parameter vector."""
        if config is None:
            members.setdefault("num_points", self.R)
            config = capi.lidar_config(**members)
        capi.check(self._L.okenv_lidar_create(self._h, C.byref(config)), self._h)
        self.lidar_config = config
        return self.lidar_num_params()

    def lidar_num_params(self):
        return self._count("okenv_lidar_num_params")

    def lidar_set_params(self, params):
        """New parameters (torch's parameters() order, then the positional table: capi.lidar_layout) from a float32 numpy array or a
        device tensor.  Enqueued on the handle's stream; the call waits for the stream when it was handed a numpy
        array (which may be a temporary), not for a device tensor."""
        self._set_params("okenv_lidar_set_params", (params,), (self.lidar_num_params(),))

    def lidar_get_params(self, out=None):
        """The parameter vector as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_lidar_get_params", {"params": self.lidar_num_params()}, None if out is None else {"params": out})["params"]

    def lidar_act(self, record=None):
        """The policy's action for every agent, enqueued on the handle's stream without a synchronisation.  record: None, or a dict
        of device tensors / addresses under "action" [N,2], "input" [N,R,2] float32 and "alive" [N] uint8, each optional."""
        self._act("okenv_lidar_act", capi.OkenvLidarRecord, record, record and {"action": self.N * 8, "input": self.N * self.R * 8, "alive": self.N})

    # ---- flow-matching driver (include/okenv.h) --------------------------------------------------------
    def flow_create(self, config=None, **members):
        """Attaches a flow-matching policy (the Euler sampler of the reference's ActionFlowTrunk) to the handle; config: a
        capi.flow_config(...), or its members by name (the reference's shape and ranges by default).  Returns the floats of its
        parameter vector."""
        if config is None:
            config = capi.flow_config(**members)
        capi.check(self._L.okenv_flow_create(self._h, C.byref(config)), self._h)
        self.flow_config = config
        return self.flow_num_params()

    def flow_num_params(self):
        return self._count("okenv_flow_num_params")

    def flow_set_params(self, params):
        """New parameters (the trunk's, in torch's parameters() order: capi.flow_layout) from a float32 numpy array or a device
        tensor.  Enqueued on the handle's stream; the call waits for the stream when it was handed a numpy
        array (which may be a temporary), not for a device tensor."""
        self._set_params("okenv_flow_set_params", (params,), (self.flow_num_params(),))

    def flow_get_params(self, out=None):
        """The parameter vector as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_flow_get_params", {"params": self.flow_num_params()}, None if out is None else {"params": out})["params"]

    def flow_set_draw_offset(self, word=None):
        """A device uint32 word (tensor or address) added to the draw index of every later flow_act; None removes it."""
        self._set_draw_offset("okenv_flow_set_draw_offset", word)

    def flow_act(self, cond, record=None):
        """The sampled action of every agent from its condition vector, enqueued on the handle's stream without a synchronisation.
        cond: a device tensor / address of [N, cond_dim] float32.  record: None, or a dict of device tensors / addresses under "x0",
        "x", "action" [N,2] float32 and "alive" [N] uint8, each optional."""
        self._act("okenv_flow_act", capi.OkenvFlowRecord, record, record and {"x0": self.N * 8, "x": self.N * 8, "action": self.N * 8, "alive": self.N},
                  capi.ptr(cond))

    # ---- the flow driver's image encoder (include/okenv.h) ---------------------------------------------
    def bev_create(self, config=None, **members):
        """Attaches the flow driver's image encoder (the reference's BEVEncoder) to the handle; config: a capi.bev_config(...), or
        its members by name (the reference's shape by default).  Returns the floats of its parameter vector."""
        if config is None:
            config = capi.bev_config(**members)
        capi.check(self._L.okenv_bev_create(self._h, C.byref(config)), self._h)
        self.bev_config = config
        return self.bev_num_params()

    def bev_num_params(self):
        return self._count("okenv_bev_num_params")

    def bev_set_params(self, params):
        """New parameters (the encoder's, in torch's parameters() order: capi.bev_layout) from a float32 numpy array or a device
        tensor.  Enqueued on the handle's stream; the call waits for the stream when it was handed a numpy array (which may be a
        temporary), not for a device tensor."""
        self._set_params("okenv_bev_set_params", (params,), (self.bev_num_params(),))

    def bev_get_params(self, out=None):
        """The parameter vector as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_bev_get_params", {"params": self.bev_num_params()}, None if out is None else {"params": out})["params"]

    def bev_encode(self, frames, out, stages=None):
        """The embedding of every agent's frame, enqueued on the handle's stream without a synchronisation.  frames: a device tensor
        / address of [N, S, S, 4] uint8; out: one of [N, embed_dim] float32.  stages: None, or a mask of capi.BEV_STAGE_* -- only those
        kernels (okenv_debug_bev_stages, for measurement)."""
        S = self.bev_config.image_size
        if stages is None:
            capi.check(self._L.okenv_bev_encode(self._h, capi.ptr(frames), self.N * S * S * 4, capi.ptr(out)), self._h)
        else:
            capi.check(self._L.okenv_debug_bev_stages(self._h, capi.ptr(frames), self.N * S * S * 4, capi.ptr(out), int(stages)), self._h)

    # ---- behavioural-cloning image policy (include/okenv.h) ---------------------------------------------
    def cnn_create(self, config=None, **members):
        """Attaches the behavioural-cloning image policy (the reference's PolicyCNN) to the handle; config: a capi.cnn_config(...), or
        its members by name (the reference's shape and controls by default).  Returns the floats of its parameter vector."""
        if config is None:
            config = capi.cnn_config(**members)
        capi.check(self._L.okenv_cnn_create(self._h, C.byref(config)), self._h)
        self.cnn_config = config
        return self.cnn_num_params()

    def cnn_num_params(self):
        return self._count("okenv_cnn_num_params")

    def cnn_set_params(self, params):
        """New parameters (the policy's, in torch's parameters() order: capi.cnn_layout) from a float32 numpy array or a device
        tensor.  Enqueued on the handle's stream; the call waits for the stream when it was handed a numpy array (which may be a
        temporary), not for a device tensor."""
        self._set_params("okenv_cnn_set_params", (params,), (self.cnn_num_params(),))

    def cnn_get_params(self, out=None):
        """The parameter vector as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_cnn_get_params", {"params": self.cnn_num_params()}, None if out is None else {"params": out})["params"]

    def cnn_act(self, frames, record=None, stages=None):
        """The policy's action of every agent from its frame, enqueued on the handle's stream without a synchronisation.  frames: a
        device tensor / address of [N, S, S, 4] uint8.  record: None, or a dict of device tensors / addresses under "out" [N],
        "action" [N,2] float32 and "alive" [N] uint8, each optional.  stages: None, or a mask of capi.CNN_STAGE_* -- only those
        kernels (okenv_debug_cnn_stages, for measurement)."""
        S = self.cnn_config.image_size
        sizes = record and {"out": self.N * 4, "action": self.N * 8, "alive": self.N}
        if stages is None:
            self._act("okenv_cnn_act", capi.OkenvCnnRecord, record, sizes, capi.ptr(frames), self.N * S * S * 4)
        else:
            rec = None if record is None else C.byref(capi.fill_pointers(capi.OkenvCnnRecord(), record, "record", sizes))
            capi.check(self._L.okenv_debug_cnn_stages(self._h, capi.ptr(frames), self.N * S * S * 4, rec, int(stages)), self._h)

    # ---- image transformer driver (include/okenv.h) ----------------------------------------------------------
    def vit_create(self, config=None, **members):
        """Attaches the image transformer policy (DinoControl's ViT and head) to the handle; config: a capi.vit_config(...), or its
        members by name (the reference's shape and controls by default).  Returns the floats of its parameter vector."""
        if config is None:
            config = capi.vit_config(**members)
        capi.check(self._L.okenv_vit_create(self._h, C.byref(config)), self._h)
        self.vit_config = config
        return self.vit_num_params()

    def vit_num_params(self):
        return self._count("okenv_vit_num_params")

    def vit_set_params(self, params):
        """New parameters (torch's parameters() order: capi.vit_layout) from a float32 numpy array or a device tensor.  Enqueued on
        the handle's stream; the call waits for the stream when it was handed a numpy array (which may be a temporary), not for a
        device tensor."""
        self._set_params("okenv_vit_set_params", (params,), (self.vit_num_params(),))

    def vit_get_params(self, out=None):
        """The parameter vector as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_vit_get_params", {"params": self.vit_num_params()}, None if out is None else {"params": out})["params"]

    def vit_act(self, frames, record=None):
        """The policy's action of every agent from its frame, enqueued on the handle's stream without a synchronisation.  frames: a
        device tensor / address of [N, S, S, 4] uint8.  record: None, or a dict of device tensors / addresses under "action" [N,2],
        "output" [N], "embedding" [N,D] float32 and "alive" [N] uint8, each optional."""
        S = self.vit_config.image_size
        sizes = record and {"action": self.N * 8, "output": self.N * 4, "embedding": self.N * self.vit_config.dim * 4, "alive": self.N}
        self._act("okenv_vit_act", capi.OkenvVitRecord, record, sizes, capi.ptr(frames), self.N * S * S * 4)

    # ---- the image transformer driver's training (include/okenv.h) -------------------------------------------
    def vit_embed(self, frames, m, out):
        """The frozen backbone over m frames (any m >= 1, not the population): frames a device tensor / address of [m, S, S, 4] uint8,
        out one of [m, D] float32.  Enqueued in passes of the act's agents_per_pass, no synchronisation; touches no agent field."""
        S = self.vit_config.image_size
        capi.check(self._L.okenv_vit_embed(self._h, capi.ptr(frames), int(m), int(m) * S * S * 4, capi.ptr(out)), self._h)

    def vit_head_num_params(self):
        c = self.vit_config
        return capi.vit_head_num_params(c.dim, c.head_hidden1, c.head_hidden2)

    def vit_head_learner_create(self, params=None, **members):
        """Adam for the policy's head (capi.vit_head_params: the reference's lr 1e-4, weight 5, threshold 0.1): moments zeroed, t = 0."""
        if params is None:
            params = capi.vit_head_params(**members)
        capi.check(self._L.okenv_vit_head_learner_create(self._h, C.byref(params)), self._h)

    def vit_head_learner_reset(self):
        capi.check(self._L.okenv_vit_head_learner_reset(self._h), self._h)

    def vit_head_state(self, out=None):
        """The head's parameters, Adam's two moments ("params", "m", "v") and the int t: float32 numpy arrays, or copied into the
        device tensors of the dict `out` (any subset).  Synchronises."""
        return self._get_state("okenv_vit_head_learner_get_state", dict.fromkeys(("params", "m", "v"), self.vit_head_num_params()), out,
                               capi.OkenvVitHeadState)

    def vit_head_update(self, embedding, steer, M, B, epochs=1, order=None, out=None):
        """okenv_vit_head_update: enqueues every minibatch of every epoch on the handle's stream (two kernels each), no synchronisation.
        embedding [M, D], steer [M]: device tensors / addresses, float32; order: None or a device int32 tensor [epochs, M]; out: None
        or a dict under "loss" (float32, one per minibatch) and "grad" (the last minibatch's)."""
        go = capi.fill_pointers(capi.OkenvVitHeadOutput(), out or {}, "vit head output")
        capi.check(self._L.okenv_vit_head_update(self._h, capi.ptr(embedding), capi.ptr(steer), int(M), int(B), int(epochs), capi.ptr(order), C.byref(go)),
                   self._h)

    def vit_head_eval(self, embedding, steer, M, B, loss):
        """okenv_vit_head_eval: the loss of every minibatch of one sequential pass into the device tensor loss [ceil(M / B)], no update."""
        capi.check(self._L.okenv_vit_head_eval(self._h, capi.ptr(embedding), capi.ptr(steer), int(M), int(B), capi.ptr(loss)), self._h)

    # ---- Deep-Q image racers (include/okenv.h) --------------------------------------------------------------
    def qcnn_create(self, config=None, **members):
        """Attaches the reference's image Q-network (RLRacers/DQN_CNN: CNN.hpp) to the handle; config: a capi.qcnn_config(...), or
        its members as keywords.  Returns the floats of the parameter vector.  A frame ring of another image_size is dropped."""
        if config is None:
            config = capi.qcnn_config(**members)
        capi.check(self._L.okenv_qcnn_create(self._h, C.byref(config)), self._h)
        self.qcnn_config = config
        return self.qcnn_num_params()

    def qcnn_num_params(self):
        return self._count("okenv_qcnn_num_params")

    def qcnn_set_params(self, params):
        """New parameters (the network's, in torch's parameters() order: capi.qcnn_layout) from a float32 numpy array or a device
        tensor / address (a device-to-device copy on the handle's stream)."""
        self._set_params("okenv_qcnn_set_params", (params,), (self.qcnn_num_params(),))

    def qcnn_get_params(self, out=None):
        """The parameter vector as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_qcnn_get_params", {"params": self.qcnn_num_params()}, None if out is None else {"params": out})["params"]

    def qcnn_set_epsilon(self, epsilon):
        capi.check(self._L.okenv_qcnn_set_epsilon(self._h, float(epsilon)), self._h)
        self.qcnn_config.epsilon = float(epsilon)

    def qcnn_set_draw_offset(self, word=None):
        """A device uint32 word (tensor or address) added to the draw index of every later qcnn_act; None removes it."""
        self._set_draw_offset("okenv_qcnn_set_draw_offset", word)

    def _qcnn_frame_bytes(self):
        return self.N * self.qcnn_config.image_size ** 2 * 4

    def qcnn_act(self, frames, record=None, stages=None):
        """The Q-network's greedy or epsilon-greedy action of every agent from `frames`, a device uint8 tensor / address
        [N][S][S][4], enqueued on the handle's stream without a synchronisation.  record: None, or a dict of device tensors /
        addresses under "q" [N,A] float32, "action" [N] int64, "value" [N] float32 and "alive" [N] uint8, each optional.  stages: None
        for the act, or a sum of capi.QCNN_STAGE_* to run only those kernels (okenv_debug_qcnn_stages, for measurement)."""
        A = self.qcnn_config.num_actions
        sizes = record and {"q": self.N * A * 4, "action": self.N * 8, "value": self.N * 4, "alive": self.N}
        if stages is None:
            self._act("okenv_qcnn_act", capi.OkenvQcnnRecord, record, sizes, capi.ptr(frames), self._qcnn_frame_bytes())
        else:
            rec = None if record is None else C.byref(capi.fill_pointers(capi.OkenvQcnnRecord(), record, "record", sizes))
            capi.check(self._L.okenv_debug_qcnn_stages(self._h, capi.ptr(frames), self._qcnn_frame_bytes(), rec, int(stages)), self._h)

    def qcnn_ring_create(self, capacity, push_all=False):
        """Attaches the frame ring of `capacity` transitions (state, next_state [C,S,S] float32 grey planes, action, reward, done [C]);
        an earlier one is dropped and its memory freed: a HIP graph that captured qcnn_push before this call must not be replayed."""
        capi.check(self._L.okenv_qcnn_ring_create(self._h, int(capacity), capi.REPLAY_PUSH_ALL if push_all else 0), self._h)
        self.qcnn_ring_capacity = int(capacity)

    def qcnn_ring_reset(self):
        capi.check(self._L.okenv_qcnn_ring_reset(self._h), self._h)

    def qcnn_ring_size(self):
        """(transitions in the ring, transitions ever pushed); waits for the stream."""
        size, pushed = C.c_int64(), C.c_int64()
        capi.check(self._L.okenv_qcnn_ring_size(self._h, C.byref(size), C.byref(pushed)), self._h)
        return size.value, pushed.value

    def qcnn_ring_get(self, out=None):
        """The ring's fields, all `capacity` slots: numpy arrays, or copied into the device tensors of the dict `out`.  Synchronises."""
        if out is None:
            out = {k: v for k, v in capi.qcnn_ring(self.qcnn_ring_capacity, self.qcnn_config.image_size).items() if isinstance(v, np.ndarray)}
        capi.check(self._L.okenv_qcnn_ring_get(self._h, C.byref(capi.fill_pointers(capi.OkenvQcnnRing(), out, "ring"))), self._h)
        return out

    def qcnn_push(self, record, frames, next_frames, reward=None):
        """Appends the transitions of the step that has just run: `record` is the dict the preceding qcnn_act was given ("action" and,
        unless push_all, "alive"), `frames` what that act saw, `next_frames` the camera after the step; reward: None (the clearance
        rule) or a device float32 tensor [N].  Three kernels on the handle's stream, no synchronisation."""
        rec = capi.fill_pointers(capi.OkenvQcnnRecord(), {k: v for k, v in record.items() if k in ("action", "alive")}, "record")
        capi.check(self._L.okenv_qcnn_push(self._h, C.byref(rec), capi.ptr(frames), capi.ptr(next_frames), self._qcnn_frame_bytes(), capi.ptr(reward)),
                   self._h)

    def qcnn_batch(self, B, out, mode="sequential", start_or_draw=0):
        """B positions of the ring into the device tensors of the dict `out` ("state", "next_state" [B,S,S] float32, "action" [B]
        int64, "reward", "done" [B] float32, "index" [B] int32, each optional): mode "uniform" (start_or_draw: the draw index) or
        "sequential" (the walk's start).  One kernel on the handle's stream, no synchronisation."""
        S = self.qcnn_config.image_size
        sizes = {"state": B * S * S * 4, "next_state": B * S * S * 4, "action": B * 8, "reward": B * 4, "done": B * 4, "index": B * 4}
        o = capi.fill_pointers(capi.OkenvQcnnBatchOut(), out, "batch", sizes)
        capi.check(self._L.okenv_qcnn_batch(self._h, int(B), capi.QCNN_BATCH_MODES.get(mode, mode), int(start_or_draw), C.byref(o)), self._h)

    # ---- world-model racers (include/okenv.h) --------------------------------------------------------------
    def world_create(self, config=None, **members):
        """Attaches the world-model racers (the reference's conv-VAE encoder and one controller per agent) to the handle; config: a
        capi.world_config(...), or its members by name (the reference's shape and controls by default).  Returns (floats of the
        encoder vector, floats of one agent's controller)."""
        if config is None:
            config = capi.world_config(**members)
        capi.check(self._L.okenv_world_create(self._h, C.byref(config)), self._h)
        self.world_config = config
        return self.world_num_params()

    def world_num_params(self):
        return self._count("okenv_world_num_params", outs=2)

    def _world_floats(self, which):
        ne, nc = self.world_num_params()
        return ne if capi.WORLD_VECTORS[which] == capi.WORLD_ENCODER else self.N * nc

    def world_set_params(self, which, params):
        """New parameters, which: "encoder" (the shared vector, capi.world_layout) or "controllers" ([N, controller], one row per
        agent), from a float32 numpy array or a device tensor.  Enqueued on the handle's stream; the call waits for the stream when
        it was handed a numpy array (which may be a temporary), not for a device tensor."""
        self._set_params("okenv_world_set_params", (params,), (self._world_floats(which),), capi.WORLD_VECTORS[which])

    def world_get_params(self, which, out=None):
        """The vector `which` as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_world_get_params", {"params": self._world_floats(which)}, None if out is None else {"params": out},
                               lead=(capi.WORLD_VECTORS[which],))["params"]

    def world_act(self, frames, record=None, stages=None):
        """Every agent's action from its frame and its own controller, enqueued on the handle's stream without a synchronisation
        (with skip_crashed: nothing is written for crashed agents).  frames: a device tensor / address of [N, S, S, 4] uint8.  record:
        None, or a dict of device tensors / addresses under "mu" [N,Z], "state" [N,Z+2], "out" [N], "action" [N,2] float32 and "alive"
        [N] uint8, each optional.  stages: None, or a mask of capi.WORLD_STAGE_* -- only those kernels (okenv_debug_world_stages)."""
        S, Z = self.world_config.image_size, self.world_config.latent
        sizes = record and {"mu": self.N * Z * 4, "state": self.N * (Z + 2) * 4, "out": self.N * 4, "action": self.N * 8, "alive": self.N}
        if stages is None:
            self._act("okenv_world_act", capi.OkenvWorldRecord, record, sizes, capi.ptr(frames), self.N * S * S * 4)
        else:
            rec = None if record is None else C.byref(capi.fill_pointers(capi.OkenvWorldRecord(), record, "record", sizes))
            capi.check(self._L.okenv_debug_world_stages(self._h, capi.ptr(frames), self.N * S * S * 4, rec, int(stages)), self._h)

    def world_set_lane_widths(self, w_left, w_right):
        """The lane widths the score divides by (Track.wl / Track.wr), one pair per centre-line point."""
        l, r = (np.ascontiguousarray(v, dtype=np.float32) for v in (w_left, w_right))
        assert l.size == r.size
        capi.check(self._L.okenv_world_set_lane_widths(self._h, capi.ptr(l), capi.ptr(r), l.size), self._h)
        self.sync()  # the host arrays are temporaries

    def world_score_begin(self):
        capi.check(self._L.okenv_world_score_begin(self._h), self._h)

    def world_score(self):
        """One step of the reference's fitness (main.cpp:329-342) for every agent: one kernel on the handle's stream."""
        capi.check(self._L.okenv_world_score(self._h), self._h)

    def world_fitness(self, out=None):
        """The fitness [N] as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        if out is None:
            out = np.empty(self.N, dtype=np.float32)
        capi.check(self._L.okenv_world_fitness(self._h, capi.ptr(out)), self._h)
        return out

    def world_fitness_device(self):
        """The device address of the fitness [N] float32, valid until the next world_create."""
        p = C.c_void_p()
        capi.check(self._L.okenv_world_fitness_device(self._h, C.byref(p)), self._h)
        return int(p.value)

    # ---- the racers' memory (include/okenv.h) ---------------------------------------------------------------
    def memory_create(self, config=None, **members):
        """Attaches the memory (the reference's GRUDynamics and one [mu | h_top] controller per agent) to the handle's world-model
        racers and zeroes every hidden state; config: a capi.memory_config(...), or its members by name.  Returns (floats of the
        network vector, floats of one agent's controller)."""
        if config is None:
            config = capi.memory_config(**members)
        capi.check(self._L.okenv_memory_create(self._h, C.byref(config)), self._h)
        self.memory_config = config
        return self.memory_num_params()

    def memory_num_params(self):
        return self._count("okenv_memory_num_params", outs=2)

    def _memory_floats(self, which):
        nn, nc = self.memory_num_params()
        return nn if capi.MEMORY_VECTORS[which] == capi.MEMORY_NETWORK else self.N * nc

    def memory_set_params(self, which, params):
        """New parameters, which: "network" (the shared vector, capi.memory_layout) or "controllers" ([N, controller]), from a float32
        numpy array or a device tensor; waits for the stream only when it was handed a numpy array."""
        self._set_params("okenv_memory_set_params", (params,), (self._memory_floats(which),), capi.MEMORY_VECTORS[which])

    def memory_get_params(self, which, out=None):
        """The vector `which` as a float32 numpy array, or copied into the device tensor `out`.  Synchronises."""
        return self._get_state("okenv_memory_get_params", {"params": self._memory_floats(which)}, None if out is None else {"params": out},
                               lead=(capi.MEMORY_VECTORS[which],))["params"]

    def memory_reset(self):
        """Zeroes every agent's hidden state: one kernel on the handle's stream."""
        capi.check(self._L.okenv_memory_reset(self._h), self._h)

    def _memory_hidden_floats(self):
        return self.N * self.memory_config.layers * self.memory_config.hidden

    def memory_set_hidden(self, hidden):
        """Every agent's hidden state [N, layers, hidden] from a float32 numpy array or a device tensor."""
        self._set_params("okenv_memory_set_hidden", (hidden,), (self._memory_hidden_floats(),))

    def memory_get_hidden(self, out=None):
        """Every agent's hidden state as a float32 numpy array [N, layers, hidden], or copied into the device tensor `out`.
        Synchronises."""
        got = self._get_state("okenv_memory_get_hidden", {"params": self._memory_hidden_floats()}, None if out is None else {"params": out})["params"]
        return got.reshape(self.N, self.memory_config.layers, self.memory_config.hidden) if out is None else got

    def memory_act(self, frames, record=None, stages=None):
        """Every agent's action from its frame, its hidden state and its own controller, enqueued on the handle's stream without a
        synchronisation (with the racers' skip_crashed nothing of a crashed agent is touched).  frames: as world_act's.  record: None,
        or a dict of device tensors / addresses under capi.MEMORY_RECORD ("mu" [N,Z], "hidden" [N,H], "prediction" [N,Z], "state"
        [N,Z+H], "out" [N], "action" [N,2] float32, "alive" [N] uint8), each optional.  stages: None, or a mask of
        capi.MEMORY_STAGE_* -- only those kernels (okenv_debug_memory_stages)."""
        S, Z, H = self.world_config.image_size, self.world_config.latent, self.memory_config.hidden
        sizes = record and {"mu": self.N * Z * 4, "hidden": self.N * H * 4, "prediction": self.N * Z * 4, "state": self.N * (Z + H) * 4,
                            "out": self.N * 4, "action": self.N * 8, "alive": self.N}
        if stages is None:
            self._act("okenv_memory_act", capi.OkenvMemoryRecord, record, sizes, capi.ptr(frames), self.N * S * S * 4)
        else:
            rec = None if record is None else C.byref(capi.fill_pointers(capi.OkenvMemoryRecord(), record, "record", sizes))
            capi.check(self._L.okenv_debug_memory_stages(self._h, capi.ptr(frames), self.N * S * S * 4, rec, int(stages)), self._h)

    # ---- the memory's training (include/okenv.h) ------------------------------------------------------
    def memory_learner_create(self, config=None, **members):
        """AdamW, clipping and the workspace of windows for the memory's network (capi.memory_learner_config: train_rnn.py's values):
        moments zeroed, t = 0.  memory_create drops it again."""
        if config is None:
            config = capi.memory_learner_config(**members)
        capi.check(self._L.okenv_memory_learner_create(self._h, C.byref(config)), self._h)
        self.memory_learner_config = config

    def memory_learner_reset(self):
        capi.check(self._L.okenv_memory_learner_reset(self._h), self._h)

    def memory_learner_state(self, out=None):
        """The network vector, Adam's two moments of its trainable prefix ("params", "m", "v") and the int t: float32 numpy arrays, or
        copied into the device tensors of the dict `out` (any subset).  Synchronises."""
        T = capi.memory_trainable(self.world_config, self.memory_config)
        return self._get_state("okenv_memory_learner_get_state", {"params": self.memory_num_params()[0], "m": T, "v": T}, out, capi.OkenvMemoryLearnerState)

    def memory_update(self, latent, action, rows, start, M, B, stride=1, epochs=1, order=None, lr_schedule=None, out=None):
        """okenv_memory_update: enqueues every minibatch of every epoch on the handle's stream, no synchronisation.  latent [rows, Z],
        action [rows, 2] float32 and start [M] int32: device tensors / addresses; order: None or a device int32 tensor [epochs, M];
        lr_schedule: None or a HOST float32 numpy array, one rate per minibatch; out: None or a dict under "loss", "norm" (float32,
        one per minibatch) and "grad" (the last minibatch's clipped gradient)."""
        go = capi.fill_pointers(capi.OkenvMemoryLearnerOutput(), out or {}, "memory learner output")
        if lr_schedule is not None:
            lr_schedule = np.ascontiguousarray(lr_schedule, np.float32)
            assert lr_schedule.size == int(epochs) * ((int(M) + int(B) - 1) // int(B)), "one rate per minibatch"
        capi.check(self._L.okenv_memory_update(self._h, capi.ptr(latent), capi.ptr(action), int(rows), capi.ptr(start), int(M), int(stride), int(B), int(epochs),
                                               capi.ptr(order), capi.ptr(lr_schedule), C.byref(go)), self._h)

    def memory_eval(self, latent, action, rows, start, M, B, loss, stride=1):
        """okenv_memory_eval: the loss of every minibatch of one sequential pass into the device tensor loss [ceil(M / B)], no step."""
        capi.check(self._L.okenv_memory_eval(self._h, capi.ptr(latent), capi.ptr(action), int(rows), capi.ptr(start), int(M), int(stride), int(B),
                                             capi.ptr(loss)), self._h)

    # ---- guided cost learning (include/okenv.h) -------------------------------------------------------
    def gcl_create(self, **config):
        """Attaches a GCL object (policy R -> H1 -> H2 -> 2 with log_std, value R -> H1 -> H2 -> 1, cost R + 2 -> C1 -> C2 -> 1) to the
        handle; config: the members of okenv_gcl_config (capi.gcl_config lists them with the reference's defaults).  Returns the floats
        of the three parameter vectors as a dict."""
        cfg = capi.gcl_config(**config)
        capi.check(self._L.okenv_gcl_create(self._h, C.byref(cfg)), self._h)
        self.gcl_config = cfg
        return {name: self.gcl_num_params(name) for name in capi.GCL_NETWORKS}

    def gcl_num_params(self, which):
        return self._count("okenv_gcl_num_params", _gcl_which(which))

    def gcl_set_params(self, which, params):
        """New parameters of network `which` ("policy" / "value" / "cost"; torch's parameters() order, flattened) from a float32 numpy
        array or a device tensor.  Enqueued on the handle's stream; the call waits for the stream when it was handed a numpy
        array (which may be a temporary), not for a device tensor."""
        self._set_params("okenv_gcl_set_params", (params,), (self.gcl_num_params(which),), _gcl_which(which))

    def gcl_state(self, which, out=None):
        """Network `which`'s parameter vector, Adam's two moments ("params", "m", "v") and the int t: float32 numpy arrays, or copied
        into the device tensors of the dict `out` (any subset).  Synchronises."""
        return self._get_state("okenv_gcl_get_state", dict.fromkeys(("params", "m", "v"), self.gcl_num_params(which)), out, capi.OkenvGclState,
                               (_gcl_which(which),))

    def gcl_set_draw_offset(self, word=None):
        """A device uint32 word (tensor or address) added to the draw index of every later gcl_act; None removes it."""
        self._set_draw_offset("okenv_gcl_set_draw_offset", word)

    def gcl_set_greedy(self, greedy):
        capi.check(self._L.okenv_gcl_set_greedy(self._h, 1 if greedy else 0), self._h)

    def gcl_act(self, record=None):
        """The sampled (or greedy) action of every agent, enqueued on the handle's stream without a synchronisation.  record: None,
        or a dict of device tensors / addresses under "state" [N,R], "eps", "pre", "squashed", "action" [N,2], "logp" [N] float32 and
        "alive" [N] uint8, each optional."""
        self._act("okenv_gcl_act", capi.OkenvGclRecord, record, record and
                  {"state": self.N * self.R * 4, "eps": self.N * 8, "pre": self.N * 8, "squashed": self.N * 8, "action": self.N * 8,
                   "logp": self.N * 4, "alive": self.N})

    def gcl_set_expert(self, state, action):
        """The expert bank from device tensors state [E,R] and action [E,2] (float32, contiguous), copied on the handle's stream."""
        E = int(state.shape[0])
        assert state.is_contiguous() and action.is_contiguous() and state.numel() == E * self.R and action.numel() == E * 2
        capi.check(self._L.okenv_gcl_set_expert(self._h, capi.ptr(state), capi.ptr(action), E), self._h)
        self._gcl_bank_inputs = (state, action)  # alive until the next hand-over: the copies are only enqueued

    def gcl_cost(self, state, squashed, out):
        """out[s] = cost([state_s | squashed_s]) for the M rows of device tensors state [M,R], squashed [M,2]; out [M] float32."""
        M = int(out.numel())
        assert state.is_contiguous() and squashed.is_contiguous() and out.is_contiguous() and state.numel() == M * self.R and squashed.numel() == M * 2
        capi.check(self._L.okenv_gcl_cost(self._h, capi.ptr(state), capi.ptr(squashed), M, capi.ptr(out)), self._h)

    def gcl_learner_create(self, lr=3e-4, clip=0.2, cost_lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
        """Adam for the three networks (the reference's learning rate and clip, GCLAgent.hpp:30-32,92): moments zeroed, t = 0."""
        lp, lc = capi.learner_params(lr, clip, beta1, beta2, eps), capi.learner_params(cost_lr, 0.0, beta1, beta2, eps)
        capi.check(self._L.okenv_gcl_learner_create(self._h, C.byref(lp), C.byref(lc)), self._h)

    def gcl_cost_update(self, batch, Mp, Me, out=None):
        """okenv_gcl_cost_update: one Adam step of the cost network on Me expert draws and the Mp policy rows of `batch` (device tensors
        "state" [Mp,R], "squashed" [Mp,2]); out: None or a dict under "loss" [1] and "grad".  No synchronisation."""
        cb = capi.fill_pointers(capi.OkenvGclCostBatch(), batch, "gcl cost batch")
        co = capi.fill_pointers(capi.OkenvGclCostOutput(), out or {}, "gcl cost output")
        capi.check(self._L.okenv_gcl_cost_update(self._h, C.byref(cb), int(Mp), int(Me), C.byref(co)), self._h)

    def gcl_policy_update(self, batch, M, B, accumulate=True, reduce="mean", order=None, out=None):
        """okenv_gcl_policy_update: the advantages, then the policy's and the value's slices on the handle's stream, no synchronisation.
        batch: dict of device tensors "state" [M,R], "pre" [M,2], "logp" [M], "ret" [M], float32; order: None or a device int32 tensor
        [M]; out: None or a dict under "policy_loss", "value_loss" (float32, one per optimiser step), "clipped" (int32 likewise),
        "grad_policy", "grad_value" and "adv" [M]."""
        cfg = capi.gcl_update_config(accumulate, reduce)
        gb = capi.fill_pointers(capi.OkenvGclBatch(), batch, "gcl batch")
        go = capi.fill_pointers(capi.OkenvGclOutput(), out or {}, "gcl output")
        capi.check(self._L.okenv_gcl_policy_update(self._h, C.byref(cfg), C.byref(gb), int(M), int(B), capi.ptr(order), C.byref(go)), self._h)

    def gcl_timing(self, which):
        """Device microseconds of network `which`'s kernels in the latest update that ran with set_timing(True), by capi.GCL_KERNELS."""
        out = (C.c_double * 2)()
        capi.check(self._L.okenv_debug_gcl_timing(self._h, _gcl_which(which), out), self._h)
        return {name: out[k] * 1e3 for k, name in enumerate(capi.GCL_KERNELS)}

    # ---- measurement / self-checks ------------------------------------------------------------------
    def work_stats(self):
        """{rays, tests, cells, points} the broad phase leaves for the current poses (okenv_work_stats)."""
        out = np.zeros(4, dtype=np.uint64)
        capi.check(self._L.okenv_work_stats(self._h, capi.ptr(out)), self._h)
        return dict(zip(("rays", "tests", "cells", "points"), (int(v) for v in out)))

    def work_stats_split(self):
        """The same for the walk with the front / back split, as the step kernels make it (okenv_work_stats_split): front and back
        walks together, plus the rays of a certified origin, the ambiguous front walks and the rays that walked the back image."""
        out = np.zeros(8, dtype=np.uint64)
        capi.check(self._L.okenv_work_stats_split(self._h, capi.ptr(out)), self._h)
        return dict(zip(("rays", "tests", "cells", "points", "certified", "ambiguous", "back_walked"), (int(v) for v in out[:7])))

    def set_timing(self, enabled):
        capi.check(self._L.okenv_set_timing(self._h, 1 if enabled else 0), self._h)

    def get_timing(self):
        ms, n = C.c_double(), C.c_uint64()
        capi.check(self._L.okenv_get_timing(self._h, C.byref(ms), C.byref(n)), self._h)
        return ms.value, n.value

    def step_forms(self, clear=False):
        """Step-kernel launches since the handle was created (or last cleared), by form (capi.STEP_FORMS, enum okenv_step_form):
        {"forms": {form: launches}, "attrs": {form: {attribute: launches with it}}}, forms that never ran left out."""
        width = 1 + len(capi.STEP_FORM_ATTRS)
        out = np.zeros(len(capi.STEP_FORMS) * width, dtype=np.uint64)
        capi.check(self._L.okenv_debug_step_forms(self._h, capi.ptr(out), out.size, 1 if clear else 0), self._h)
        out = out.reshape(len(capi.STEP_FORMS), width)
        forms, attrs = {}, {}
        for name, row in zip(capi.STEP_FORMS, out):
            if row[0]:
                forms[name] = int(row[0])
                attrs[name] = {a: int(v) for a, v in zip(capi.STEP_FORM_ATTRS, row[1:])}
        return {"forms": forms, "attrs": attrs}

    def debug_cast_rays(self, ox, oy, angle_rad):
        ox, oy, ang = [np.ascontiguousarray(a, dtype=np.float32) for a in (ox, oy, angle_rad)]
        out = np.zeros(ox.size, dtype=np.float32)
        capi.check(self._L.okenv_debug_cast_rays(self._h, capi.ptr(ox), capi.ptr(oy), capi.ptr(ang), ox.size, capi.ptr(out)),
                   self._h)
        return out


def debug_sincos(x, device=0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    s, c = np.zeros_like(x), np.zeros_like(x)
    capi.check(capi.load().okenv_debug_sincos(int(device), capi.ptr(x), capi.ptr(s), capi.ptr(c), x.size))
    return s, c


def debug_math(fn, a, b=None, device=0):
    """One leaf function of include/okenv_math.h on a float32 array (okenv_debug_math), on GPU `device` or, with
    device=capi.DEBUG_ON_HOST, by the library's host compilation of the same header (no GPU needed).  fn: a name of capi.DEBUG_FNS or
    the integer.  b is the second argument of "atan2" (a = y, b = x) and of "sincos_pair".  Returns the result; (sine, cosine) for
    "sincos"; for "sincos_pair" two arrays of shape a.shape + (2,): (sine, cosine) of a and of b (ok_sincosf_pair)."""
    k = capi.DEBUG_FNS.index(fn) if isinstance(fn, str) else int(fn)
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
    if b is not None and b.shape != a.shape:
        raise ValueError("debug_math: a and b differ in shape")
    if k == capi.DEBUG_FNS.index("sincos_pair"):
        if b is None:
            raise ValueError("debug_math: sincos_pair takes two arrays")
        out0, out1 = np.zeros(a.shape + (2,), np.float32), np.zeros(a.shape + (2,), np.float32)
        capi.check(capi.load().okenv_debug_math(int(device), k, capi.ptr(a), capi.ptr(b), capi.ptr(out0), capi.ptr(out1), a.size))
        return out0, out1
    out0 = np.zeros_like(a)
    out1 = np.zeros_like(a) if k == capi.DEBUG_FNS.index("sincos") else None
    capi.check(capi.load().okenv_debug_math(int(device), k, capi.ptr(a), capi.ptr(b), capi.ptr(out0), capi.ptr(out1), a.size))
    return out0 if out1 is None else (out0, out1)


def debug_adam_device(params, t, p, m, v, g, device=0):
    """debug_adam with ok_learn_adam evaluated per element on GPU `device` (okenv_debug_adam_device), or on the host with
    device=capi.DEBUG_ON_HOST; params.eps may be 0 here.  Returns the new (p, m, v)."""
    p, m, v = (np.array(a, dtype=np.float32, copy=True).ravel() for a in (p, m, v))
    g = np.ascontiguousarray(g, dtype=np.float32).ravel()
    if not p.size == m.size == v.size == g.size:
        raise ValueError("debug_adam_device: p, m, v and g differ in size")
    capi.check(capi.load().okenv_debug_adam_device(int(device), C.byref(params), int(t), capi.ptr(p), capi.ptr(m), capi.ptr(v), capi.ptr(g), p.size))
    return p, m, v


def expert_act_host(params, ray_angles_deg, pos_x, pos_y, rot, dist, centerline=None, goals=None):
    """The experts' rule on host arrays, no GPU needed (okenv_expert_act_host): returns (throttle, steer) for n agents.  params:
    capi.expert_params(...); dist [n, R]; centerline = (x, y) of the track's centre line, or goals = (x, y) per agent."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    fan, pos_x, pos_y, rot, dist = f(ray_angles_deg), f(pos_x), f(pos_y), f(rot), f(dist)
    n = pos_x.size
    assert dist.size == n * fan.size and pos_y.size == n and rot.size == n
    cx = cy = gx = gy = None
    P = 0
    if goals is not None:
        gx, gy = f(goals[0]), f(goals[1])
        assert gx.size == n and gy.size == n
    if centerline is not None:
        cx, cy = f(centerline[0]), f(centerline[1])
        P = cx.size
    thr, steer = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    capi.check(capi.load().okenv_expert_act_host(C.byref(params) if params is not None else None, capi.ptr(fan), fan.size, capi.ptr(cx),
                                                 capi.ptr(cy), P, n, capi.ptr(pos_x), capi.ptr(pos_y), capi.ptr(rot), capi.ptr(dist), capi.ptr(gx),
                                                 capi.ptr(gy), capi.ptr(thr), capi.ptr(steer)))
    return thr, steer


def actor_act_host(params, policy, value, dist, crashed=None, draw_index=0):
    """The shared-network actors' rule on host arrays, no GPU needed (okenv_actor_act_host).  params: capi.actor_params(...);
    policy / value: flattened float32 parameter vectors (value None without a value network); dist [n, R].  Returns a dict:
    throttle, steer, prob [n] float32, action [n] int64, state [n, R] float32, alive [n] uint8 and, with a value network, value."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, R = dist.shape
    policy = None if policy is None else np.ascontiguousarray(policy, dtype=np.float32).ravel()
    value = None if value is None else np.ascontiguousarray(value, dtype=np.float32).ravel()
    if params is not None and policy is not None:
        assert policy.size == params.hidden * R + params.hidden + params.num_actions * params.hidden + params.num_actions
        assert value is None or value.size == params.value_hidden * R + 2 * params.value_hidden + 1
    crashed = None if crashed is None else np.ascontiguousarray(crashed, dtype=np.uint8)
    out = {"throttle": np.zeros(n, np.float32), "steer": np.zeros(n, np.float32), "action": np.zeros(n, np.int64),
           "prob": np.zeros(n, np.float32), "value": np.zeros(n, np.float32), "state": np.zeros((n, R), np.float32),
           "alive": np.zeros(n, np.uint8)}
    capi.check(capi.load().okenv_actor_act_host(C.byref(params) if params is not None else None, capi.ptr(policy), capi.ptr(value), R, n,
                                                capi.ptr(dist), capi.ptr(crashed), int(draw_index) & 0xFFFFFFFF, capi.ptr(out["throttle"]),
                                                capi.ptr(out["steer"]), capi.ptr(out["action"]), capi.ptr(out["prob"]), capi.ptr(out["value"]),
                                                capi.ptr(out["state"]), capi.ptr(out["alive"])))
    if params.value_hidden == 0:
        del out["value"]
    return out


def actor_act_dropout_host(params, p, dropout_seed, policy, value, dist, crashed=None, draw_index=0):
    """actor_act_host with REINFORCE's dropout (p, dropout_seed) on the policy network's hidden layer (okenv_actor_act_dropout_host);
    the same arguments and the same dict."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, R = dist.shape
    policy = None if policy is None else np.ascontiguousarray(policy, dtype=np.float32).ravel()
    value = None if value is None else np.ascontiguousarray(value, dtype=np.float32).ravel()
    if params is not None and policy is not None:
        assert policy.size == params.hidden * R + params.hidden + params.num_actions * params.hidden + params.num_actions
        assert value is None or value.size == params.value_hidden * R + 2 * params.value_hidden + 1
    crashed = None if crashed is None else np.ascontiguousarray(crashed, dtype=np.uint8)
    out = {"throttle": np.zeros(n, np.float32), "steer": np.zeros(n, np.float32), "action": np.zeros(n, np.int64),
           "prob": np.zeros(n, np.float32), "value": np.zeros(n, np.float32), "state": np.zeros((n, R), np.float32),
           "alive": np.zeros(n, np.uint8)}
    capi.check(capi.load().okenv_actor_act_dropout_host(C.byref(params) if params is not None else None, float(p), int(dropout_seed) & 0xFFFFFFFF,
                                                        capi.ptr(policy), capi.ptr(value), R, n, capi.ptr(dist), capi.ptr(crashed),
                                                        int(draw_index) & 0xFFFFFFFF, capi.ptr(out["throttle"]), capi.ptr(out["steer"]),
                                                        capi.ptr(out["action"]), capi.ptr(out["prob"]), capi.ptr(out["value"]),
                                                        capi.ptr(out["state"]), capi.ptr(out["alive"])))
    if params.value_hidden == 0:
        del out["value"]
    return out


def reinforce_update_host(params, shape, state, batch, B, accumulate=True, reduce="sum", p=0.0, dropout_seed=0, agent_base=0, num_agents=0,
                          draw_first=0, order=None, want=("loss", "grad_policy")):
    """REINFORCE's update on host arrays, no GPU needed (okenv_reinforce_update_host).  params: capi.learner_params(...); shape:
    (R, H, A); state: dict of float32 numpy arrays "policy", "policy_m", "policy_v" and the int "t" -- copied, the new state is
    returned; batch: dict of numpy arrays "state" [M,R], "action" [M] int64, "ret" [M] and, with p > 0, "index" [M] int32; order: None
    or int32 [M].  Returns (new state, outputs): outputs holds the arrays named in `want` ("loss": one value per optimiser step)."""
    R, H, A = (int(v) for v in shape)
    M = int(np.asarray(batch["ret"]).shape[0])
    b = {"state": np.ascontiguousarray(batch["state"], dtype=np.float32), "action": np.ascontiguousarray(batch["action"], dtype=np.int64),
         "ret": np.ascontiguousarray(batch["ret"], dtype=np.float32)}
    if batch.get("index") is not None:
        b["index"] = np.ascontiguousarray(batch["index"], dtype=np.int32)
    new = {k: np.array(v, dtype=np.float32, copy=True).ravel() for k, v in state.items() if k != "t" and v is not None}
    st = capi.fill_pointers(capi.OkenvLearnerState(), new, "learner state")
    st.t = int(state.get("t", 0))
    steps = (1 if accumulate else (M + int(B) - 1) // int(B)) if M > 0 and B > 0 else 0
    sizes = {"loss": steps, "grad_policy": H * R + H + A * H + A}
    outs = {k: np.zeros(sizes[k], dtype=np.float32) for k in want}
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
    cfg = capi.reinforce_config(accumulate, reduce, num_agents, draw_first) if reduce is not None else None
    capi.check(capi.load().okenv_reinforce_update_host(
        C.byref(params) if params is not None else None, C.byref(cfg) if cfg is not None else None, float(p), int(dropout_seed) & 0xFFFFFFFF,
        int(agent_base) & 0xFFFFFFFF, R, H, A, C.byref(st), C.byref(capi.fill_pointers(capi.OkenvReinforceBatch(), b, "reinforce batch")), M, int(B),
        capi.ptr(order), C.byref(capi.fill_pointers(capi.OkenvReinforceOutput(), {k: v for k, v in outs.items() if v.size}, "reinforce output"))))
    new["t"] = int(st.t)
    return new, outs


def batch_prepare_host(reward, alive, value=None, last_value=None, state=None, action=None, prob=None, num_agents=None, gamma=0.99, lam=1.0,
                       normalize=0, want=None, block_threads=0):
    """The episode-to-batch rule on host arrays, no GPU needed (okenv_batch_prepare_host).  reward / alive / value: [T, S] with
    S >= num_agents (default S) agent slots per row, the rest padding; state [T, S', R], action [T, S'] int64, prob [T, S'] share
    their own S'.  want: the outputs to ask for (default: every one the inputs allow) out of "state", "action", "prob", "ret", "adv",
    "index", "ret_plane", "adv_plane", "stats", "count"; the others are passed as NULL.  Returns a dict: the dense outputs cut to M
    rows, the planes [T, N], "stats" as a dict, "count" (the word) and "M" (the out-parameter)."""
    reward = np.ascontiguousarray(reward, dtype=np.float32)
    alive = np.ascontiguousarray(alive).view(np.uint8) if np.asarray(alive).dtype == np.bool_ else np.ascontiguousarray(alive, dtype=np.uint8)
    T, S = reward.shape
    N = S if num_agents is None else int(num_agents)
    assert alive.shape == (T, S)
    value = None if value is None else np.ascontiguousarray(value, dtype=np.float32)
    last_value = None if last_value is None else np.ascontiguousarray(last_value, dtype=np.float32)
    state = None if state is None else np.ascontiguousarray(state, dtype=np.float32)
    action = None if action is None else np.ascontiguousarray(action, dtype=np.int64)
    prob = None if prob is None else np.ascontiguousarray(prob, dtype=np.float32)
    fields = [a for a in (state, action, prob) if a is not None]
    Sf = fields[0].shape[1] if fields else S
    assert all(a.shape[:2] == (T, Sf) for a in fields) and (value is None or value.shape == (T, S))
    R = state.shape[2] if state is not None else 0
    cap = max(T * N, 1)
    possible = {"ret": np.zeros(cap, np.float32), "index": np.zeros(cap, np.int32), "ret_plane": np.zeros((max(T, 1), max(N, 1)), np.float32),
                "stats": np.zeros(capi.BATCH_STATS_BYTES, np.uint8), "count": np.zeros(1, np.int32)}
    if value is not None:
        possible.update(adv=np.zeros(cap, np.float32), adv_plane=np.zeros((max(T, 1), max(N, 1)), np.float32))
    if state is not None:
        possible["state"] = np.zeros((cap, R), np.float32)
    if action is not None:
        possible["action"] = np.zeros(cap, np.int64)
    if prob is not None:
        possible["prob"] = np.zeros(cap, np.float32)
    out = possible if want is None else {k: (possible[k] if k in possible else np.zeros(cap, np.float32)) for k in want}
    bp = capi.OkenvBatchParams(T, N, R, S if S != N else 0, Sf if Sf != N else 0, float(gamma), float(lam), int(normalize), int(block_threads))
    bi, bo = capi.OkenvBatchInput(), capi.OkenvBatchOutput()
    for k, v in (("reward", reward), ("alive", alive), ("value", value), ("last_value", last_value), ("state", state), ("action", action),
                 ("prob", prob)):
        if v is not None:
            setattr(bi, k, v.ctypes.data)
    for k, v in out.items():
        setattr(bo, k, v.ctypes.data)
    m = C.c_int32(-1)
    capi.check(capi.load().okenv_batch_prepare_host(C.byref(bp), C.byref(bi), C.byref(bo), C.byref(m)))
    res = {"M": m.value}
    for k, v in out.items():
        if k == "stats":
            res[k] = capi.batch_stats_dict(v)
        elif k in ("ret_plane", "adv_plane", "count"):
            res[k] = v
        else:
            res[k] = v[:m.value]
    return res


def ppo_update_host(params, shape, state, batch, B, epochs=1, order=None, want=("actor_loss", "critic_loss", "clipped", "grad_policy", "grad_value")):
    """PPO's update on host arrays, no GPU needed (okenv_ppo_update_host).  params: capi.learner_params(...); shape: (R, H, A, Hv);
    state: dict of float32 numpy arrays "policy", "policy_m", "policy_v" (and "value", "value_m", "value_v" with a critic) and the int
    "t" -- copied, the new state is returned; batch: dict of numpy arrays "state" [M,R], "action" [M] int64, "prob", "ret" and
    optionally "adv"; order: None or int32 [epochs, M].  Returns (new state, outputs): outputs holds the arrays named in `want`."""
    R, H, A, Hv = (int(v) for v in shape)
    M = int(np.asarray(batch["ret"]).shape[0])
    b = {"state": np.ascontiguousarray(batch["state"], dtype=np.float32), "action": np.ascontiguousarray(batch["action"], dtype=np.int64),
         "prob": np.ascontiguousarray(batch["prob"], dtype=np.float32), "ret": np.ascontiguousarray(batch["ret"], dtype=np.float32)}
    if batch.get("adv") is not None:
        b["adv"] = np.ascontiguousarray(batch["adv"], dtype=np.float32)
    new = {k: np.array(v, dtype=np.float32, copy=True).ravel() for k, v in state.items() if k != "t" and v is not None}
    st = capi.fill_pointers(capi.OkenvLearnerState(), new, "learner state")
    st.t = int(state.get("t", 0))
    nmb = int(epochs) * ((M + int(B) - 1) // int(B)) if M > 0 and B > 0 and epochs > 0 else 0
    n_policy = H * R + H + A * H + A
    n_value = Hv * R + Hv + Hv + 1 if Hv > 0 else 0
    sizes = {"actor_loss": (nmb, np.float32), "critic_loss": (nmb, np.float32), "clipped": (nmb, np.int32), "grad_policy": (n_policy, np.float32),
             "grad_value": (n_value, np.float32)}
    outs = {k: np.zeros(sizes[k][0], dtype=sizes[k][1]) for k in want}
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
    capi.check(capi.load().okenv_ppo_update_host(C.byref(params) if params is not None else None, R, H, A, Hv, C.byref(st),
                                                 C.byref(capi.fill_pointers(capi.OkenvPpoBatch(), b, "ppo batch")), M, int(B), int(epochs),
                                                 capi.ptr(order), C.byref(capi.fill_pointers(capi.OkenvPpoOutput(), {k: v for k, v in outs.items() if v.size}, "ppo output"))))
    new["t"] = int(st.t)
    return new, outs


def _host_ring(kind, capacity, num_rays, new=np.zeros):
    return {"state": new((capacity, num_rays), np.float32), "next_state": new((capacity, num_rays), np.float32),
            "action": new((capacity,) + kind.action_shape, kind.action_dtype), "reward": new(capacity, np.float32),
            "done": new(capacity, np.float32), "pushed": 0}


def _ring_struct(kind, ring):
    return capi.fill_pointers(kind.ring_struct(), {k: v for k, v in ring.items() if k != "pushed"}, "replay ring")


def _push_host(kind, ring, state, action, alive, dist, crashed, reward, push_all):
    Cn, R = ring["state"].shape
    state = np.ascontiguousarray(state, dtype=np.float32)
    action = np.ascontiguousarray(action, dtype=kind.action_dtype)
    alive = None if alive is None else np.ascontiguousarray(alive).astype(np.uint8)
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    crashed = np.ascontiguousarray(crashed).astype(np.uint8)
    reward = None if reward is None else np.ascontiguousarray(reward, dtype=np.float32)
    n = action.shape[0]
    assert state.shape == (n, R) and dist.shape == (n, R) and crashed.shape == (n,)
    assert not kind.action_shape or action.shape == (n,) + kind.action_shape  # (Deep-Q's one index per agent was never checked)
    pushed = C.c_uint64(int(ring["pushed"]))
    entry = getattr(capi.load(), kind.prefix + "_push_host")
    capi.check(entry(C.byref(_ring_struct(kind, ring)), Cn, R, C.byref(pushed), capi.REPLAY_PUSH_ALL if push_all else 0, n, capi.ptr(state),
                     capi.ptr(action), capi.ptr(alive), capi.ptr(dist), capi.ptr(crashed), capi.ptr(reward)))
    ring["pushed"] = int(pushed.value)
    return ring


def replay_ring(capacity, num_rays):
    """An empty replay ring on the host: dict of zeroed numpy arrays and "pushed" = 0."""
    return _host_ring(_DQN_RING, capacity, num_rays)


def replay_push_host(ring, state, action, alive, dist, crashed, reward=None, push_all=False):
    """One push on host arrays, no GPU needed (okenv_replay_push_host): `ring` (replay_ring(...)) is updated in place, "pushed"
    included.  state [n,R], action [n] int64 and alive [n] are the actor record, dist [n,R] and crashed [n] the fields after the step."""
    return _push_host(_DQN_RING, ring, state, action, alive, dist, crashed, reward, push_all)


def dqn_update_host(params, config, shape, state, ring, B, iterations=1, resample=False, draw_base=0, target=None, size=None,
                    want=("loss", "grad_policy", "index")):
    """Deep-Q's update on host arrays, no GPU needed (okenv_dqn_update_host).  params: capi.learner_params(...); config:
    capi.dqn_config(...); shape: (R, H, A); state: dict of float32 arrays "policy", "policy_m", "policy_v" and the int "t" -- copied, the
    new state is returned; ring: replay_ring(...) as the pushes left it; target: the target network's parameters when config turns it
    on.  Returns (new state, outputs): outputs holds the arrays named in `want`."""
    R, H, A = (int(v) for v in shape)
    new = {k: np.array(state[k], dtype=np.float32, copy=True).ravel() for k in ("policy", "policy_m", "policy_v")}
    st = capi.fill_pointers(capi.OkenvLearnerState(), new, "learner state")
    st.t = int(state.get("t", 0))
    size = min(int(ring["pushed"]), ring["state"].shape[0]) if size is None else int(size)
    sizes = {"loss": (max(int(iterations), 0), np.float32), "grad_policy": (H * R + H + A * H + A, np.float32), "index": (max(int(B), 0), np.int32)}
    outs = {k: np.zeros(sizes[k][0], dtype=sizes[k][1]) for k in want}
    target = None if target is None else np.ascontiguousarray(target, dtype=np.float32).ravel()
    capi.check(capi.load().okenv_dqn_update_host(C.byref(params) if params is not None else None, C.byref(config) if config is not None else None,
                                                 R, H, A, C.byref(st), capi.ptr(target), C.byref(_ring_struct(_DQN_RING, ring)), size, int(B), int(iterations),
                                                 1 if resample else 0, int(draw_base) & 0xFFFFFFFF,
                                                 C.byref(capi.fill_pointers(capi.OkenvDqnOutput(), {k: v for k, v in outs.items() if v.size}, "dqn output"))))
    new["t"] = int(st.t)
    return new, outs


def ddpg_act_host(config, actor, dist, crashed=None, draw_index=0):
    """DDPG's action on host arrays, no GPU needed (okenv_ddpg_act_host).  config: capi.ddpg_config(...); actor: the flattened float32
    parameters; dist [n, R].  Returns a dict: throttle, steer [n], action [n, 2], state [n, R] float32 and alive [n] uint8."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, R = dist.shape
    actor = None if actor is None else np.ascontiguousarray(actor, dtype=np.float32).ravel()
    if config is not None and actor is not None:
        assert actor.size == config.hidden * R + config.hidden + 2 * config.hidden + 2
    crashed = None if crashed is None else np.ascontiguousarray(crashed, dtype=np.uint8)
    out = {"throttle": np.zeros(n, np.float32), "steer": np.zeros(n, np.float32), "action": np.zeros((n, 2), np.float32),
           "state": np.zeros((n, R), np.float32), "alive": np.zeros(n, np.uint8)}
    capi.check(capi.load().okenv_ddpg_act_host(C.byref(config) if config is not None else None, capi.ptr(actor), R, n, capi.ptr(dist), capi.ptr(crashed),
                                               int(draw_index) & 0xFFFFFFFF, capi.ptr(out["throttle"]), capi.ptr(out["steer"]), capi.ptr(out["action"]),
                                               capi.ptr(out["state"]), capi.ptr(out["alive"])))
    return out


def ddpg_ring(capacity, num_rays):
    """An empty DDPG replay ring on the host: dict of zeroed numpy arrays (action [C, 2] float32) and "pushed" = 0."""
    return _host_ring(_DDPG_RING, capacity, num_rays)


def ddpg_replay_push_host(ring, state, action, alive, dist, crashed, reward=None, push_all=False):
    """One push on host arrays, no GPU needed (okenv_ddpg_replay_push_host): `ring` (ddpg_ring(...)) is updated in place, "pushed"
    included.  state [n,R], action [n,2] and alive [n] are the record, dist [n,R] and crashed [n] the fields after the step."""
    return _push_host(_DDPG_RING, ring, state, action, alive, dist, crashed, reward, push_all)


def ddpg_update_host(config, num_rays, state, ring, B, iterations=1, resample=False, draw_base=0, size=None,
                     want=("critic_loss", "actor_loss", "grad_critic", "grad_actor", "index")):
    """DDPG's update on host arrays, no GPU needed (okenv_ddpg_update_host).  config: capi.ddpg_config(...); state: dict of the float32
    arrays capi.DDPG_STATE_VECTORS and the int "t" -- copied, the new state is returned; ring: ddpg_ring(...) as the pushes left it.
    Returns (new state, outputs): outputs holds the arrays named in `want`."""
    R = int(num_rays)
    new = {k: np.array(state[k], dtype=np.float32, copy=True).ravel() for k in capi.DDPG_STATE_VECTORS if state.get(k) is not None}
    st = capi.fill_pointers(capi.OkenvDdpgState(), new, "ddpg state")
    st.t = int(state.get("t", 0))
    size = min(int(ring["pushed"]), ring["state"].shape[0]) if size is None else int(size)
    H, Hc = (config.hidden, config.critic_hidden) if config is not None else (0, 0)
    sizes = {"critic_loss": (max(int(iterations), 0), np.float32), "actor_loss": (max(int(iterations), 0), np.float32),
             "grad_critic": (max(Hc * (R + 2) + 2 * Hc + 1, 0), np.float32), "grad_actor": (max(H * R + 3 * H + 2, 0), np.float32),
             "index": (max(int(B), 0), np.int32)}
    outs = {k: np.zeros(sizes[k][0], dtype=sizes[k][1]) for k in want}
    capi.check(capi.load().okenv_ddpg_update_host(C.byref(config) if config is not None else None, R, C.byref(st), C.byref(_ring_struct(_DDPG_RING, ring)), size,
                                                  int(B), int(iterations), 1 if resample else 0, int(draw_base) & 0xFFFFFFFF,
                                                  C.byref(capi.fill_pointers(capi.OkenvDdpgOutput(), {k: v for k, v in outs.items() if v.size}, "ddpg output"))))
    new["t"] = int(st.t)
    return new, outs


def debug_adam(params, t, p, m, v, g):
    """ok_learn_adam on host arrays (no GPU): step number t of float32 arrays p, m, v with gradients g; returns the new (p, m, v)."""
    p, m, v = (np.array(a, dtype=np.float32, copy=True).ravel() for a in (p, m, v))
    g = np.ascontiguousarray(g, dtype=np.float32).ravel()
    capi.check(capi.load().okenv_debug_adam(C.byref(params), int(t), capi.ptr(p), capi.ptr(m), capi.ptr(v), capi.ptr(g), p.size))
    return p, m, v


def debug_expf(x):
    """ok_expf (the actors' softmax) on a host array (no GPU)."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(a)
    capi.check(capi.load().okenv_debug_expf(capi.ptr(a), capi.ptr(out), a.size))
    return out


def debug_logf(x):
    """ok_logf of include/okenv_math.h (the logarithm of REINFORCE's loss column) for an array of positive float32 arguments."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    capi.check(capi.load().okenv_debug_logf(capi.ptr(x), capi.ptr(out), x.size))
    return out


def debug_reinforce_mask(p, seed, agent, draw, hidden):
    """REINFORCE's dropout mask of hidden units 0 .. hidden-1 for one (global agent id, draw index): uint8, 1 kept."""
    out = np.zeros(int(hidden), dtype=np.uint8)
    capi.check(capi.load().okenv_debug_reinforce_mask(float(p), int(seed) & 0xFFFFFFFF, int(agent) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFF, int(hidden),
                                                      capi.ptr(out)))
    return out


def debug_atan2f(y, x):
    """ok_atan2f of include/okenv_math.h on host arrays (no GPU)."""
    y, x = np.ascontiguousarray(y, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros_like(y)
    capi.check(capi.load().okenv_debug_atan2f(capi.ptr(y), capi.ptr(x), capi.ptr(out), y.size))
    return out


def debug_expert_normalize_angle(angle_deg):
    """The experts' bounded normalizeAngleDeg on a host array (no GPU)."""
    a = np.ascontiguousarray(angle_deg, dtype=np.float32)
    out = np.zeros_like(a)
    capi.check(capi.load().okenv_debug_expert_normalize_angle(capi.ptr(a), capi.ptr(out), a.size))
    return out


def debug_normal(w0, w1, device=0):
    """ok_gauss_normal_pair of include/okenv_gauss.h on uint32 word pairs (okenv_debug_normal), on GPU `device` or, with
    device=capi.DEBUG_ON_HOST, on the host (no GPU needed).  Returns (r cos, r sin): the even and the odd component of a block."""
    w0, w1 = np.ascontiguousarray(w0, dtype=np.uint32), np.ascontiguousarray(w1, dtype=np.uint32)
    if w0.shape != w1.shape:
        raise ValueError("debug_normal: w0 and w1 differ in shape")
    out0, out1 = np.zeros(w0.shape, np.float32), np.zeros(w0.shape, np.float32)
    capi.check(capi.load().okenv_debug_normal(int(device), capi.ptr(w0), capi.ptr(w1), capi.ptr(out0), capi.ptr(out1), w0.size))
    return out0, out1


def gauss_act_host(config, params, dist, crashed=None, draw_index=0):
    """The Gaussian actor's action on host arrays, no GPU needed (okenv_gauss_act_host).  config: capi.gauss_config(...); params: the
    flattened float32 parameter vector; dist [n, R].  Returns a dict: throttle, steer [n], eps, pre, action [n, 2], logp [n], state
    [n, R] float32 and alive [n] uint8 (eps stays NaN when acting greedily: nothing is drawn)."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, R = dist.shape
    params = None if params is None else np.ascontiguousarray(params, dtype=np.float32).ravel()
    if config is not None and params is not None:
        assert params.size == capi.gauss_num_params(R, config.hidden1, config.hidden2)
    crashed = None if crashed is None else np.ascontiguousarray(crashed, dtype=np.uint8)
    out = {"throttle": np.zeros(n, np.float32), "steer": np.zeros(n, np.float32), "eps": np.full((n, 2), np.nan, np.float32),
           "pre": np.zeros((n, 2), np.float32), "action": np.zeros((n, 2), np.float32), "logp": np.zeros(n, np.float32),
           "state": np.zeros((n, R), np.float32), "alive": np.zeros(n, np.uint8)}
    capi.check(capi.load().okenv_gauss_act_host(C.byref(config) if config is not None else None, capi.ptr(params), R, n, capi.ptr(dist),
                                                capi.ptr(crashed), int(draw_index) & 0xFFFFFFFF, capi.ptr(out["throttle"]), capi.ptr(out["steer"]),
                                                capi.ptr(out["eps"]), capi.ptr(out["pre"]), capi.ptr(out["action"]), capi.ptr(out["logp"]),
                                                capi.ptr(out["state"]), capi.ptr(out["alive"])))
    return out


def gauss_update_host(params, shape, state, batch, B, accumulate=True, reduce="sum", grad="reference", order=None, want=("loss", "grad")):
    """The continuous REINFORCE update on host arrays, no GPU needed (okenv_gauss_update_host).  params: capi.learner_params(...); shape:
    (R, H1, H2) or (R, H1, H2, A); state: dict of float32 numpy arrays "params", "m", "v" and the int "t" -- copied, the new state is
    returned; batch: dict of numpy arrays "state" [M,R], "ret" [M] and "eps" / "pre" [M,A]; order: None or int32 [M].  Returns
    (new state, outputs): outputs holds the arrays named in `want` ("loss": one value per optimiser step)."""
    R, H1, H2, A = (tuple(int(v) for v in shape) + (2,))[:4]
    M = int(np.asarray(batch["ret"]).shape[0])
    b = {k: np.ascontiguousarray(batch[k], dtype=np.float32) for k in ("state", "eps", "pre", "ret") if batch.get(k) is not None}
    new = {k: np.array(v, dtype=np.float32, copy=True).ravel() for k, v in state.items() if k != "t" and v is not None}
    st = capi.fill_pointers(capi.OkenvGaussState(), new, "gauss state")
    st.t = int(state.get("t", 0))
    steps = (1 if accumulate else (M + int(B) - 1) // int(B)) if M > 0 and B > 0 else 0
    sizes = {"loss": steps, "grad": capi.gauss_num_params(R, H1, H2, A)}
    outs = {k: np.zeros(sizes[k], dtype=np.float32) for k in want}
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
    cfg = capi.gauss_update_config(accumulate, reduce, grad) if reduce is not None else None
    capi.check(capi.load().okenv_gauss_update_host(
        C.byref(params) if params is not None else None, C.byref(cfg) if cfg is not None else None, R, H1, H2, A, C.byref(st),
        C.byref(capi.fill_pointers(capi.OkenvGaussBatch(), b, "gauss batch")), M, int(B), capi.ptr(order),
        C.byref(capi.fill_pointers(capi.OkenvGaussOutput(), {k: v for k, v in outs.items() if v.size}, "gauss output"))))
    new["t"] = int(st.t)
    return new, outs


def _gcl_which(which):
    return capi.GCL_NETWORKS[which] if isinstance(which, str) else int(which)


def gcl_act_host(config, policy, rel_xy, crashed=None, draw_index=0):
    """Guided cost learning's action on host arrays, no GPU needed (okenv_gcl_act_host).  config: capi.gcl_config(...); policy: the
    flattened float32 parameter vector; rel_xy [n, R, 2]: the hits relative to the agent.  Returns a dict: throttle, steer [n], eps, pre,
    squashed, action [n, 2], logp [n], state [n, R] float32 and alive [n] uint8 (eps stays NaN when acting greedily)."""
    rel_xy = np.asarray(rel_xy, dtype=np.float32)
    n, R = rel_xy.shape[:2]
    rel_x, rel_y = np.ascontiguousarray(rel_xy[..., 0]), np.ascontiguousarray(rel_xy[..., 1])
    policy = None if policy is None else np.ascontiguousarray(policy, dtype=np.float32).ravel()
    if config is not None and policy is not None:
        assert policy.size == capi.gcl_num_params("policy", R, config.hidden1, config.hidden2)
    crashed = None if crashed is None else np.ascontiguousarray(crashed, dtype=np.uint8)
    out = {"throttle": np.zeros(n, np.float32), "steer": np.zeros(n, np.float32), "eps": np.full((n, 2), np.nan, np.float32),
           "pre": np.zeros((n, 2), np.float32), "squashed": np.zeros((n, 2), np.float32), "action": np.zeros((n, 2), np.float32),
           "logp": np.zeros(n, np.float32), "state": np.zeros((n, R), np.float32), "alive": np.zeros(n, np.uint8)}
    capi.check(capi.load().okenv_gcl_act_host(C.byref(config) if config is not None else None, capi.ptr(policy), R, n, capi.ptr(rel_x), capi.ptr(rel_y),
                                              capi.ptr(crashed), int(draw_index) & 0xFFFFFFFF, capi.ptr(out["throttle"]), capi.ptr(out["steer"]),
                                              capi.ptr(out["eps"]), capi.ptr(out["pre"]), capi.ptr(out["squashed"]), capi.ptr(out["action"]),
                                              capi.ptr(out["logp"]), capi.ptr(out["state"]), capi.ptr(out["alive"])))
    return out


def gcl_cost_host(cost, shape, state, squashed):
    """The cost of M rows on host arrays (okenv_gcl_cost_host).  shape: (R, C1, C2); state [M, R], squashed [M, 2].  Returns [M]."""
    R, C1, C2 = (int(v) for v in shape)
    state, squashed = np.ascontiguousarray(state, dtype=np.float32), np.ascontiguousarray(squashed, dtype=np.float32)
    out = np.zeros(state.shape[0], np.float32)
    cost = None if cost is None else np.ascontiguousarray(cost, dtype=np.float32).ravel()
    capi.check(capi.load().okenv_gcl_cost_host(capi.ptr(cost), R, C1, C2, capi.ptr(state), capi.ptr(squashed), out.size, capi.ptr(out)))
    return out


def _gcl_host_state(state):
    new = {k: np.array(v, dtype=np.float32, copy=True).ravel() for k, v in state.items() if k != "t" and v is not None}
    st = capi.fill_pointers(capi.OkenvGclState(), new, "gcl state")
    st.t = int(state.get("t", 0))
    return new, st


def gcl_cost_update_host(params, seed, shape, state, bank, batch, Me, want=("loss", "grad")):
    """One step of the cost network on host arrays (okenv_gcl_cost_update_host).  params: capi.learner_params(...); shape: (R, C1, C2);
    state: dict "params", "m", "v", "t" (copied; the new state is returned); bank: dict "state" [E, R], "action" [E, 2]; batch: dict
    "state" [Mp, R], "squashed" [Mp, 2].  Returns (new state, outputs)."""
    R, C1, C2 = (int(v) for v in shape)
    new, st = _gcl_host_state(state)
    bs = None if bank.get("state") is None else np.ascontiguousarray(bank["state"], dtype=np.float32)
    ba = None if bank.get("action") is None else np.ascontiguousarray(bank["action"], dtype=np.float32)
    E = 0 if bs is None else bs.shape[0]
    b = {k: np.ascontiguousarray(batch[k], dtype=np.float32) for k in ("state", "squashed") if batch.get(k) is not None}
    Mp = int(np.asarray(batch["squashed"]).shape[0]) if batch.get("squashed") is not None else int(np.asarray(batch["state"]).shape[0])
    sizes = {"loss": 1, "grad": capi.gcl_num_params("cost", R, C1, C2)}
    outs = {k: np.zeros(sizes[k], dtype=np.float32) for k in want}
    capi.check(capi.load().okenv_gcl_cost_update_host(
        C.byref(params) if params is not None else None, int(seed) & 0xFFFFFFFF, R, C1, C2, C.byref(st), capi.ptr(bs), capi.ptr(ba), E,
        C.byref(capi.fill_pointers(capi.OkenvGclCostBatch(), b, "gcl cost batch")), Mp, int(Me),
        C.byref(capi.fill_pointers(capi.OkenvGclCostOutput(), outs, "gcl cost output"))))
    new["t"] = int(st.t)
    return new, outs


def gcl_policy_update_host(params, shape, policy, value, batch, B, accumulate=True, reduce="mean", order=None,
                           want=("policy_loss", "value_loss", "clipped", "grad_policy", "grad_value", "adv")):
    """The policy / value update on host arrays (okenv_gcl_policy_update_host).  params: capi.learner_params(...); shape: (R, H1, H2);
    policy, value: dicts "params", "m", "v" (and "t" in policy), copied; batch: dict "state" [M, R], "pre" [M, 2], "logp" [M], "ret" [M];
    order: None or int32 [M].  Returns (new policy state, new value state, outputs)."""
    R, H1, H2 = (int(v) for v in shape)
    M = int(np.asarray(batch["ret"]).shape[0])
    b = {k: np.ascontiguousarray(batch[k], dtype=np.float32) for k in ("state", "pre", "logp", "ret") if batch.get(k) is not None}
    newp, sp = _gcl_host_state(policy)
    newv, sv = _gcl_host_state(dict(value, t=policy.get("t", 0)))
    steps = (1 if accumulate else (M + int(B) - 1) // int(B)) if M > 0 and B > 0 else 0
    sizes = {"policy_loss": steps, "value_loss": steps, "clipped": steps, "grad_policy": capi.gcl_num_params("policy", R, H1, H2),
             "grad_value": capi.gcl_num_params("value", R, H1, H2), "adv": M}
    outs = {k: np.zeros(sizes[k], dtype=np.int32 if k == "clipped" else np.float32) for k in want}
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
    cfg = capi.gcl_update_config(accumulate, reduce) if reduce is not None else None
    capi.check(capi.load().okenv_gcl_policy_update_host(
        C.byref(params) if params is not None else None, C.byref(cfg) if cfg is not None else None, R, H1, H2, C.byref(sp), C.byref(sv),
        C.byref(capi.fill_pointers(capi.OkenvGclBatch(), b, "gcl batch")), M, int(B), capi.ptr(order),
        C.byref(capi.fill_pointers(capi.OkenvGclOutput(), {k: v for k, v in outs.items() if v.size}, "gcl output"))))
    newp["t"] = newv["t"] = int(sp.t)
    return newp, newv, outs
