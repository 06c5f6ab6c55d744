"""ctypes binding of the C ABI in include/okenv.h (libokenv.so, built by openkitchen_amd/buildlib.py).

Fails loudly if the shared object is missing or cannot be loaded: there is no Python or CPU fallback for
the hot path.
"""
import ctypes as C
import functools
import os

import numpy as np

from . import buildlib as _build

OKENV_OK = 0
ERR_NAMES = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE", -4: "IO", -5: "STATE"}

MODE_VELOCITY, MODE_ACCELERATION, MODE_MANUAL = 0, 1, 2
RESET_RANDOM_POINT, RESET_RANDOM_LANE, RESET_RANDOM_HEADING, RESET_ONLY_DONE = 1, 2, 4, 8
FLAG_NONE, FLAG_FORCE_GLOBAL_GRID, FLAG_BRUTE_FORCE = 0, 1, 2

(F_POS_X, F_POS_Y, F_ROT, F_SPEED, F_ACC, F_THROTTLE, F_STEER, F_MODE, F_CRASHED, F_TIMED_OUT, F_DISP_CTR, F_DISP_X,
 F_DISP_Y, F_DISP_TO, F_HIT_X, F_HIT_Y, F_REL_X, F_REL_Y, F_DIST) = range(19)
FIELD_NAMES = ["pos_x", "pos_y", "rot", "speed", "acc", "thr", "steer", "mode", "crashed", "timed_out", "disp_ctr",
               "disp_x", "disp_y", "disp_to", "hit_x", "hit_y", "rel_x", "rel_y", "dist"]
FIELD_DTYPE = [np.float32] * 7 + [np.uint8] * 3 + [np.uint32, np.float32, np.float32, np.uint8] + [np.float32] * 5
PER_RAY = {F_HIT_X, F_HIT_Y, F_REL_X, F_REL_Y, F_DIST}
# rollout bookkeeping fields (exist after okenv_tracker_create)
F_REWARD, F_FITNESS, F_TRACK_IDX, F_EPISODE_STEPS, F_EPISODE_RETURN, F_PREV_CRASHED = range(19, 25)
FIELD_NAMES += ["reward", "fitness", "track_idx", "episode_steps", "episode_return", "prev_crashed"]
FIELD_DTYPE += [np.float32, np.float32, np.int32, np.uint32, np.float32, np.uint8]
REWARD_STEP, REWARD_PROGRESS = 0, 1
# bird's-eye camera views (include/okenv.h)
VIEW_RGBA8, VIEW_CLASS8 = 0, 1
VIEW_DRAW_AGENT, VIEW_DRAW_HEADING, VIEW_HEADING_UP = 1, 2, 4
VIEW_FOLLOW_W, VIEW_FOLLOW_H = 1600.0 / 15.0, 1400.0 / 15.0  # as fp32 these equal OKENV_VIEW_FOLLOW_W / _H
# expert drivers (include/okenv.h)
EXPERT_POTFIELD, EXPERT_VFH = 0, 1
EXPERT_KINDS = {"potfield": EXPERT_POTFIELD, "vfh": EXPERT_VFH}
# shared-network actors (include/okenv.h)
ACTOR_SAMPLE, ACTOR_GREEDY, ACTOR_EPS_GREEDY = 0, 1, 2
ACTOR_MODES = {"sample": ACTOR_SAMPLE, "greedy": ACTOR_GREEDY, "eps_greedy": ACTOR_EPS_GREEDY}
ACTOR_MAX_RAYS, ACTOR_MAX_HIDDEN, ACTOR_MAX_ACTIONS = 64, 256, 8
# episode -> batch (include/okenv.h)
BATCH_NORMALIZE_RETURN, BATCH_NORMALIZE_ADVANTAGE = 1, 2
BATCH_KERNELS = ("walk", "tree", "count", "scan", "gather")
# PPO's update (include/okenv.h)
UPDATE_KERNELS = ("grad", "step")
LEARN_CHUNK = 32
# REINFORCE (include/okenv.h)
REINFORCE_SUM, REINFORCE_MEAN = 0, 1
REINFORCE_REDUCE = {"sum": REINFORCE_SUM, "mean": REINFORCE_MEAN}
REINFORCE_KERNELS = ("grad", "step")
# okenv_debug_math (include/okenv.h): enum okenv_debug_fn in order, and the device number that means "evaluate on the host"
DEBUG_FNS = ("sincos", "tanh", "exp", "log", "atan2", "normalize_angle", "expert_normalize_angle", "sincos_pair", "erf")
DEBUG_ON_HOST = -1

# every symbol include/okenv.h declares (tests/test_capi_symbols.py checks the library exports them all)
SYMBOLS = [
    "okenv_create", "okenv_destroy", "okenv_get_info", "okenv_last_error", "okenv_set_sensor_offset",
    "okenv_set_centerline", "okenv_set_stream", "okenv_sync", "okenv_set_field", "okenv_get_field",
    "okenv_upload_state", "okenv_download_state", "okenv_set_actions", "okenv_reset_agents", "okenv_get_hits",
    "okenv_get_distances", "okenv_get_flags", "okenv_step", "okenv_collide", "okenv_rollout_random",
    "okenv_init_bench_state", "okenv_nearest_track_idx", "okenv_set_timing", "okenv_get_timing", "okenv_track_load",
    "okenv_track_free", "okenv_track_num_points", "okenv_track_num_segments", "okenv_track_get",
    "okenv_track_segments", "okenv_track_queries", "okenv_debug_sincos", "okenv_debug_cast_rays", "okenv_policy_mlp_create",
    "okenv_policy_mlp_weights_per_agent", "okenv_policy_mlp_get_weights", "okenv_policy_mlp_set_weights",
    "okenv_rollout_policy", "okenv_alive_count", "okenv_reset_all", "okenv_ga_scores", "okenv_ga_select_mate",
    "okenv_q_create", "okenv_q_begin_episode", "okenv_rollout_q", "okenv_q_get_table", "okenv_q_set_table", "okenv_q_get_state",
    "okenv_q_table_sums", "okenv_q_assign_mean", "okenv_q_share_knowledge",
    "okenv_set_lane_bounds", "okenv_reset_random", "okenv_set_auto_reset", "okenv_get_step_count",
    "okenv_set_step_count", "okenv_field_device_ptr", "okenv_tracker_create", "okenv_tracker_begin",
    "okenv_tracker_update", "okenv_step_packed",
    "okenv_controller_create", "okenv_controller_num_params", "okenv_controller_set_params", "okenv_controller_act", "okenv_rollout_controller",
    "okenv_episode_begin", "okenv_episode_compact", "okenv_episode_end", "okenv_episode_tail_limit", "okenv_work_stats",
    "okenv_ga_scores_device", "okenv_get_stream", "okenv_off_grid_count", "okenv_work_stats_split", "okenv_debug_step_forms",
    "okenv_render_create", "okenv_render_views", "okenv_render_get_info", "okenv_track_band_triangles",
    "okenv_expert_create", "okenv_expert_act", "okenv_expert_act_host", "okenv_debug_atan2f", "okenv_debug_expert_normalize_angle",
    "okenv_debug_plan_step",
    "okenv_actor_create", "okenv_actor_num_params", "okenv_actor_set_params", "okenv_actor_set_epsilon", "okenv_actor_set_draw_offset",
    "okenv_actor_act", "okenv_actor_act_host", "okenv_debug_expf",
    "okenv_batch_prepare", "okenv_batch_count", "okenv_batch_prepare_host", "okenv_debug_batch_timing",
    "okenv_learner_create", "okenv_learner_reset", "okenv_ppo_update", "okenv_ppo_update_host", "okenv_actor_get_params",
    "okenv_learner_get_state", "okenv_debug_update_timing", "okenv_debug_adam",
    "okenv_replay_create", "okenv_replay_reset", "okenv_replay_push", "okenv_replay_size", "okenv_replay_get", "okenv_dqn_params",
    "okenv_dqn_update", "okenv_dqn_sync_target", "okenv_replay_push_host", "okenv_dqn_update_host",
    "okenv_debug_dqn_timing",
    "okenv_ddpg_create", "okenv_ddpg_num_params", "okenv_ddpg_set_params", "okenv_ddpg_get_state", "okenv_ddpg_set_draw_offset",
    "okenv_ddpg_act", "okenv_ddpg_replay_create", "okenv_ddpg_replay_reset", "okenv_ddpg_replay_push", "okenv_ddpg_replay_size",
    "okenv_ddpg_replay_get", "okenv_ddpg_update", "okenv_debug_ddpg_timing", "okenv_ddpg_act_host", "okenv_ddpg_replay_push_host",
    "okenv_ddpg_update_host",
    "okenv_actor_set_dropout", "okenv_actor_act_dropout_host", "okenv_reinforce_update", "okenv_reinforce_update_host",
    "okenv_debug_reinforce_timing", "okenv_debug_logf", "okenv_debug_reinforce_mask",
    "okenv_debug_math", "okenv_debug_adam_device",
    "okenv_gauss_lds_bytes", "okenv_gauss_create", "okenv_gauss_num_params", "okenv_gauss_set_params", "okenv_gauss_get_params",
    "okenv_gauss_get_state", "okenv_gauss_set_draw_offset", "okenv_gauss_set_greedy", "okenv_gauss_act", "okenv_gauss_learner_create",
    "okenv_gauss_update", "okenv_gauss_act_host", "okenv_gauss_update_host", "okenv_debug_gauss_timing", "okenv_debug_normal",
    "okenv_gcl_lds_bytes", "okenv_gcl_create", "okenv_gcl_num_params", "okenv_gcl_set_params", "okenv_gcl_get_params", "okenv_gcl_get_state",
    "okenv_gcl_set_draw_offset", "okenv_gcl_set_greedy", "okenv_gcl_act", "okenv_gcl_set_expert", "okenv_gcl_cost", "okenv_gcl_learner_create",
    "okenv_gcl_cost_update", "okenv_gcl_policy_update", "okenv_debug_gcl_timing", "okenv_gcl_act_host", "okenv_gcl_cost_host",
    "okenv_gcl_cost_update_host", "okenv_gcl_policy_update_host",
    "okenv_lidar_lds_bytes", "okenv_lidar_create", "okenv_lidar_num_params", "okenv_lidar_set_params", "okenv_lidar_get_params", "okenv_lidar_act",
    "okenv_lidar_act_host", "okenv_debug_lidar_linear",
    "okenv_flow_lds_bytes", "okenv_flow_create", "okenv_flow_num_params", "okenv_flow_set_params", "okenv_flow_get_params",
    "okenv_flow_set_draw_offset", "okenv_flow_act", "okenv_flow_act_host",
    "okenv_bev_lds_bytes", "okenv_bev_tiles", "okenv_bev_create", "okenv_bev_num_params", "okenv_bev_set_params", "okenv_bev_get_params",
    "okenv_bev_encode", "okenv_debug_bev_stages", "okenv_bev_encode_host",
    "okenv_cnn_lds_bytes", "okenv_cnn_plan", "okenv_cnn_create", "okenv_cnn_num_params", "okenv_cnn_set_params", "okenv_cnn_get_params",
    "okenv_cnn_act", "okenv_debug_cnn_stages", "okenv_cnn_act_host",
    "okenv_world_lds_bytes", "okenv_world_plan", "okenv_world_workspace_bytes", "okenv_world_create", "okenv_world_num_params",
    "okenv_world_set_params", "okenv_world_get_params", "okenv_world_act", "okenv_world_set_lane_widths", "okenv_world_score_begin",
    "okenv_world_score", "okenv_world_fitness", "okenv_world_fitness_device", "okenv_debug_world_stages", "okenv_world_act_host",
    "okenv_world_score_host",
    "okenv_memory_lds_bytes", "okenv_memory_plan", "okenv_memory_workspace_bytes", "okenv_memory_create", "okenv_memory_num_params",
    "okenv_memory_set_params", "okenv_memory_get_params", "okenv_memory_reset", "okenv_memory_set_hidden", "okenv_memory_get_hidden",
    "okenv_memory_act", "okenv_debug_memory_stages", "okenv_memory_act_host",
    "okenv_memory_learner_workspace_bytes", "okenv_memory_learner_lds_bytes", "okenv_memory_learner_create", "okenv_memory_learner_reset",
    "okenv_memory_learner_get_state", "okenv_memory_update", "okenv_memory_eval", "okenv_memory_update_host", "okenv_memory_eval_host",
    "okenv_memory_window_host",
    "okenv_qcnn_lds_bytes", "okenv_qcnn_plan", "okenv_qcnn_create", "okenv_qcnn_num_params", "okenv_qcnn_set_params", "okenv_qcnn_get_params",
    "okenv_qcnn_set_epsilon", "okenv_qcnn_set_draw_offset", "okenv_qcnn_act", "okenv_debug_qcnn_stages", "okenv_qcnn_ring_create",
    "okenv_qcnn_ring_reset", "okenv_qcnn_ring_size", "okenv_qcnn_ring_get", "okenv_qcnn_push", "okenv_qcnn_batch", "okenv_qcnn_act_host",
    "okenv_qcnn_push_host", "okenv_qcnn_batch_host", "okenv_debug_qcnn_grey_host", "okenv_debug_qcnn_forward_planes_host",
    "okenv_vit_lds_bytes", "okenv_vit_create", "okenv_vit_num_params", "okenv_vit_set_params", "okenv_vit_get_params", "okenv_vit_act",
    "okenv_vit_act_host", "okenv_debug_vit_attend",
    "okenv_vit_embed", "okenv_vit_head_lds_bytes", "okenv_vit_head_learner_create", "okenv_vit_head_learner_reset",
    "okenv_vit_head_learner_get_state", "okenv_vit_head_update", "okenv_vit_head_eval", "okenv_vit_head_update_host", "okenv_vit_head_eval_host",
]

# enum okenv_step_form / okenv_step_form_attr of include/okenv.h, in order (tests/test_step_form_table.py keeps them in step)
STEP_FORMS = ["tail_q", "tail_mlp32", "tail_mlp15", "tail_mlp", "coop_q", "coop_ctrl", "coop_mlp32", "coop_mlp",
              "coop_packed_direct", "coop_packed", "coop_direct", "coop_g64_random", "coop_g64", "coop", "resident_direct", "resident",
              "lds", "lds_mlp", "global", "global_mlp", "brute", "brute_mlp"]
STEP_FORM_ATTRS = ["front_back", "list", "widened", "ctrl_lds", "agents_per_block"]


class OkenvInfo(C.Structure):
    _fields_ = [("num_agents", C.c_int32), ("num_rays", C.c_int32), ("num_segments", C.c_int32),
                ("grid_nx", C.c_int32), ("grid_ny", C.c_int32), ("grid_cell", C.c_float), ("grid_refs", C.c_int32),
                ("grid_in_lds", C.c_int32), ("lds_bytes", C.c_int32), ("block_threads", C.c_int32),
                ("grid_blocks", C.c_int32), ("lanes_per_agent", C.c_int32), ("device", C.c_int32),
                ("agents_per_block", C.c_int32), ("packed_resident", C.c_int32), ("packed_resident_steps", C.c_int32),
                ("packed_fallbacks", C.c_int32), ("compute_units", C.c_int32), ("front_back_bytes", C.c_int32),
                ("back_segments", C.c_int32)]


class OkenvViewDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("format", C.c_int32),
                ("view_w", C.c_float), ("view_h", C.c_float), ("flags", C.c_uint32), ("radius", C.c_float),
                ("agent_rgb", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class OkenvRenderInfo(C.Structure):
    _fields_ = [("triangles", C.c_int32), ("grid_nx", C.c_int32), ("grid_ny", C.c_int32), ("grid_cell", C.c_float),
                ("registrations", C.c_int32), ("solid_cells", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("samples", C.c_int32), ("channels", C.c_int32), ("bytes_per_call", C.c_uint64)]


class OkenvExpertParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lookahead", C.c_int32), ("goal_wrap", C.c_int32), ("k_att", C.c_float), ("k_rep", C.c_float),
                ("effect_range", C.c_float), ("clamp_deg", C.c_float), ("vfh_throttle", C.c_float), ("vfh_threshold", C.c_int32)]


class OkenvExpertRecord(C.Structure):
    _fields_ = [("action", C.c_void_p), ("dist", C.c_void_p), ("rel_xy", C.c_void_p), ("alive", C.c_void_p)]


def expert_params(kind, lookahead=2, goal_wrap=False, k_att=100.0, k_rep=10.0, effect_range=5.0, clamp_deg=0.0, vfh_throttle=100.0,
                  vfh_threshold=1):
    """okenv_expert_params with the reference's constants as defaults (PotentialFieldAgent.hpp:22-25, VFHAgent.hpp:20-21);
    kind: "potfield" / "vfh" or the integer."""
    k = EXPERT_KINDS[kind] if isinstance(kind, str) else int(kind)
    return OkenvExpertParams(k, int(lookahead), 1 if goal_wrap else 0, k_att, k_rep, effect_range, clamp_deg, vfh_throttle, int(vfh_threshold))


class OkenvActorParams(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("num_actions", C.c_int32), ("value_hidden", C.c_int32), ("mode", C.c_int32), ("epsilon", C.c_float),
                ("seed", C.c_uint32), ("agent_base", C.c_uint32), ("action_table", (C.c_float * 2) * 8)]


class OkenvActorRecord(C.Structure):
    _fields_ = [("state", C.c_void_p), ("action", C.c_void_p), ("prob", C.c_void_p), ("value", C.c_void_p), ("alive", C.c_void_p)]


def actor_params(hidden, actions, value_hidden=0, mode="sample", epsilon=0.0, seed=0, agent_base=0):
    """okenv_actor_params; actions: the table [(throttle_delta, steering_delta), ...] (2 .. 8 rows), mode: "sample" / "greedy" /
    "eps_greedy" or the integer."""
    ap = OkenvActorParams(int(hidden), len(actions), int(value_hidden), ACTOR_MODES[mode] if isinstance(mode, str) else int(mode),
                          float(epsilon), int(seed) & 0xFFFFFFFF, int(agent_base) & 0xFFFFFFFF)
    for k, (thr, steer) in enumerate(list(actions)[:ACTOR_MAX_ACTIONS]):
        ap.action_table[k][0], ap.action_table[k][1] = float(thr), float(steer)
    return ap


class OkenvBatchParams(C.Structure):
    _fields_ = [("num_steps", C.c_int32), ("num_agents", C.c_int32), ("state_width", C.c_int32), ("record_stride", C.c_int32),
                ("field_stride", C.c_int32), ("gamma", C.c_float), ("lam", C.c_float), ("normalize", C.c_uint32), ("block_threads", C.c_int32)]


class OkenvBatchInput(C.Structure):
    _fields_ = [("reward", C.c_void_p), ("alive", C.c_void_p), ("value", C.c_void_p), ("last_value", C.c_void_p), ("state", C.c_void_p),
                ("action", C.c_void_p), ("prob", C.c_void_p)]


class OkenvBatchStats(C.Structure):
    _fields_ = [("sum_ret", C.c_double), ("sumsq_ret", C.c_double), ("sum_adv", C.c_double), ("sumsq_adv", C.c_double),
                ("mean_ret", C.c_float), ("std_ret", C.c_float), ("mean_adv", C.c_float), ("std_adv", C.c_float),
                ("count", C.c_int32), ("reserved", C.c_int32)]


class OkenvBatchOutput(C.Structure):
    _fields_ = [("state", C.c_void_p), ("action", C.c_void_p), ("prob", C.c_void_p), ("ret", C.c_void_p), ("adv", C.c_void_p),
                ("index", C.c_void_p), ("ret_plane", C.c_void_p), ("adv_plane", C.c_void_p), ("stats", C.c_void_p), ("count", C.c_void_p)]


BATCH_STATS_BYTES = C.sizeof(OkenvBatchStats)  # 56


class OkenvLearnerParams(C.Structure):
    _fields_ = [("lr", C.c_float), ("clip", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class OkenvPpoBatch(C.Structure):
    _fields_ = [("state", C.c_void_p), ("action", C.c_void_p), ("prob", C.c_void_p), ("ret", C.c_void_p), ("adv", C.c_void_p)]


class OkenvPpoOutput(C.Structure):
    _fields_ = [("actor_loss", C.c_void_p), ("critic_loss", C.c_void_p), ("clipped", C.c_void_p), ("grad_policy", C.c_void_p),
                ("grad_value", C.c_void_p)]


class OkenvLearnerState(C.Structure):
    _fields_ = [("policy", C.c_void_p), ("policy_m", C.c_void_p), ("policy_v", C.c_void_p), ("value", C.c_void_p), ("value_m", C.c_void_p),
                ("value_v", C.c_void_p), ("t", C.c_int64)]


def learner_params(lr=3e-4, clip=0.2, beta1=0.9, beta2=0.999, eps=1e-8):
    """okenv_learner_params with the reference's learning rate and clip (PPOAgent.hpp:24-26) and torch.optim.Adam's defaults."""
    return OkenvLearnerParams(float(lr), float(clip), float(beta1), float(beta2), float(eps))


class OkenvReinforceConfig(C.Structure):
    _fields_ = [("accumulate", C.c_int32), ("reduce", C.c_int32), ("num_agents", C.c_int32), ("draw_first", C.c_uint32)]


class OkenvReinforceBatch(C.Structure):
    _fields_ = [("state", C.c_void_p), ("action", C.c_void_p), ("ret", C.c_void_p), ("index", C.c_void_p)]


class OkenvReinforceOutput(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("grad_policy", C.c_void_p)]


def reinforce_config(accumulate=True, reduce="sum", num_agents=0, draw_first=0):
    """okenv_reinforce_config with the reference's choices as defaults (ReinforceAgent.hpp:109-118: one step on the summed loss);
    reduce: "sum" / "mean" or the integer."""
    return OkenvReinforceConfig(1 if accumulate else 0, REINFORCE_REDUCE[reduce] if isinstance(reduce, str) else int(reduce), int(num_agents),
                                int(draw_first) & 0xFFFFFFFF)


REPLAY_PUSH_ALL = 1  # OKENV_REPLAY_PUSH_ALL
DQN_MASK_DONE = 1    # OKENV_DQN_MASK_DONE


class OkenvReplayRing(C.Structure):
    _fields_ = [("state", C.c_void_p), ("next_state", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p)]


class OkenvDqnConfig(C.Structure):
    _fields_ = [("gamma", C.c_float), ("flags", C.c_uint32), ("target_network", C.c_int32), ("seed", C.c_uint32)]


class OkenvDqnOutput(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("grad_policy", C.c_void_p), ("index", C.c_void_p)]


def dqn_config(gamma=0.99, mask_done=False, target_network=False, seed=0):
    """okenv_dqn_config with the reference's discount (DQAgent.hpp:33) and target (:133: no mask, no target network)."""
    return OkenvDqnConfig(float(gamma), DQN_MASK_DONE if mask_done else 0, 1 if target_network else 0, int(seed) & 0xFFFFFFFF)


# DDPG (include/okenv.h)
DDPG_MAX_RAYS = 62
DDPG_KERNELS = ("critic_grad", "critic_step", "actor_grad", "actor_step")


class OkenvDdpgConfig(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("critic_hidden", C.c_int32), ("scale", C.c_float * 2), ("bias", C.c_float * 2), ("noise", C.c_float * 2),
                ("seed", C.c_uint32), ("agent_base", C.c_uint32), ("gamma", C.c_float), ("tau", C.c_float), ("lr_actor", C.c_float),
                ("lr_critic", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("sample_seed", C.c_uint32)]


class OkenvDdpgRecord(C.Structure):
    _fields_ = [("state", C.c_void_p), ("action", C.c_void_p), ("alive", C.c_void_p)]


class OkenvDdpgRing(C.Structure):
    _fields_ = [("state", C.c_void_p), ("next_state", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p)]


class OkenvDdpgState(C.Structure):
    _fields_ = [("actor", C.c_void_p), ("critic", C.c_void_p), ("actor_target", C.c_void_p), ("critic_target", C.c_void_p),
                ("actor_m", C.c_void_p), ("actor_v", C.c_void_p), ("critic_m", C.c_void_p), ("critic_v", C.c_void_p), ("t", C.c_int64)]


DDPG_STATE_VECTORS = [name for name, _ in OkenvDdpgState._fields_ if name != "t"]


class OkenvDdpgOutput(C.Structure):
    _fields_ = [("critic_loss", C.c_void_p), ("actor_loss", C.c_void_p), ("grad_critic", C.c_void_p), ("grad_actor", C.c_void_p),
                ("index", C.c_void_p)]


def ddpg_config(hidden, critic_hidden, scale=(50.0, 5.0), bias=(50.0, 0.0), noise=(0.0, 0.0), seed=0, agent_base=0, gamma=0.99, tau=0.005,
                lr_actor=1e-4, lr_critic=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, sample_seed=0):
    """okenv_ddpg_config with the reference's constants as defaults (Actor.hpp:14-17, DDPGAgent.hpp:27-33: no exploration noise) and
    torch.optim.Adam's."""
    return OkenvDdpgConfig(int(hidden), int(critic_hidden), (C.c_float * 2)(*map(float, scale)), (C.c_float * 2)(*map(float, bias)),
                           (C.c_float * 2)(*map(float, noise)), int(seed) & 0xFFFFFFFF, int(agent_base) & 0xFFFFFFFF, float(gamma), float(tau),
                           float(lr_actor), float(lr_critic), float(beta1), float(beta2), float(eps), int(sample_seed) & 0xFFFFFFFF)


# continuous REINFORCE (include/okenv.h)
GAUSS_GRAD_REFERENCE, GAUSS_GRAD_SCORE = 0, 1
GAUSS_GRAD = {"reference": GAUSS_GRAD_REFERENCE, "score": GAUSS_GRAD_SCORE}
GAUSS_KERNELS = ("grad", "step")
GAUSS_MAX_HIDDEN = 128
GAUSS_LDS_BUDGET = 160 * 1024


class OkenvGaussConfig(C.Structure):
    _fields_ = [("hidden1", C.c_int32), ("hidden2", C.c_int32), ("scale", C.c_float * 2), ("bias", C.c_float * 2), ("greedy", C.c_int32),
                ("seed", C.c_uint32), ("agent_base", C.c_uint32)]


class OkenvGaussRecord(C.Structure):
    _fields_ = [("state", C.c_void_p), ("eps", C.c_void_p), ("pre", C.c_void_p), ("action", C.c_void_p), ("logp", C.c_void_p),
                ("alive", C.c_void_p)]


class OkenvGaussState(C.Structure):
    _fields_ = [("params", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("t", C.c_int64)]


class OkenvGaussUpdateConfig(C.Structure):
    _fields_ = [("accumulate", C.c_int32), ("reduce", C.c_int32), ("grad_mode", C.c_int32)]


class OkenvGaussBatch(C.Structure):
    _fields_ = [("state", C.c_void_p), ("eps", C.c_void_p), ("pre", C.c_void_p), ("ret", C.c_void_p)]


class OkenvGaussOutput(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("grad", C.c_void_p)]


def gauss_config(hidden1=128, hidden2=128, scale=(50.0, 10.0), bias=(50.0, 0.0), greedy=False, seed=0, agent_base=0):
    """okenv_gauss_config with the reference's widths and action ranges as defaults (Policy.hpp:17-24, ReinforceAgent.hpp:85-88)."""
    return OkenvGaussConfig(int(hidden1), int(hidden2), (C.c_float * 2)(*map(float, scale)), (C.c_float * 2)(*map(float, bias)),
                            int(greedy), int(seed) & 0xFFFFFFFF, int(agent_base) & 0xFFFFFFFF)


def gauss_update_config(accumulate=True, reduce="sum", grad="reference"):
    """okenv_gauss_update_config with the reference's choices as defaults; reduce: "sum" / "mean", grad: "reference" / "score", or
    the integers."""
    return OkenvGaussUpdateConfig(1 if accumulate else 0, REINFORCE_REDUCE[reduce] if isinstance(reduce, str) else int(reduce),
                                  GAUSS_GRAD[grad] if isinstance(grad, str) else int(grad))


def gauss_num_params(R, H1, H2, A=2):
    """Floats of the parameter vector [log_std | fc1.weight | fc1.bias | fc2.weight | fc2.bias | mean.weight | mean.bias]."""
    return A + H1 * R + H1 + H2 * H1 + H2 + A * H2 + A


def gauss_lds_bytes(R, H1, H2, A=2):
    """okenv_gauss_lds_bytes: the gradient kernel's LDS for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_gauss_lds_bytes(int(R), int(H1), int(H2), int(A)))


# lidar transformer driver (include/okenv.h)
LIDAR_LDS_BUDGET = 160 * 1024


class OkenvLidarConfig(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("d_model", C.c_int32), ("nhead", C.c_int32), ("num_layers", C.c_int32),
                ("dim_feedforward", C.c_int32), ("head_hidden1", C.c_int32), ("head_hidden2", C.c_int32), ("action_lo", C.c_float * 2),
                ("action_hi", C.c_float * 2), ("sensor_range", C.c_float)]


class OkenvLidarRecord(C.Structure):
    _fields_ = [("action", C.c_void_p), ("input", C.c_void_p), ("alive", C.c_void_p)]


def lidar_config(num_points=7, d_model=128, nhead=8, num_layers=3, dim_feedforward=512, head_hidden1=256, head_hidden2=64,
                 action_lo=(0.0, -2.0), action_hi=(100.0, 2.0), sensor_range=200.0):
    """okenv_lidar_config with the reference's shape and ranges as defaults (laser_transformer.py, infer_torch_traced_main.cpp:19-43)."""
    return OkenvLidarConfig(int(num_points), int(d_model), int(nhead), int(num_layers), int(dim_feedforward), int(head_hidden1),
                            int(head_hidden2), (C.c_float * 2)(*map(float, action_lo)), (C.c_float * 2)(*map(float, action_hi)),
                            float(sensor_range))


def lidar_layout(cfg):
    """ok_lidar_offsets: where every piece of the parameter vector begins, as (name, offset, shape) in order; the names are the
    reference module's state-dict keys, the last piece is the positional table "pos".  The last entry's end is the vector's length."""
    R, d, F, H1, H2 = cfg.num_points, cfg.d_model, cfg.dim_feedforward, cfg.head_hidden1, cfg.head_hidden2
    pieces = [("point_embedding.weight", (d, 2)), ("point_embedding.bias", (d,))]
    for i in range(cfg.num_layers):
        pre = "transformer_encoder.layers.%d." % i
        pieces += [(pre + "self_attn.in_proj_weight", (3 * d, d)), (pre + "self_attn.in_proj_bias", (3 * d,)),
                   (pre + "self_attn.out_proj.weight", (d, d)), (pre + "self_attn.out_proj.bias", (d,)),
                   (pre + "linear1.weight", (F, d)), (pre + "linear1.bias", (F,)), (pre + "linear2.weight", (d, F)), (pre + "linear2.bias", (d,)),
                   (pre + "norm1.weight", (d,)), (pre + "norm1.bias", (d,)), (pre + "norm2.weight", (d,)), (pre + "norm2.bias", (d,))]
    pieces += [("control_head.0.weight", (H1, R * d)), ("control_head.0.bias", (H1,)), ("control_head.2.weight", (H2, H1)),
               ("control_head.2.bias", (H2,)), ("control_head.4.weight", (2, H2)), ("control_head.4.bias", (2,)), ("pos", (R, d))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def lidar_num_params(cfg):
    """Floats of the parameter vector, the positional table included."""
    name, at, shape = lidar_layout(cfg)[-1]
    return at + int(np.prod(shape))


def lidar_lds_bytes(cfg):
    """okenv_lidar_lds_bytes: the act kernel's LDS for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_lidar_lds_bytes(C.byref(cfg)))


def lidar_act_host(cfg, params, rel_xy, crashed=None):
    """okenv_lidar_act_host on numpy arrays: rel_xy [n][R][2] -> dict(throttle, steer [n], input [n][R][2], alive [n]).  No GPU needed."""
    rel_xy = np.ascontiguousarray(rel_xy, np.float32)
    params = np.ascontiguousarray(params, np.float32)
    n = rel_xy.shape[0]
    assert rel_xy.shape == (n, cfg.num_points, 2) and params.size == lidar_num_params(cfg)
    crashed = None if crashed is None else np.ascontiguousarray(crashed, np.uint8)
    out = dict(throttle=np.empty(n, np.float32), steer=np.empty(n, np.float32), input=np.empty((n, cfg.num_points, 2), np.float32),
               alive=np.empty(n, np.uint8))
    check(load().okenv_lidar_act_host(C.byref(cfg), ptr(params), n, ptr(rel_xy), ptr(crashed), ptr(out["throttle"]), ptr(out["steer"]),
                                      ptr(out["input"]), ptr(out["alive"])))
    return out


def debug_lidar_linear(x, w, bias, relu=False, device=DEBUG_ON_HOST):
    """okenv_debug_lidar_linear: x [M][K], w [N][K], bias [N] -> [M][N]; device < 0 evaluates the rule on the host."""
    x, w, bias = (np.ascontiguousarray(a, np.float32) for a in (x, w, bias))
    (M, K), N = x.shape, w.shape[0]
    assert w.shape == (N, K) and bias.shape == (N,)
    out = np.empty((M, N), np.float32)
    check(load().okenv_debug_lidar_linear(int(device), M, K, N, ptr(x), ptr(w), ptr(bias), 1 if relu else 0, ptr(out)))
    return out


# flow-matching driver (include/okenv.h)
FLOW_LDS_BUDGET = 160 * 1024
FLOW_AGENTS = 16  # agents per workgroup of the act kernel (ok_flow.h: kFlowAgents); tests/test_flow_rule.py keeps the two in step


class OkenvFlowConfig(C.Structure):
    _fields_ = [("cond_dim", C.c_int32), ("hidden", C.c_int32), ("steps", C.c_int32), ("noise", C.c_int32), ("action_lo", C.c_float * 2),
                ("action_hi", C.c_float * 2), ("seed", C.c_uint32), ("agent_base", C.c_uint32)]


class OkenvFlowRecord(C.Structure):
    _fields_ = [("x0", C.c_void_p), ("x", C.c_void_p), ("action", C.c_void_p), ("alive", C.c_void_p)]


def flow_config(cond_dim=128, hidden=256, steps=32, noise=True, action_lo=(0.0, -10.0), action_hi=(100.0, 10.0), seed=0, agent_base=0):
    """okenv_flow_config with the reference's shape and ranges as defaults (flow_matching_model.py, main_flow_control.cpp:19, 97-101)."""
    return OkenvFlowConfig(int(cond_dim), int(hidden), int(steps), int(noise), (C.c_float * 2)(*map(float, action_lo)),
                           (C.c_float * 2)(*map(float, action_hi)), int(seed) & 0xFFFFFFFF, int(agent_base) & 0xFFFFFFFF)


def flow_layout(cfg):
    """ok_flow_offsets: where every piece of the parameter vector begins, as (name, offset, shape) in order; the names are the
    state-dict keys of the reference's ActionFlowTrunk.  The last entry's end is the vector's length."""
    Cd, H = cfg.cond_dim, cfg.hidden
    pieces = [("net.0.weight", (H, 3 + Cd)), ("net.0.bias", (H,)), ("net.2.weight", (H, H)), ("net.2.bias", (H,)), ("net.4.weight", (2, H)),
              ("net.4.bias", (2,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def flow_num_params(cfg):
    """Floats of the trunk's parameter vector."""
    name, at, shape = flow_layout(cfg)[-1]
    return at + int(np.prod(shape))


def flow_lds_bytes(cfg):
    """okenv_flow_lds_bytes: the act kernel's LDS for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_flow_lds_bytes(C.byref(cfg)))


def flow_act_host(cfg, params, cond, crashed=None, draw_index=0):
    """okenv_flow_act_host on numpy arrays: cond [n][cond_dim] -> dict(throttle, steer [n], x0, x [n][2], alive [n]).  No GPU needed."""
    cond = np.ascontiguousarray(cond, np.float32)
    params = np.ascontiguousarray(params, np.float32)
    n = cond.shape[0]
    assert cond.shape == (n, cfg.cond_dim) and params.size == flow_num_params(cfg)
    crashed = None if crashed is None else np.ascontiguousarray(crashed, np.uint8)
    out = dict(throttle=np.empty(n, np.float32), steer=np.empty(n, np.float32), x0=np.empty((n, 2), np.float32), x=np.empty((n, 2), np.float32),
               alive=np.empty(n, np.uint8))
    check(load().okenv_flow_act_host(C.byref(cfg), ptr(params), n, ptr(cond), ptr(crashed), int(draw_index) & 0xFFFFFFFF, ptr(out["throttle"]),
                                     ptr(out["steer"]), ptr(out["x0"]), ptr(out["x"]), ptr(out["alive"])))
    return out


# the flow driver's image encoder (include/okenv.h)
BEV_LDS_BUDGET = 160 * 1024
BEV_STAGE_FRONT, BEV_STAGE_BACK, BEV_STAGE_HEAD = 1, 2, 4


class OkenvBevConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("kernel", C.c_int32 * 3), ("channels", C.c_int32 * 3), ("embed_dim", C.c_int32)]


def bev_config(image_size=128, kernel=(5, 3, 3), channels=(32, 64, 128), embed_dim=128):
    """okenv_bev_config with the reference's shape as defaults (flow_matching_model.py: BEVEncoder)."""
    return OkenvBevConfig(int(image_size), (C.c_int32 * 3)(*map(int, kernel)), (C.c_int32 * 3)(*map(int, channels)), int(embed_dim))


def bev_layout(cfg):
    """ok_bev_offsets: where every piece of the parameter vector begins, as (name, offset, shape) in order; the names are the
    state-dict keys of the reference's BEVEncoder.  The last entry's end is the vector's length."""
    k, c = list(cfg.kernel), list(cfg.channels)
    pieces = []
    for l, cin in enumerate([3] + c[:2]):
        pieces += [("conv.%d.weight" % (2 * l), (c[l], cin, k[l], k[l])), ("conv.%d.bias" % (2 * l), (c[l],))]
    pieces += [("proj.weight", (cfg.embed_dim, c[2])), ("proj.bias", (cfg.embed_dim,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def bev_num_params(cfg):
    """Floats of the encoder's parameter vector."""
    name, at, shape = bev_layout(cfg)[-1]
    return at + int(np.prod(shape))


def bev_lds_bytes(cfg):
    """okenv_bev_lds_bytes: the larger conv kernel's LDS for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_bev_lds_bytes(C.byref(cfg)))


def bev_tiles(cfg):
    """okenv_bev_tiles: the sides of the output tiles of the two conv kernels, the kernels' paths.  No GPU needed."""
    out = (C.c_int32 * 2)()
    check(load().okenv_bev_tiles(C.byref(cfg), out))
    return int(out[0]), int(out[1])


def bev_encode_host(cfg, params, frames):
    """okenv_bev_encode_host on numpy arrays: frames [n][S][S][4] uint8 -> [n][embed_dim] float32.  No GPU needed."""
    frames = np.ascontiguousarray(frames, np.uint8)
    params = np.ascontiguousarray(params, np.float32)
    n = frames.shape[0]
    assert frames.shape == (n, cfg.image_size, cfg.image_size, 4) and params.size == bev_num_params(cfg)
    out = np.empty((n, cfg.embed_dim), np.float32)
    check(load().okenv_bev_encode_host(C.byref(cfg), ptr(params), n, ptr(frames), ptr(out)))
    return out


# behavioural-cloning image policy (include/okenv.h)
CNN_LDS_BUDGET = 160 * 1024
CNN_STAGE_CONV, CNN_STAGE_HEAD = 1, 2
CNN_AGENTS = 16  # agents per workgroup of the head kernel (ok_conv.h: kConvAgents)


class OkenvCnnConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("kernel", C.c_int32 * 3), ("stride", C.c_int32 * 3), ("channels", C.c_int32 * 3),
                ("hidden", C.c_int32), ("throttle", C.c_float), ("steer_scale", C.c_float)]


class OkenvCnnRecord(C.Structure):
    _fields_ = [("out", C.c_void_p), ("action", C.c_void_p), ("alive", C.c_void_p)]


def cnn_config(image_size=96, kernel=(8, 4, 3), stride=(4, 2, 1), channels=(32, 64, 64), hidden=256, throttle=100.0, steer_scale=10.0):
    """okenv_cnn_config with the reference's shape and controls as defaults (BehavioralCloning: env_train_bc.py PolicyCNN, main.cpp)."""
    return OkenvCnnConfig(int(image_size), (C.c_int32 * 3)(*map(int, kernel)), (C.c_int32 * 3)(*map(int, stride)),
                          (C.c_int32 * 3)(*map(int, channels)), int(hidden), float(throttle), float(steer_scale))


def cnn_sides(cfg):
    """ok_cnn_side: the sides of the three convolutions' outputs (a valid convolution floors; 0 where the kernel does not fit)."""
    side, out = cfg.image_size, []
    for k, s in zip(cfg.kernel, cfg.stride):
        side = 0 if side < k or s < 1 else (side - k) // s + 1
        out.append(side)
    return tuple(out)


def cnn_layout(cfg):
    """ok_cnn_offsets: where every piece of the parameter vector begins, as (name, offset, shape) in order; the names are the
    state-dict keys of the reference's PolicyCNN.  The last entry's end is the vector's length."""
    k, c, H = list(cfg.kernel), list(cfg.channels), cfg.hidden
    F = c[2] * cnn_sides(cfg)[2] ** 2
    pieces = []
    for l, cin in enumerate([3] + c[:2]):
        pieces += [("encoder.%d.weight" % (2 * l), (c[l], cin, k[l], k[l])), ("encoder.%d.bias" % (2 * l), (c[l],))]
    pieces += [("steering_head.0.weight", (H, F)), ("steering_head.0.bias", (H,)), ("steering_head.2.weight", (1, H)),
               ("steering_head.2.bias", (1,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def cnn_num_params(cfg):
    """Floats of the policy's parameter vector."""
    name, at, shape = cnn_layout(cfg)[-1]
    return at + int(np.prod(shape))


def cnn_lds_bytes(cfg):
    """okenv_cnn_lds_bytes: the larger act kernel's LDS for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_cnn_lds_bytes(C.byref(cfg)))


def cnn_plan(cfg):
    """okenv_cnn_plan: (tiles of 16 hidden units per wave of the head kernel, what sizes the conv kernel's first LDS region), the
    kernels' paths.  No GPU needed."""
    out = (C.c_int32 * 2)()
    check(load().okenv_cnn_plan(C.byref(cfg), out))
    return int(out[0]), int(out[1])


def cnn_act_host(cfg, params, frames, crashed=None):
    """okenv_cnn_act_host on numpy arrays: frames [n][S][S][4] uint8 -> dict(throttle, steer, out [n] float32, alive [n]).  No GPU
    needed."""
    frames = np.ascontiguousarray(frames, np.uint8)
    params = np.ascontiguousarray(params, np.float32)
    n = frames.shape[0]
    assert frames.shape == (n, cfg.image_size, cfg.image_size, 4) and params.size == cnn_num_params(cfg)
    crashed = None if crashed is None else np.ascontiguousarray(crashed, np.uint8)
    out = dict(throttle=np.empty(n, np.float32), steer=np.empty(n, np.float32), out=np.empty(n, np.float32), alive=np.empty(n, np.uint8))
    check(load().okenv_cnn_act_host(C.byref(cfg), ptr(params), n, ptr(frames), ptr(crashed), ptr(out["throttle"]), ptr(out["steer"]),
                                    ptr(out["out"]), ptr(out["alive"])))
    return out


# Deep-Q image racers (include/okenv.h)
QCNN_LDS_BUDGET = 160 * 1024
QCNN_STAGE_CONV, QCNN_STAGE_HEAD, QCNN_STAGE_HEAD_32 = 1, 2, 4
QCNN_AGENTS = 16  # agents per workgroup of the head kernel (ok_conv.h: kConvAgents)
QCNN_BATCH_UNIFORM, QCNN_BATCH_SEQUENTIAL = 0, 1
QCNN_BATCH_MODES = {"uniform": QCNN_BATCH_UNIFORM, "sequential": QCNN_BATCH_SEQUENTIAL}
# DQCNNAgent::kActionMap: (throttle_delta, steering_delta) per action index (kVelocity 60, kSteeringDelta 5 degrees)
QCNN_ACTION_MAP = ((60.0, 0.0), (30.0, 5.0), (30.0, -5.0), (30.0, 2.5), (30.0, -2.5))


class OkenvQcnnConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("kernel", C.c_int32 * 3), ("stride", C.c_int32 * 3), ("padding", C.c_int32 * 3),
                ("channels", C.c_int32 * 3), ("hidden", C.c_int32), ("num_actions", C.c_int32), ("mode", C.c_int32), ("epsilon", C.c_float),
                ("seed", C.c_uint32), ("agent_base", C.c_uint32), ("action_table", (C.c_float * 2) * 8)]


class OkenvQcnnRecord(C.Structure):
    _fields_ = [("q", C.c_void_p), ("action", C.c_void_p), ("value", C.c_void_p), ("alive", C.c_void_p)]


class OkenvQcnnRing(C.Structure):
    _fields_ = [("state", C.c_void_p), ("next_state", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p)]


class OkenvQcnnBatchOut(C.Structure):
    _fields_ = [("state", C.c_void_p), ("next_state", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("index", C.c_void_p)]


def qcnn_config(image_size=96, kernel=(8, 4, 3), stride=(4, 2, 1), padding=(2, 1, 1), channels=(32, 64, 64), hidden=512, num_actions=5,
                mode="greedy", epsilon=0.0, seed=0, agent_base=0, action_table=QCNN_ACTION_MAP):
    """okenv_qcnn_config with the reference's layers, action count and action table as defaults (RLRacers/DQN_CNN: CNN.hpp,
    DQCNNAgent.hpp); mode: "greedy", "eps_greedy" or the number."""
    cfg = OkenvQcnnConfig(int(image_size), (C.c_int32 * 3)(*map(int, kernel)), (C.c_int32 * 3)(*map(int, stride)),
                          (C.c_int32 * 3)(*map(int, padding)), (C.c_int32 * 3)(*map(int, channels)), int(hidden), int(num_actions),
                          ACTOR_MODES.get(mode, mode), float(epsilon), int(seed) & 0xFFFFFFFF, int(agent_base) & 0xFFFFFFFF)
    for i, (thr, steer) in enumerate(action_table):
        cfg.action_table[i][0], cfg.action_table[i][1] = float(thr), float(steer)
    return cfg


def qcnn_sides(cfg):
    """ok_qcnn_side: the sides of the three padded convolutions' outputs (torch's flooring; 0 where the kernel does not fit)."""
    side, out = cfg.image_size, []
    for k, s, p in zip(cfg.kernel, cfg.stride, cfg.padding):
        side = 0 if side + 2 * p < k or s < 1 else (side + 2 * p - k) // s + 1
        out.append(side)
    return tuple(out)


def qcnn_layout(cfg):
    """ok_qcnn_offsets: where every piece of the parameter vector begins, as (name, offset, shape) in order; the names are the
    state-dict keys of the reference's CNN.  The last entry's end is the vector's length."""
    k, c, H, A = list(cfg.kernel), list(cfg.channels), cfg.hidden, cfg.num_actions
    F = c[2] * qcnn_sides(cfg)[2] ** 2
    pieces = []
    for l, cin in enumerate([1] + c[:2]):
        pieces += [("conv%d.weight" % (l + 1), (c[l], cin, k[l], k[l])), ("conv%d.bias" % (l + 1), (c[l],))]
    pieces += [("fc1.weight", (H, F)), ("fc1.bias", (H,)), ("fc2.weight", (A, H)), ("fc2.bias", (A,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def qcnn_num_params(cfg):
    """Floats of the Q-network's parameter vector."""
    name, at, shape = qcnn_layout(cfg)[-1]
    return at + int(np.prod(shape))


def qcnn_lds_bytes(cfg):
    """okenv_qcnn_lds_bytes: the larger act kernel's LDS for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_qcnn_lds_bytes(C.byref(cfg)))


def qcnn_plan(cfg):
    """okenv_qcnn_plan: (tiles of 16 hidden units per wave of the head kernel, what sizes the conv kernel's first LDS region, whether
    planes move as 16-byte vectors), the kernels' paths.  No GPU needed."""
    out = (C.c_int32 * 3)()
    check(load().okenv_qcnn_plan(C.byref(cfg), out))
    return tuple(int(v) for v in out)


def qcnn_act_host(cfg, params, frames, crashed=None, draw_index=0):
    """okenv_qcnn_act_host on numpy arrays: frames [n][S][S][4] uint8 -> dict(throttle, steer, value [n] float32, q [n][A] float32,
    action [n] int64, alive [n] uint8).  No GPU needed."""
    frames = np.ascontiguousarray(frames, np.uint8)
    params = np.ascontiguousarray(params, np.float32)
    n = frames.shape[0]
    assert frames.shape == (n, cfg.image_size, cfg.image_size, 4) and params.size == qcnn_num_params(cfg)
    crashed = None if crashed is None else np.ascontiguousarray(crashed, np.uint8)
    out = dict(throttle=np.empty(n, np.float32), steer=np.empty(n, np.float32), q=np.empty((n, cfg.num_actions), np.float32),
               action=np.empty(n, np.int64), value=np.empty(n, np.float32), alive=np.empty(n, np.uint8))
    check(load().okenv_qcnn_act_host(C.byref(cfg), ptr(params), n, ptr(frames), ptr(crashed), int(draw_index) & 0xFFFFFFFF, ptr(out["throttle"]),
                                     ptr(out["steer"]), ptr(out["q"]), ptr(out["action"]), ptr(out["value"]), ptr(out["alive"])))
    return out


def qcnn_ring(capacity, image_size):
    """An empty host-side frame ring: dict of zeroed numpy arrays (state, next_state [C][S][S]; action int64, reward, done [C]), its
    "pushed" count, "capacity" and "image_size"."""
    C_, S = int(capacity), int(image_size)
    return dict(state=np.zeros((C_, S, S), np.float32), next_state=np.zeros((C_, S, S), np.float32), action=np.zeros(C_, np.int64),
                reward=np.zeros(C_, np.float32), done=np.zeros(C_, np.float32), pushed=0, capacity=C_, image_size=S)


def _qcnn_ring_struct(ring):
    return fill_pointers(OkenvQcnnRing(), {k: ring[k] for k in ("state", "next_state", "action", "reward", "done")}, "ring")


def qcnn_push_host(ring, action, alive, frames, next_frames, crashed, reward=None, dist=None, push_all=False):
    """One push on host arrays, no GPU needed (okenv_qcnn_push_host): `ring` (qcnn_ring(...)) is updated in place, "pushed" included."""
    S = ring["image_size"]
    frames, next_frames = np.ascontiguousarray(frames, np.uint8), np.ascontiguousarray(next_frames, np.uint8)
    n = frames.shape[0]
    assert frames.shape == next_frames.shape == (n, S, S, 4)
    action = np.ascontiguousarray(action, np.int64)
    alive = None if alive is None else np.ascontiguousarray(alive, np.uint8)
    crashed = np.ascontiguousarray(crashed, np.uint8)
    reward = None if reward is None else np.ascontiguousarray(reward, np.float32)
    dist = None if dist is None else np.ascontiguousarray(dist, np.float32)
    pushed = C.c_uint64(ring["pushed"])
    check(load().okenv_qcnn_push_host(C.byref(_qcnn_ring_struct(ring)), ring["capacity"], S, C.byref(pushed), REPLAY_PUSH_ALL if push_all else 0, n,
                                      ptr(action), ptr(alive), ptr(frames), ptr(next_frames), ptr(crashed), ptr(reward), ptr(dist),
                                      0 if dist is None else dist.shape[1]))
    ring["pushed"] = int(pushed.value)
    return ring


def qcnn_batch_host(ring, B, mode="sequential", start_or_draw=0, seed=0):
    """B positions of a host-side ring (okenv_qcnn_batch_host): dict(state, next_state [B][S][S], action, reward, done, index [B])."""
    S, B = ring["image_size"], int(B)
    out = dict(state=np.full((B, S, S), -7.0, np.float32), next_state=np.full((B, S, S), -7.0, np.float32), action=np.full(B, -7, np.int64),
               reward=np.full(B, -7.0, np.float32), done=np.full(B, -7.0, np.float32), index=np.full(B, -7, np.int32))
    check(load().okenv_qcnn_batch_host(C.byref(_qcnn_ring_struct(ring)), ring["capacity"], S, int(ring["pushed"]), int(seed) & 0xFFFFFFFF, B,
                                       QCNN_BATCH_MODES.get(mode, mode), int(start_or_draw), C.byref(fill_pointers(OkenvQcnnBatchOut(), out, "batch"))))
    return out


def qcnn_grey_host(frames):
    """The rule's grey planes [n][S][S] float32 of frames [n][S][S][4] uint8 (a test hook).  No GPU needed."""
    frames = np.ascontiguousarray(frames, np.uint8)
    n, S = frames.shape[0], frames.shape[1]
    assert frames.shape == (n, S, S, 4)
    out = np.empty((n, S, S), np.float32)
    check(load().okenv_debug_qcnn_grey_host(S, n, ptr(frames), ptr(out)))
    return out


# image transformer driver (include/okenv.h)
VIT_LDS_BUDGET = 160 * 1024
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class OkenvVitConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("patch", C.c_int32), ("dim", C.c_int32), ("heads", C.c_int32), ("depth", C.c_int32),
                ("dim_feedforward", C.c_int32), ("head_hidden1", C.c_int32), ("head_hidden2", C.c_int32), ("mean", C.c_float * 3),
                ("std", C.c_float * 3), ("ln_eps", C.c_float), ("throttle", C.c_float), ("steer_scale", C.c_float),
                ("agents_per_pass", C.c_int32), ("workspace_bytes", C.c_int64)]


class OkenvVitRecord(C.Structure):
    _fields_ = [("action", C.c_void_p), ("output", C.c_void_p), ("embedding", C.c_void_p), ("alive", C.c_void_p)]


def vit_config(image_size=224, patch=8, dim=384, heads=6, depth=12, dim_feedforward=1536, head_hidden1=128, head_hidden2=64,
               mean=IMAGENET_MEAN, std=IMAGENET_STD, ln_eps=1e-6, throttle=100.0, steer_scale=10.0, agents_per_pass=0, workspace_bytes=0):
    """okenv_vit_config with the reference's shape and controls as defaults (DinoControl: timm's vit_small_patch8_224.dino, the
    384-128-64-1 head, main_dino_control.cpp:80-89)."""
    return OkenvVitConfig(int(image_size), int(patch), int(dim), int(heads), int(depth), int(dim_feedforward), int(head_hidden1),
                          int(head_hidden2), (C.c_float * 3)(*map(float, mean)), (C.c_float * 3)(*map(float, std)), float(ln_eps),
                          float(throttle), float(steer_scale), int(agents_per_pass), int(workspace_bytes))


def vit_tokens(cfg):
    return (cfg.image_size // cfg.patch) ** 2 + 1


def vit_layout(cfg):
    """ok_vit_offsets: where every piece of the parameter vector begins, as (name, offset, shape) in order; the names are timm's
    state-dict keys with the head's behind them (openkitchen_amd/dino.py: DinoPolicy)."""
    D, F, P, T = cfg.dim, cfg.dim_feedforward, cfg.patch, vit_tokens(cfg)
    pieces = [("cls_token", (1, 1, D)), ("pos_embed", (1, T, D)), ("patch_embed.proj.weight", (D, 3, P, P)), ("patch_embed.proj.bias", (D,))]
    for i in range(cfg.depth):
        pre = "blocks.%d." % i
        pieces += [(pre + "norm1.weight", (D,)), (pre + "norm1.bias", (D,)), (pre + "attn.qkv.weight", (3 * D, D)), (pre + "attn.qkv.bias", (3 * D,)),
                   (pre + "attn.proj.weight", (D, D)), (pre + "attn.proj.bias", (D,)), (pre + "norm2.weight", (D,)), (pre + "norm2.bias", (D,)),
                   (pre + "mlp.fc1.weight", (F, D)), (pre + "mlp.fc1.bias", (F,)), (pre + "mlp.fc2.weight", (D, F)), (pre + "mlp.fc2.bias", (D,))]
    pieces += [("norm.weight", (D,)), ("norm.bias", (D,)), ("head.net.0.weight", (cfg.head_hidden1, D)), ("head.net.0.bias", (cfg.head_hidden1,)),
               ("head.net.2.weight", (cfg.head_hidden2, cfg.head_hidden1)), ("head.net.2.bias", (cfg.head_hidden2,)),
               ("head.output_layer.weight", (1, cfg.head_hidden2)), ("head.output_layer.bias", (1,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def vit_num_params(cfg):
    name, at, shape = vit_layout(cfg)[-1]
    return at + int(np.prod(shape))


def vit_lds_bytes(cfg):
    """okenv_vit_lds_bytes: the largest LDS of the act's kernels for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_vit_lds_bytes(C.byref(cfg)))


def vit_act_host(cfg, params, frames, crashed=None):
    """okenv_vit_act_host on numpy arrays: frames [n][S][S][4] uint8 -> dict(throttle, steer, output [n], embedding [n][D] float32,
    alive [n]).  No GPU needed."""
    frames = np.ascontiguousarray(frames, np.uint8)
    params = np.ascontiguousarray(params, np.float32)
    n = frames.shape[0]
    assert frames.shape == (n, cfg.image_size, cfg.image_size, 4) and params.size == vit_num_params(cfg)
    crashed = None if crashed is None else np.ascontiguousarray(crashed, np.uint8)
    out = dict(throttle=np.empty(n, np.float32), steer=np.empty(n, np.float32), output=np.empty(n, np.float32),
               embedding=np.empty((n, cfg.dim), np.float32), alive=np.empty(n, np.uint8))
    check(load().okenv_vit_act_host(C.byref(cfg), ptr(params), n, ptr(frames), ptr(crashed), ptr(out["throttle"]), ptr(out["steer"]),
                                    ptr(out["output"]), ptr(out["embedding"]), ptr(out["alive"])))
    return out


def debug_vit_attend(qkv, heads, device=DEBUG_ON_HOST):
    """okenv_debug_vit_attend: qkv [seqs][T][3 heads dh] -> ctx [seqs][T][heads dh]; device < 0 evaluates the rule on the host."""
    qkv = np.ascontiguousarray(qkv, np.float32)
    seqs, T, W = qkv.shape
    D = W // 3
    out = np.empty((seqs, T, D), np.float32)
    check(load().okenv_debug_vit_attend(int(device), seqs, T, int(heads), D // int(heads), ptr(qkv), ptr(out)))
    return out


# the image transformer driver's training (include/okenv.h)
VIT_HEAD_CHUNK = 64


class OkenvVitHeadParams(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight", C.c_float), ("threshold", C.c_float)]


class OkenvVitHeadState(C.Structure):
    _fields_ = [("params", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("t", C.c_int64)]


class OkenvVitHeadOutput(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("grad", C.c_void_p)]


def vit_head_params(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight=5.0, threshold=0.1):
    """okenv_vit_head_params with the reference's values as defaults (train_dino_control.py)."""
    return OkenvVitHeadParams(float(lr), float(beta1), float(beta2), float(eps), float(weight), float(threshold))


def vit_head_num_params(D, H1, H2):
    return H1 * D + H1 + H2 * H1 + H2 + H2 + 1


def vit_head_offset(cfg):
    """Where the head begins in the driver's parameter vector (vit_layout's head.net.0.weight)."""
    return vit_num_params(cfg) - vit_head_num_params(cfg.dim, cfg.head_hidden1, cfg.head_hidden2)


def vit_head_lds_bytes(D, H1, H2):
    """okenv_vit_head_lds_bytes: the LDS of the update's forward kernel, 0 outside the limits.  No GPU needed."""
    return int(load().okenv_vit_head_lds_bytes(int(D), int(H1), int(H2)))


def vit_head_update_host(params, shape, steer_scale, state, embedding, steer, B, epochs=1, order=None, want=("loss", "grad")):
    """The head's update on host arrays, no GPU needed (okenv_vit_head_update_host).  params: vit_head_params(...); shape: (D, H1, H2);
    state: dict of float32 numpy arrays "params", "m", "v" (the head's slice) and the int "t" -- copied, the new state is returned;
    embedding [M, D], steer [M]; order: None or int32 [epochs, M].  Returns (new state, outputs): "loss" holds one value per
    minibatch, "grad" the last minibatch's gradient."""
    D, H1, H2 = (int(v) for v in shape)
    embedding = None if embedding is None else np.ascontiguousarray(embedding, np.float32)
    steer = None if steer is None else np.ascontiguousarray(steer, np.float32)
    M = int(steer.shape[0]) if steer is not None else 0
    new = {k: np.array(v, dtype=np.float32, copy=True).ravel() for k, v in state.items() if k != "t" and v is not None}
    st = fill_pointers(OkenvVitHeadState(), new, "vit head state")
    st.t = int(state.get("t", 0))
    steps = int(epochs) * ((M + int(B) - 1) // int(B)) if M > 0 and B > 0 and epochs > 0 else 0
    sizes = {"loss": steps, "grad": vit_head_num_params(D, H1, H2)}
    outs = {k: np.zeros(sizes[k], dtype=np.float32) for k in want}
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int32)
    check(load().okenv_vit_head_update_host(C.byref(params) if params is not None else None, D, H1, H2, float(steer_scale), C.byref(st), ptr(embedding),
                                            ptr(steer), M, int(B), int(epochs), ptr(order),
                                            C.byref(fill_pointers(OkenvVitHeadOutput(), {k: v for k, v in outs.items() if v.size}, "vit head output"))))
    new["t"] = int(st.t)
    return new, outs


def vit_head_eval_host(params, shape, steer_scale, head, embedding, steer, B):
    """okenv_vit_head_eval_host: the loss of every minibatch of one sequential pass, float32 [ceil(M / B)].  No GPU needed."""
    D, H1, H2 = (int(v) for v in shape)
    head, embedding, steer = (np.ascontiguousarray(a, np.float32) for a in (head, embedding, steer))
    M = int(steer.shape[0])
    loss = np.zeros((M + int(B) - 1) // int(B) if M > 0 and B > 0 else 0, np.float32)
    check(load().okenv_vit_head_eval_host(C.byref(params), D, H1, H2, float(steer_scale), ptr(head), ptr(embedding), ptr(steer), M, int(B), ptr(loss)))
    return loss


def qcnn_forward_planes_host(cfg, params, planes):
    """The network of okenv_qcnn_act_host on grey planes [n][S][S] float32 -> q [n][A] (a test hook).  No GPU needed."""
    planes, params = np.ascontiguousarray(planes, np.float32), np.ascontiguousarray(params, np.float32)
    n = planes.shape[0]
    assert planes.shape == (n, cfg.image_size, cfg.image_size) and params.size == qcnn_num_params(cfg)
    out = np.empty((n, cfg.num_actions), np.float32)
    check(load().okenv_debug_qcnn_forward_planes_host(C.byref(cfg), ptr(params), n, ptr(planes), ptr(out)))
    return out


# world-model racers (include/okenv.h)
WORLD_LDS_BUDGET = 160 * 1024
WORLD_ENCODER, WORLD_CONTROLLERS = 0, 1
WORLD_VECTORS = {"encoder": WORLD_ENCODER, "controllers": WORLD_CONTROLLERS}
WORLD_STAGE_LIST, WORLD_STAGE_CONV0, WORLD_STAGE_LATENT, WORLD_STAGE_HEAD = 1, 2, 32, 64  # CONV0 << l: layer l
WORLD_STAGES = (("list", 1), ("conv0", 2), ("conv1", 4), ("conv2", 8), ("conv3", 16), ("latent", 32), ("head", 64))
WORLD_COLS, WORLD_CHUNK = 128, 64  # output channels per workgroup and input channels per K block (ok_world.h)


class OkenvWorldConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("channels", C.c_int32 * 4), ("latent", C.c_int32), ("hidden", C.c_int32),
                ("throttle", C.c_float), ("steer_scale", C.c_float), ("skip_crashed", C.c_int32)]


class OkenvWorldRecord(C.Structure):
    _fields_ = [("mu", C.c_void_p), ("state", C.c_void_p), ("out", C.c_void_p), ("action", C.c_void_p), ("alive", C.c_void_p)]


def world_config(image_size=128, channels=(64, 128, 256, 512), latent=32, hidden=16, throttle=100.0, steer_scale=5.0, skip_crashed=0):
    """okenv_world_config with the reference's shape and controls as defaults (WorldModelVaeRnn: train_vae.py's defaults, main.cpp)."""
    return OkenvWorldConfig(int(image_size), (C.c_int32 * 4)(*map(int, channels)), int(latent), int(hidden), float(throttle),
                            float(steer_scale), int(skip_crashed))


def world_layout(cfg):
    """ok_world_offsets: where every piece of the encoder vector begins, as (name, offset, shape) in order; the names are the
    state-dict keys of the reference's Encoder (the BatchNorm layers net.3 / net.6 / net.9 are folded into the convolutions in front
    of them).  The last entry's end is the vector's length."""
    c = list(cfg.channels)
    F = c[3] * (cfg.image_size // 16) ** 2
    pieces = []
    for l, cin in enumerate([3] + c[:3]):
        name = "net.%d" % (0, 2, 5, 8)[l]
        pieces += [(name + ".weight", (c[l], cin, 4, 4)), (name + ".bias", (c[l],))]
    pieces += [("fc_mu.weight", (cfg.latent, F)), ("fc_mu.bias", (cfg.latent,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def world_num_params(cfg):
    """(floats of the encoder vector, floats of one agent's controller: ok_controller_num_params(latent + 2, hidden, 1))."""
    name, at, shape = world_layout(cfg)[-1]
    i, h = cfg.latent + 2, cfg.hidden
    return at + int(np.prod(shape)), h * i + h + (h // 2) * h + h // 2 + h // 2 + 1


def world_lds_bytes(cfg):
    """okenv_world_lds_bytes: the largest act kernel's LDS for the shape, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_world_lds_bytes(C.byref(cfg)))


def world_plan(cfg):
    """okenv_world_plan: per convolution (workgroups its output channels take, K blocks per tap -- 0 for layer 0 --, channels of a tap's
    last block).  No GPU needed."""
    out = (C.c_int32 * 12)()
    check(load().okenv_world_plan(C.byref(cfg), out))
    return tuple(tuple(int(v) for v in out[3 * l:3 * l + 3]) for l in range(4))


def world_workspace_bytes(cfg, num_agents):
    """okenv_world_workspace_bytes: device bytes okenv_world_create allocates for num_agents; 0 for a refused shape."""
    return int(load().okenv_world_workspace_bytes(C.byref(cfg), int(num_agents)))


def world_act_host(cfg, encoder, controllers, frames, rot, crashed=None, into=None):
    """okenv_world_act_host on numpy arrays: frames [n][S][S][4] uint8, rot [n] (degrees, as stored), controllers [n][.] ->
    dict(mu [n][Z], state [n][Z+2], out, throttle, steer [n] float32, alive [n] uint8).  into: such a dict to write into (with
    skip_crashed the entries of crashed agents keep what it holds).  No GPU needed."""
    frames = np.ascontiguousarray(frames, np.uint8)
    encoder = np.ascontiguousarray(encoder, np.float32)
    controllers = np.ascontiguousarray(controllers, np.float32)
    rot = np.ascontiguousarray(rot, np.float32)
    n, Z = frames.shape[0], cfg.latent
    ne, nc = world_num_params(cfg)
    assert frames.shape == (n, cfg.image_size, cfg.image_size, 4) and encoder.size == ne and controllers.size == n * nc and rot.size == n
    crashed = None if crashed is None else np.ascontiguousarray(crashed, np.uint8)
    out = into if into is not None else dict(
        mu=np.zeros((n, Z), np.float32), state=np.zeros((n, Z + 2), np.float32), out=np.zeros(n, np.float32),
        throttle=np.zeros(n, np.float32), steer=np.zeros(n, np.float32), alive=np.zeros(n, np.uint8))
    check(load().okenv_world_act_host(C.byref(cfg), ptr(encoder), ptr(controllers), n, ptr(frames), ptr(rot), ptr(crashed), ptr(out["mu"]),
                                      ptr(out["state"]), ptr(out["out"]), ptr(out["throttle"]), ptr(out["steer"]), ptr(out["alive"])))
    return out


def world_score_host(cx, cy, w_left, w_right, x, y, crashed, timed_out, fitness):
    """okenv_world_score_host: one okenv_world_score on host arrays; returns the new fitness [n].  No GPU needed."""
    cx, cy, w_left, w_right, x, y = (np.ascontiguousarray(v, np.float32) for v in (cx, cy, w_left, w_right, x, y))
    crashed, timed_out = np.ascontiguousarray(crashed, np.uint8), np.ascontiguousarray(timed_out, np.uint8)
    fitness = np.array(fitness, np.float32)
    assert cx.size == cy.size == w_left.size == w_right.size and x.size == y.size == crashed.size == timed_out.size == fitness.size
    check(load().okenv_world_score_host(ptr(cx), ptr(cy), ptr(w_left), ptr(w_right), cx.size, x.size, ptr(x), ptr(y), ptr(crashed),
                                        ptr(timed_out), ptr(fitness)))
    return fitness


# the world-model racers' memory (include/okenv.h)
MEMORY_NETWORK, MEMORY_CONTROLLERS = 0, 1
MEMORY_VECTORS = {"network": MEMORY_NETWORK, "controllers": MEMORY_CONTROLLERS}
MEMORY_STAGE_ENCODER, MEMORY_STAGE_INPUT, MEMORY_STAGE_LAYER0, MEMORY_STAGE_HEAD = 1, 2, 4, 64  # LAYER0 << l: layer l
MEMORY_COLS, MEMORY_CHUNK, MEMORY_ROWS = 32, 64, 128  # hidden units and list slots per workgroup, k's per K block (ok_memory.h)
MEMORY_RECORD = ("mu", "hidden", "prediction", "state", "out", "action", "alive")


class OkenvMemoryConfig(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("layers", C.c_int32), ("ctrl_hidden", C.c_int32), ("carry", C.c_int32), ("throttle", C.c_float),
                ("steer_scale", C.c_float)]


class OkenvMemoryRecord(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in MEMORY_RECORD]


def memory_config(hidden=512, layers=3, ctrl_hidden=16, carry=1, throttle=100.0, steer_scale=5.0):
    """okenv_memory_config with the reference's shape and controls as defaults (WorldModelVaeRnn: train_rnn.py's defaults, main.cpp);
    carry=0 is the reference as written (every act starts from a zero hidden state)."""
    return OkenvMemoryConfig(int(hidden), int(layers), int(ctrl_hidden), int(carry), float(throttle), float(steer_scale))


def memory_layout(world, cfg):
    """ok_memory_offsets: where every piece of the network vector begins, as (name, offset, shape) in order: the state-dict keys of
    worldmodel.GRUDynamics, then the statistics z_mean, z_std, a_mean, a_std.  The last entry's end is the vector's length."""
    Z, H = world.latent, cfg.hidden
    pieces = []
    for l in range(cfg.layers):
        pieces += [("gru.weight_ih_l%d" % l, (3 * H, Z + 2 if l == 0 else H)), ("gru.weight_hh_l%d" % l, (3 * H, H)),
                   ("gru.bias_ih_l%d" % l, (3 * H,)), ("gru.bias_hh_l%d" % l, (3 * H,))]
    pieces += [("head.weight", (Z, H)), ("head.bias", (Z,)), ("z_mean", (Z,)), ("z_std", (Z,)), ("a_mean", (2,)), ("a_std", (2,))]
    out, at = [], 0
    for name, shape in pieces:
        out.append((name, at, shape))
        at += int(np.prod(shape))
    return out


def memory_num_params(world, cfg):
    """(floats of the network vector, floats of one agent's controller: ok_controller_num_params(latent + hidden, ctrl_hidden, 1))."""
    name, at, shape = memory_layout(world, cfg)[-1]
    i, h = world.latent + cfg.hidden, cfg.ctrl_hidden
    return at + int(np.prod(shape)), h * i + h + (h // 2) * h + h // 2 + h // 2 + 1


def memory_lds_bytes(world, cfg):
    """okenv_memory_lds_bytes: the layer kernel's LDS, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_memory_lds_bytes(C.byref(world), C.byref(cfg)))


def memory_plan(world, cfg):
    """okenv_memory_plan: (column blocks of a layer, live column tiles of the last, K blocks of layer 0's input, k's of the last, K blocks
    of a chain over the hidden width, k's of the last, carry, layers).  No GPU needed."""
    out = (C.c_int32 * 8)()
    check(load().okenv_memory_plan(C.byref(world), C.byref(cfg), out))
    return tuple(int(v) for v in out)


def memory_workspace_bytes(world, cfg, num_agents):
    """okenv_memory_workspace_bytes: device bytes okenv_memory_create allocates for num_agents; 0 for a refused shape."""
    return int(load().okenv_memory_workspace_bytes(C.byref(world), C.byref(cfg), int(num_agents)))


def memory_act_host(world, cfg, encoder, network, controllers, frames, hidden, throttle, steer, crashed=None, into=None):
    """okenv_memory_act_host on numpy arrays: frames [n][S][S][4] uint8, hidden [n][L][H], throttle and steer [n] (the stored action) ->
    dict of the record's members (capi.MEMORY_RECORD) plus "hidden_state" [n][L][H], "throttle" and "steer" [n], the new ones; the
    arguments are not written.  into: such a dict to write into (with skip_crashed the entries of crashed agents keep what it holds;
    its hidden_state, throttle and steer are then the inputs too).  No GPU needed."""
    frames = np.ascontiguousarray(frames, np.uint8)
    encoder, network, controllers = (np.ascontiguousarray(v, np.float32) for v in (encoder, network, controllers))
    n, Z, H, L = frames.shape[0], world.latent, cfg.hidden, cfg.layers
    nn, nc = memory_num_params(world, cfg)
    assert frames.shape == (n, world.image_size, world.image_size, 4) and encoder.size == world_num_params(world)[0]
    assert network.size == nn and controllers.size == n * nc
    crashed = None if crashed is None else np.ascontiguousarray(crashed, np.uint8)
    if into is None:
        out = dict(mu=np.zeros((n, Z), np.float32), hidden=np.zeros((n, H), np.float32), prediction=np.zeros((n, Z), np.float32),
                   state=np.zeros((n, Z + H), np.float32), out=np.zeros(n, np.float32), action=np.zeros((n, 2), np.float32),
                   alive=np.zeros(n, np.uint8), hidden_state=np.array(hidden, np.float32).reshape(n, L, H),
                   throttle=np.array(throttle, np.float32).reshape(n), steer=np.array(steer, np.float32).reshape(n))
    else:
        out = into
    rec = fill_pointers(OkenvMemoryRecord(), {k: out.get(k) for k in MEMORY_RECORD}, "record")
    check(load().okenv_memory_act_host(C.byref(world), C.byref(cfg), ptr(encoder), ptr(network), ptr(controllers), n, ptr(frames), ptr(crashed),
                                       ptr(out["hidden_state"]), ptr(out["throttle"]), ptr(out["steer"]), C.byref(rec)))
    return out


# the memory's training (include/okenv.h)
MEMORY_TRAIN_BLOCK, MEMORY_TRAIN_MAX_SEQ = 64, 16


class OkenvMemoryLearnerConfig(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("clip_grad", C.c_float),
                ("seq_len", C.c_int32), ("max_batch", C.c_int32)]


class OkenvMemoryLearnerState(C.Structure):
    _fields_ = [("params", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("t", C.c_int64)]


class OkenvMemoryLearnerOutput(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("norm", C.c_void_p), ("grad", C.c_void_p)]


def memory_learner_config(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, clip_grad=1.0, seq_len=5, max_batch=256):
    """okenv_memory_learner_config with train_rnn.py's values as defaults."""
    return OkenvMemoryLearnerConfig(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(clip_grad), int(seq_len), int(max_batch))


def memory_trainable(world, cfg):
    """Floats of the trainable prefix of the network vector: everything in front of the statistics."""
    return memory_num_params(world, cfg)[0] - (2 * world.latent + 4)


def memory_learner_workspace_bytes(world, cfg, learner):
    """okenv_memory_learner_workspace_bytes: device bytes okenv_memory_learner_create allocates; 0 for a refused argument.  No GPU needed."""
    return int(load().okenv_memory_learner_workspace_bytes(C.byref(world), C.byref(cfg), C.byref(learner)))


def memory_learner_lds_bytes(world, cfg):
    """okenv_memory_learner_lds_bytes: the LDS of the learner's largest kernel.  No GPU needed."""
    return int(load().okenv_memory_learner_lds_bytes(C.byref(world), C.byref(cfg)))


def _memory_windows_args(world, latent, action, start):
    latent = None if latent is None else np.ascontiguousarray(latent, np.float32).reshape(-1, world.latent)
    action = None if action is None else np.ascontiguousarray(action, np.float32).reshape(-1, 2)
    start = None if start is None else np.ascontiguousarray(start, np.int32).ravel()
    return latent, action, start, (int(latent.shape[0]) if latent is not None else 0), (int(start.size) if start is not None else 0)


def memory_update_host(world, cfg, learner, state, latent, action, start, B, stride=1, epochs=1, order=None, lr_schedule=None, want=("loss", "norm", "grad")):
    """The memory's update on host arrays, no GPU needed (okenv_memory_update_host).  state: dict of float32 numpy arrays "params" (the
    whole network vector), "m", "v" (its trainable prefix) and the int "t" -- copied, the new state is returned; latent [rows, Z],
    action [rows, 2], start [M] int32; order: None or int32 [epochs, M]; lr_schedule: None or float32 [epochs * ceil(M / B)].  Returns
    (new state, outputs): "loss" and "norm" hold one value per minibatch, "grad" the last minibatch's clipped gradient."""
    latent, action, start, rows, M = _memory_windows_args(world, latent, action, start)
    new = {k: np.array(v, dtype=np.float32, copy=True).ravel() for k, v in state.items() if k != "t" and v is not None}
    st = fill_pointers(OkenvMemoryLearnerState(), new, "memory learner state")
    st.t = int(state.get("t", 0))
    steps = int(epochs) * ((M + int(B) - 1) // int(B)) if M > 0 and B > 0 and epochs > 0 else 0
    sizes = {"loss": steps, "norm": steps, "grad": memory_trainable(world, cfg)}
    outs = {k: np.zeros(sizes[k], dtype=np.float32) for k in want}
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    lr_schedule = None if lr_schedule is None else np.ascontiguousarray(lr_schedule, dtype=np.float32)
    assert lr_schedule is None or lr_schedule.size == steps
    check(load().okenv_memory_update_host(C.byref(world), C.byref(cfg), C.byref(learner) if learner is not None else None, C.byref(st), ptr(latent), ptr(action),
                                          rows, ptr(start), M, int(stride), int(B), int(epochs), ptr(order), ptr(lr_schedule),
                                          C.byref(fill_pointers(OkenvMemoryLearnerOutput(), {k: v for k, v in outs.items() if v.size}, "memory learner output"))))
    new["t"] = int(st.t)
    return new, outs


def memory_eval_host(world, cfg, learner, network, latent, action, start, B, stride=1):
    """okenv_memory_eval_host: the loss of every minibatch of one sequential pass, float32 [ceil(M / B)].  No GPU needed."""
    latent, action, start, rows, M = _memory_windows_args(world, latent, action, start)
    network = np.ascontiguousarray(network, np.float32)
    loss = np.zeros((M + int(B) - 1) // int(B) if M > 0 and B > 0 else 0, np.float32)
    check(load().okenv_memory_eval_host(C.byref(world), C.byref(cfg), C.byref(learner), ptr(network), ptr(latent), ptr(action), rows, ptr(start), M, int(stride),
                                        int(B), ptr(loss)))
    return loss


def memory_window_host(world, cfg, network, latent, action, start, seq_len, stride=1):
    """okenv_memory_window_host: the update's forward of one window -> (hidden [S, L, H], zn [S, Z]).  No GPU needed."""
    latent, action, _, rows, _ = _memory_windows_args(world, latent, action, None)
    network = np.ascontiguousarray(network, np.float32)
    hidden = np.zeros((int(seq_len), cfg.layers, cfg.hidden), np.float32)
    zn = np.zeros((int(seq_len), world.latent), np.float32)
    check(load().okenv_memory_window_host(C.byref(world), C.byref(cfg), ptr(network), ptr(latent), ptr(action), rows, int(start), int(stride), int(seq_len),
                                          ptr(hidden), ptr(zn)))
    return hidden, zn


# guided cost learning (include/okenv.h)
GCL_POLICY,GCL_VALUE, GCL_COST = 0, 1, 2
GCL_NETWORKS = {"policy": GCL_POLICY, "value": GCL_VALUE, "cost": GCL_COST}
GCL_KERNELS = ("grad", "step")
GCL_LDS_BUDGET = 160 * 1024


class OkenvGclConfig(C.Structure):
    _fields_ = [("hidden1", C.c_int32), ("hidden2", C.c_int32), ("cost_hidden1", C.c_int32), ("cost_hidden2", C.c_int32), ("scale", C.c_float * 2),
                ("bias", C.c_float * 2), ("greedy", C.c_int32), ("seed", C.c_uint32), ("agent_base", C.c_uint32)]


class OkenvGclRecord(C.Structure):
    _fields_ = [("state", C.c_void_p), ("eps", C.c_void_p), ("pre", C.c_void_p), ("squashed", C.c_void_p), ("action", C.c_void_p),
                ("logp", C.c_void_p), ("alive", C.c_void_p)]


class OkenvGclState(C.Structure):
    _fields_ = [("params", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("t", C.c_int64)]


class OkenvGclCostBatch(C.Structure):
    _fields_ = [("state", C.c_void_p), ("squashed", C.c_void_p)]


class OkenvGclCostOutput(C.Structure):
    _fields_ = [("loss", C.c_void_p), ("grad", C.c_void_p)]


class OkenvGclUpdateConfig(C.Structure):
    _fields_ = [("accumulate", C.c_int32), ("reduce", C.c_int32)]


class OkenvGclBatch(C.Structure):
    _fields_ = [("state", C.c_void_p), ("pre", C.c_void_p), ("logp", C.c_void_p), ("ret", C.c_void_p)]


class OkenvGclOutput(C.Structure):
    _fields_ = [("policy_loss", C.c_void_p), ("value_loss", C.c_void_p), ("clipped", C.c_void_p), ("grad_policy", C.c_void_p),
                ("grad_value", C.c_void_p), ("adv", C.c_void_p)]


def gcl_config(hidden1=64, hidden2=64, cost_hidden1=64, cost_hidden2=64, scale=(50.0, 10.0), bias=(50.0, 0.0), greedy=False, seed=0, agent_base=0):
    """okenv_gcl_config with the reference's widths and action ranges as defaults (Networks.hpp, GCLAgent.hpp:64-72)."""
    return OkenvGclConfig(int(hidden1), int(hidden2), int(cost_hidden1), int(cost_hidden2), (C.c_float * 2)(*map(float, scale)),
                          (C.c_float * 2)(*map(float, bias)), int(greedy), int(seed) & 0xFFFFFFFF, int(agent_base) & 0xFFFFFFFF)


def gcl_update_config(accumulate=True, reduce="mean"):
    """okenv_gcl_update_config with the reference's choices as defaults (one step on the mean); reduce: "sum" / "mean" or the integer."""
    return OkenvGclUpdateConfig(1 if accumulate else 0, REINFORCE_REDUCE[reduce] if isinstance(reduce, str) else int(reduce))


def gcl_num_params(which, R, H1, H2):
    """Floats of a network's parameter vector; which: "policy" [log_std | fc1 | fc2 | fc3] (R -> H1 -> H2 -> 2), "value" [fc1 | fc2 | fc3]
    (R -> H1 -> H2 -> 1) or "cost" (R + 2 -> H1 -> H2 -> 1), or the integer."""
    which = GCL_NETWORKS[which] if isinstance(which, str) else int(which)
    n_in, out, nls = (R + 2 if which == GCL_COST else R), (2 if which == GCL_POLICY else 1), (2 if which == GCL_POLICY else 0)
    return nls + H1 * n_in + H1 + H2 * H1 + H2 + out * H2 + out


def gcl_lds_bytes(R, H1, H2, C1, C2):
    """okenv_gcl_lds_bytes: the largest gradient kernel's LDS for the shapes, 0 outside the rule's limits.  No GPU needed."""
    return int(load().okenv_gcl_lds_bytes(int(R), int(H1), int(H2), int(C1), int(C2)))


@functools.lru_cache(maxsize=None)
def _members(struct_type):
    return frozenset(name for name, _ in struct_type._fields_)


def fill_pointers(struct, given, what, sizes=None, strided=False):
    """Sets the pointer members of a ctypes struct from a dict of tensors / arrays / addresses (None: left NULL): the one way a dict
    of slots becomes a struct of the C ABI.  A key that is no member raises KeyError; arrays and tensors must be contiguous.
    sizes: {slot: bytes}, the least a tensor under that slot may hold.  strided=True hands tensors over by their first element without
    the contiguity check, for callers that state the strides themselves (batch_prepare)."""
    names = _members(type(struct))
    for k, v in given.items():
        if k not in names:
            raise KeyError("unknown %s slot %r" % (what, k))
        if v is None:
            continue
        if hasattr(v, "data_ptr"):  # torch tensor: on the act -> step -> push path, so without the detour through ptr()
            assert strided or v.is_contiguous(), "%s slot %r is not contiguous" % (what, k)
            assert sizes is None or v.numel() * v.element_size() >= sizes[k], "%s slot %r is too small" % (what, k)
            setattr(struct, k, v.data_ptr())
        else:
            setattr(struct, k, ptr(v).value)
    return struct


def batch_stats_dict(raw):
    """okenv_batch_stats from its 56 bytes (a numpy uint8 array, or anything np.frombuffer takes) as a dict."""
    s = OkenvBatchStats.from_buffer_copy(np.ascontiguousarray(raw).tobytes()[:BATCH_STATS_BYTES])
    return {name: getattr(s, name) for name, _ in s._fields_ if name != "reserved"}


PLAN_FIRST_ROLLOUT = -2


class OkenvPlanQuery(C.Structure):
    """okenv_plan_query; the defaults are a stored-action okenv_step with every launch variable unset."""
    _fields_ = [("num_agents", C.c_int32), ("num_rays", C.c_int32), ("compute_units", C.c_int32), ("flags", C.c_uint32),
                ("image_fits_lds", C.c_int32), ("lanes_per_agent", C.c_int32), ("block_threads", C.c_int32), ("coop", C.c_int32),
                ("agents_per_block", C.c_int32), ("tail_max_agents", C.c_int32), ("resident", C.c_int32), ("front_back", C.c_int32),
                ("phase1_range", C.c_float), ("image_bytes", C.c_int32), ("front_back_bytes", C.c_int32), ("q_bytes", C.c_int32),
                ("action_source", C.c_int32), ("n_listed", C.c_int32), ("packed", C.c_int32), ("resident_launch", C.c_int32),
                ("do_move", C.c_int32), ("reset_flags", C.c_uint32), ("ctrl_num_params", C.c_int32)]
    DEFAULTS = dict(compute_units=256, image_fits_lds=1, coop=1, agents_per_block=-1, tail_max_agents=-1, resident=-1, front_back=1,
                    phase1_range=-1.0, n_listed=-1, do_move=1)


class OkenvPlanResult(C.Structure):
    _fields_ = [("lanes_per_agent", C.c_int32), ("natural_lanes", C.c_int32), ("rays_per_lane", C.c_int32), ("phase1_range", C.c_float),
                ("grid_cell", C.c_float), ("grid_mode", C.c_int32), ("front_back_built", C.c_int32), ("block_threads", C.c_int32),
                ("grid_blocks", C.c_int32), ("coop", C.c_int32), ("agents_per_block", C.c_int32), ("tail_max_agents", C.c_int32),
                ("resident_mode", C.c_int32), ("resident_eligible", C.c_int32), ("tail_limit", C.c_int32), ("form", C.c_int32),
                ("launch_grid", C.c_int32), ("launch_block", C.c_int32), ("launch_lds_bytes", C.c_int32), ("launch_image_off", C.c_int32),
                ("launch_phase1", C.c_float), ("launch_lanes", C.c_int32), ("launch_front_back", C.c_int32),
                ("launch_ctrl_lds_off", C.c_int32), ("launch_waves", C.c_int32)]


def plan_step(**query):
    """okenv_debug_plan_step: the library's launch policy for a shape and a call, as a dict (form by name).  No GPU needed."""
    q = OkenvPlanQuery(**dict(OkenvPlanQuery.DEFAULTS, **query))
    r = OkenvPlanResult()
    check(load().okenv_debug_plan_step(C.byref(q), C.byref(r)))
    out = {name: getattr(r, name) for name, _ in r._fields_}
    out["form"] = STEP_FORMS[r.form]
    return out


class OkenvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("okenv error %s (%d): %s" % (ERR_NAMES.get(code, "?"), code, msg))
        self.code = code


_lib = None


def lib_path():
    return _build.LIB_PATH


def load(build_if_missing=True):
    """Loads libokenv.so; raises if it is absent and cannot be built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise OkenvError(-3, "libokenv.so is missing at %s (run python -m openkitchen_amd.buildlib)" % path)
        _build.build()
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 and opens it by path, so
    # if libokenv.so pulled in /opt/rocm's copy first the process would hold two runtimes and whichever
    # initialises second sees "no HIP device".  Importing torch first makes libokenv.so's DT_NEEDED
    # libamdhip64.so.7 resolve (by soname) to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, i32, u32, f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_float
    L.okenv_create.argtypes = [C.POINTER(vp), vp, i32, i32, i32, vp, i32, u32, f32]
    L.okenv_destroy.argtypes = [vp]
    L.okenv_get_info.argtypes = [vp, C.POINTER(OkenvInfo)]
    L.okenv_last_error.argtypes = [vp]
    L.okenv_last_error.restype = C.c_char_p
    L.okenv_set_sensor_offset.argtypes = [vp, f32]
    L.okenv_set_centerline.argtypes = [vp, vp, vp, vp, i32]
    L.okenv_set_stream.argtypes = [vp, vp]
    L.okenv_sync.argtypes = [vp]
    L.okenv_set_field.argtypes = [vp, i32, vp]
    L.okenv_get_field.argtypes = [vp, i32, vp]
    L.okenv_upload_state.argtypes = [vp, vp]
    L.okenv_download_state.argtypes = [vp, vp]
    L.okenv_set_actions.argtypes = [vp, vp, vp]
    L.okenv_reset_agents.argtypes = [vp, vp, vp, vp, vp, i32]
    L.okenv_get_hits.argtypes = [vp, vp]
    L.okenv_get_distances.argtypes = [vp, vp]
    L.okenv_get_flags.argtypes = [vp, vp]
    L.okenv_step.argtypes = [vp, i32]
    L.okenv_collide.argtypes = [vp]
    L.okenv_rollout_random.argtypes = [vp, i32, u32, u32, u32]
    L.okenv_init_bench_state.argtypes = [vp, u32, i32]
    L.okenv_nearest_track_idx.argtypes = [vp, vp, vp, i32, vp]
    L.okenv_set_timing.argtypes = [vp, i32]
    L.okenv_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.okenv_track_load.argtypes = [C.POINTER(vp), C.c_char_p]
    L.okenv_track_free.argtypes = [vp]
    L.okenv_track_num_points.argtypes = [vp]
    L.okenv_track_num_segments.argtypes = [vp]
    L.okenv_track_get.argtypes = [vp, i32, vp]
    L.okenv_track_segments.argtypes = [vp, vp]
    L.okenv_track_queries.argtypes = [vp, vp, vp, i32, vp, vp]
    L.okenv_debug_sincos.argtypes = [i32, vp, vp, vp, i32]
    L.okenv_debug_math.argtypes = [i32, i32, vp, vp, vp, vp, i32]
    L.okenv_debug_adam_device.argtypes = [i32, C.POINTER(OkenvLearnerParams), C.c_int64, vp, vp, vp, vp, i32]
    L.okenv_debug_cast_rays.argtypes = [vp, vp, vp, vp, i32, vp]
    L.okenv_debug_step_forms.argtypes = [vp, vp, i32, i32]
    L.okenv_policy_mlp_create.argtypes = [vp, i32, u32, u32]
    L.okenv_policy_mlp_weights_per_agent.argtypes = [vp]
    L.okenv_policy_mlp_get_weights.argtypes = [vp, vp]
    L.okenv_policy_mlp_set_weights.argtypes = [vp, vp]
    L.okenv_rollout_policy.argtypes = [vp, i32]
    L.okenv_alive_count.argtypes = [vp, C.POINTER(i32)]
    L.okenv_reset_all.argtypes = [vp, f32, f32, f32]
    L.okenv_ga_scores.argtypes = [vp, vp]
    L.okenv_ga_select_mate.argtypes = [vp, u32, u32, u32, vp]
    L.okenv_q_create.argtypes = [vp]
    L.okenv_q_begin_episode.argtypes = [vp, i32]
    L.okenv_rollout_q.argtypes = [vp, i32, f32, u32, u32, u32]
    L.okenv_q_get_table.argtypes = [vp, vp]
    L.okenv_q_set_table.argtypes = [vp, vp]
    L.okenv_q_get_state.argtypes = [vp, vp, vp, vp]
    L.okenv_q_table_sums.argtypes = [vp, vp, vp]
    L.okenv_q_assign_mean.argtypes = [vp, vp, vp]
    L.okenv_q_share_knowledge.argtypes = [vp]
    L.okenv_set_lane_bounds.argtypes = [vp, vp, vp, i32]
    L.okenv_reset_random.argtypes = [vp, vp, i32, u32, u32, u32, u32]
    L.okenv_set_auto_reset.argtypes = [vp, i32, u32, u32, u32]
    L.okenv_get_step_count.argtypes = [vp, C.POINTER(u32)]
    L.okenv_set_step_count.argtypes = [vp, u32]
    L.okenv_step_packed.argtypes = [vp, vp, vp, vp, u32]
    L.okenv_controller_create.argtypes = [vp, C.c_int32]
    L.okenv_controller_num_params.argtypes = [vp, C.POINTER(C.c_int32)]
    L.okenv_controller_set_params.argtypes = [vp, vp]
    L.okenv_controller_act.argtypes = [vp, C.c_float, C.c_float]
    L.okenv_rollout_controller.argtypes = [vp, C.c_int32, C.c_float, C.c_float]
    L.okenv_tracker_create.argtypes = [vp, i32]
    L.okenv_tracker_begin.argtypes = [vp]
    L.okenv_tracker_update.argtypes = [vp]
    L.okenv_field_device_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.okenv_work_stats.argtypes = [vp, vp]
    L.okenv_work_stats_split.argtypes = [vp, vp]
    L.okenv_episode_begin.argtypes = [vp]
    L.okenv_episode_compact.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.okenv_episode_end.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_uint64)]
    L.okenv_episode_tail_limit.argtypes = [vp, C.POINTER(i32)]
    L.okenv_ga_scores_device.argtypes = [vp, C.POINTER(vp)]
    L.okenv_get_stream.argtypes = [vp, C.POINTER(vp)]
    L.okenv_off_grid_count.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.okenv_render_create.argtypes = [vp, vp, vp, vp, vp, i32, C.POINTER(OkenvViewDesc)]
    L.okenv_render_views.argtypes = [vp, vp, C.c_uint64]
    L.okenv_render_get_info.argtypes = [vp, C.POINTER(OkenvRenderInfo)]
    L.okenv_track_band_triangles.argtypes = [vp, vp, vp, i32]
    L.okenv_expert_create.argtypes = [vp, C.POINTER(OkenvExpertParams)]
    L.okenv_expert_act.argtypes = [vp, C.POINTER(OkenvExpertRecord)]
    L.okenv_expert_act_host.argtypes = [C.POINTER(OkenvExpertParams), vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.okenv_debug_atan2f.argtypes = [vp, vp, vp, i32]
    L.okenv_debug_expert_normalize_angle.argtypes = [vp, vp, i32]
    L.okenv_debug_plan_step.argtypes = [C.POINTER(OkenvPlanQuery), C.POINTER(OkenvPlanResult)]
    L.okenv_actor_create.argtypes = [vp, C.POINTER(OkenvActorParams)]
    L.okenv_actor_num_params.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.okenv_actor_set_params.argtypes = [vp, vp, vp]
    L.okenv_actor_set_epsilon.argtypes = [vp, f32]
    L.okenv_actor_set_draw_offset.argtypes = [vp, vp]
    L.okenv_actor_act.argtypes = [vp, C.POINTER(OkenvActorRecord)]
    L.okenv_actor_act_host.argtypes = [C.POINTER(OkenvActorParams), vp, vp, i32, i32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.okenv_debug_expf.argtypes = [vp, vp, i32]
    L.okenv_batch_prepare.argtypes = [vp, C.POINTER(OkenvBatchParams), C.POINTER(OkenvBatchInput), C.POINTER(OkenvBatchOutput)]
    L.okenv_batch_count.argtypes = [vp, C.POINTER(i32)]
    L.okenv_batch_prepare_host.argtypes = [C.POINTER(OkenvBatchParams), C.POINTER(OkenvBatchInput), C.POINTER(OkenvBatchOutput), C.POINTER(i32)]
    L.okenv_debug_batch_timing.argtypes = [vp, vp]
    L.okenv_learner_create.argtypes = [vp, C.POINTER(OkenvLearnerParams)]
    L.okenv_learner_reset.argtypes = [vp]
    L.okenv_ppo_update.argtypes = [vp, C.POINTER(OkenvPpoBatch), i32, i32, i32, vp, C.POINTER(OkenvPpoOutput)]
    L.okenv_ppo_update_host.argtypes = [C.POINTER(OkenvLearnerParams), i32, i32, i32, i32, C.POINTER(OkenvLearnerState), C.POINTER(OkenvPpoBatch),
                                        i32, i32, i32, vp, C.POINTER(OkenvPpoOutput)]
    L.okenv_actor_get_params.argtypes = [vp, vp, vp]
    L.okenv_learner_get_state.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_int64)]
    L.okenv_debug_update_timing.argtypes = [vp, vp]
    L.okenv_debug_adam.argtypes = [C.POINTER(OkenvLearnerParams), C.c_int64, vp, vp, vp, vp, i32]
    L.okenv_replay_create.argtypes = [vp, i32, u32]
    L.okenv_replay_reset.argtypes = [vp]
    L.okenv_replay_push.argtypes = [vp, C.POINTER(OkenvActorRecord), vp]
    L.okenv_replay_size.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.okenv_replay_get.argtypes = [vp, C.POINTER(OkenvReplayRing)]
    L.okenv_dqn_params.argtypes = [vp, C.POINTER(OkenvDqnConfig)]
    L.okenv_dqn_update.argtypes = [vp, i32, i32, i32, u32, C.POINTER(OkenvDqnOutput)]
    L.okenv_dqn_sync_target.argtypes = [vp]
    L.okenv_replay_push_host.argtypes = [C.POINTER(OkenvReplayRing), i32, i32, C.POINTER(C.c_uint64), u32, i32, vp, vp, vp, vp, vp, vp]
    L.okenv_dqn_update_host.argtypes = [C.POINTER(OkenvLearnerParams), C.POINTER(OkenvDqnConfig), i32, i32, i32, C.POINTER(OkenvLearnerState), vp,
                                        C.POINTER(OkenvReplayRing), C.c_int64, i32, i32, i32, u32, C.POINTER(OkenvDqnOutput)]
    L.okenv_debug_dqn_timing.argtypes = [vp, vp]
    L.okenv_ddpg_create.argtypes = [vp, C.POINTER(OkenvDdpgConfig)]
    L.okenv_ddpg_num_params.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.okenv_ddpg_set_params.argtypes = [vp, vp, vp]
    L.okenv_ddpg_get_state.argtypes = [vp, C.POINTER(OkenvDdpgState)]
    L.okenv_ddpg_set_draw_offset.argtypes = [vp, vp]
    L.okenv_ddpg_act.argtypes = [vp, C.POINTER(OkenvDdpgRecord)]
    L.okenv_ddpg_replay_create.argtypes = [vp, i32, u32]
    L.okenv_ddpg_replay_reset.argtypes = [vp]
    L.okenv_ddpg_replay_push.argtypes = [vp, C.POINTER(OkenvDdpgRecord), vp]
    L.okenv_ddpg_replay_size.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.okenv_ddpg_replay_get.argtypes = [vp, C.POINTER(OkenvDdpgRing)]
    L.okenv_ddpg_update.argtypes = [vp, i32, i32, i32, u32, C.POINTER(OkenvDdpgOutput)]
    L.okenv_debug_ddpg_timing.argtypes = [vp, vp]
    L.okenv_ddpg_act_host.argtypes = [C.POINTER(OkenvDdpgConfig), vp, i32, i32, vp, vp, u32, vp, vp, vp, vp, vp]
    L.okenv_ddpg_replay_push_host.argtypes = [C.POINTER(OkenvDdpgRing), i32, i32, C.POINTER(C.c_uint64), u32, i32, vp, vp, vp, vp, vp, vp]
    L.okenv_ddpg_update_host.argtypes = [C.POINTER(OkenvDdpgConfig), i32, C.POINTER(OkenvDdpgState), C.POINTER(OkenvDdpgRing), C.c_int64, i32, i32, i32,
                                         u32, C.POINTER(OkenvDdpgOutput)]
    L.okenv_actor_set_dropout.argtypes = [vp, f32, u32]
    L.okenv_actor_act_dropout_host.argtypes = [C.POINTER(OkenvActorParams), f32, u32, vp, vp, i32, i32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.okenv_reinforce_update.argtypes = [vp, C.POINTER(OkenvReinforceConfig), C.POINTER(OkenvReinforceBatch), i32, i32, vp,
                                         C.POINTER(OkenvReinforceOutput)]
    L.okenv_reinforce_update_host.argtypes = [C.POINTER(OkenvLearnerParams), C.POINTER(OkenvReinforceConfig), f32, u32, u32, i32, i32, i32,
                                              C.POINTER(OkenvLearnerState), C.POINTER(OkenvReinforceBatch), i32, i32, vp,
                                              C.POINTER(OkenvReinforceOutput)]
    L.okenv_debug_reinforce_timing.argtypes = [vp, vp]
    L.okenv_debug_logf.argtypes = [vp, vp, i32]
    L.okenv_debug_reinforce_mask.argtypes = [f32, u32, u32, u32, i32, vp]
    L.okenv_gauss_lds_bytes.argtypes = [i32, i32, i32, i32]
    L.okenv_gauss_lds_bytes.restype = C.c_int64
    L.okenv_gauss_create.argtypes = [vp, C.POINTER(OkenvGaussConfig)]
    L.okenv_gauss_num_params.argtypes = [vp, C.POINTER(i32)]
    L.okenv_gauss_set_params.argtypes = [vp, vp]
    L.okenv_gauss_get_params.argtypes = [vp, vp]
    L.okenv_gauss_get_state.argtypes = [vp, C.POINTER(OkenvGaussState)]
    L.okenv_gauss_set_draw_offset.argtypes = [vp, vp]
    L.okenv_gauss_set_greedy.argtypes = [vp, i32]
    L.okenv_gauss_act.argtypes = [vp, C.POINTER(OkenvGaussRecord)]
    L.okenv_gauss_learner_create.argtypes = [vp, C.POINTER(OkenvLearnerParams)]
    L.okenv_gauss_update.argtypes = [vp, C.POINTER(OkenvGaussUpdateConfig), C.POINTER(OkenvGaussBatch), i32, i32, vp, C.POINTER(OkenvGaussOutput)]
    L.okenv_gauss_act_host.argtypes = [C.POINTER(OkenvGaussConfig), vp, i32, i32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.okenv_gauss_update_host.argtypes = [C.POINTER(OkenvLearnerParams), C.POINTER(OkenvGaussUpdateConfig), i32, i32, i32, i32,
                                          C.POINTER(OkenvGaussState), C.POINTER(OkenvGaussBatch), i32, i32, vp, C.POINTER(OkenvGaussOutput)]
    L.okenv_debug_gauss_timing.argtypes = [vp, vp]
    L.okenv_gcl_lds_bytes.argtypes = [i32, i32, i32, i32, i32]
    L.okenv_gcl_lds_bytes.restype = C.c_int64
    L.okenv_gcl_create.argtypes = [vp, C.POINTER(OkenvGclConfig)]
    L.okenv_gcl_num_params.argtypes = [vp, i32, C.POINTER(i32)]
    L.okenv_gcl_set_params.argtypes = [vp, i32, vp]
    L.okenv_gcl_get_params.argtypes = [vp, i32, vp]
    L.okenv_gcl_get_state.argtypes = [vp, i32, C.POINTER(OkenvGclState)]
    L.okenv_gcl_set_draw_offset.argtypes = [vp, vp]
    L.okenv_gcl_set_greedy.argtypes = [vp, i32]
    L.okenv_gcl_act.argtypes = [vp, C.POINTER(OkenvGclRecord)]
    L.okenv_gcl_set_expert.argtypes = [vp, vp, vp, i32]
    L.okenv_gcl_cost.argtypes = [vp, vp, vp, i32, vp]
    L.okenv_gcl_learner_create.argtypes = [vp, C.POINTER(OkenvLearnerParams), C.POINTER(OkenvLearnerParams)]
    L.okenv_gcl_cost_update.argtypes = [vp, C.POINTER(OkenvGclCostBatch), i32, i32, C.POINTER(OkenvGclCostOutput)]
    L.okenv_gcl_policy_update.argtypes = [vp, C.POINTER(OkenvGclUpdateConfig), C.POINTER(OkenvGclBatch), i32, i32, vp, C.POINTER(OkenvGclOutput)]
    L.okenv_debug_gcl_timing.argtypes = [vp, i32, vp]
    L.okenv_gcl_act_host.argtypes = [C.POINTER(OkenvGclConfig), vp, i32, i32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.okenv_gcl_cost_host.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp]
    L.okenv_gcl_cost_update_host.argtypes = [C.POINTER(OkenvLearnerParams), u32, i32, i32, i32, C.POINTER(OkenvGclState), vp, vp, i32,
                                             C.POINTER(OkenvGclCostBatch), i32, i32, C.POINTER(OkenvGclCostOutput)]
    L.okenv_gcl_policy_update_host.argtypes = [C.POINTER(OkenvLearnerParams), C.POINTER(OkenvGclUpdateConfig), i32, i32, i32, C.POINTER(OkenvGclState),
                                               C.POINTER(OkenvGclState), C.POINTER(OkenvGclBatch), i32, i32, vp, C.POINTER(OkenvGclOutput)]
    L.okenv_debug_normal.argtypes = [i32, vp, vp, vp, vp, i32]
    L.okenv_lidar_lds_bytes.argtypes = [C.POINTER(OkenvLidarConfig)]
    L.okenv_lidar_lds_bytes.restype = C.c_int64
    L.okenv_lidar_create.argtypes = [vp, C.POINTER(OkenvLidarConfig)]
    L.okenv_lidar_num_params.argtypes = [vp, C.POINTER(i32)]
    L.okenv_lidar_set_params.argtypes = [vp, vp]
    L.okenv_lidar_get_params.argtypes = [vp, vp]
    L.okenv_lidar_act.argtypes = [vp, C.POINTER(OkenvLidarRecord)]
    L.okenv_lidar_act_host.argtypes = [C.POINTER(OkenvLidarConfig), vp, i32, vp, vp, vp, vp, vp, vp]
    L.okenv_debug_lidar_linear.argtypes = [i32, i32, i32, i32, vp, vp, vp, i32, vp]
    L.okenv_flow_lds_bytes.argtypes = [C.POINTER(OkenvFlowConfig)]
    L.okenv_flow_lds_bytes.restype = C.c_int64
    L.okenv_flow_create.argtypes = [vp, C.POINTER(OkenvFlowConfig)]
    L.okenv_flow_num_params.argtypes = [vp, C.POINTER(i32)]
    L.okenv_flow_set_params.argtypes = [vp, vp]
    L.okenv_flow_get_params.argtypes = [vp, vp]
    L.okenv_flow_set_draw_offset.argtypes = [vp, vp]
    L.okenv_flow_act.argtypes = [vp, vp, C.POINTER(OkenvFlowRecord)]
    L.okenv_flow_act_host.argtypes = [C.POINTER(OkenvFlowConfig), vp, i32, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.okenv_bev_lds_bytes.argtypes = [C.POINTER(OkenvBevConfig)]
    L.okenv_bev_lds_bytes.restype = C.c_int64
    L.okenv_bev_tiles.argtypes = [C.POINTER(OkenvBevConfig), vp]
    L.okenv_bev_create.argtypes = [vp, C.POINTER(OkenvBevConfig)]
    L.okenv_bev_num_params.argtypes = [vp, C.POINTER(i32)]
    L.okenv_bev_set_params.argtypes = [vp, vp]
    L.okenv_bev_get_params.argtypes = [vp, vp]
    L.okenv_bev_encode.argtypes = [vp, vp, C.c_int64, vp]
    L.okenv_debug_bev_stages.argtypes = [vp, vp, C.c_int64, vp, C.c_uint32]
    L.okenv_bev_encode_host.argtypes = [C.POINTER(OkenvBevConfig), vp, i32, vp, vp]
    L.okenv_cnn_lds_bytes.argtypes = [C.POINTER(OkenvCnnConfig)]
    L.okenv_cnn_lds_bytes.restype = C.c_int64
    L.okenv_cnn_plan.argtypes = [C.POINTER(OkenvCnnConfig), vp]
    L.okenv_cnn_create.argtypes = [vp, C.POINTER(OkenvCnnConfig)]
    L.okenv_cnn_num_params.argtypes = [vp, C.POINTER(i32)]
    L.okenv_cnn_set_params.argtypes = [vp, vp]
    L.okenv_cnn_get_params.argtypes = [vp, vp]
    L.okenv_cnn_act.argtypes = [vp, vp, C.c_int64, C.POINTER(OkenvCnnRecord)]
    L.okenv_debug_cnn_stages.argtypes = [vp, vp, C.c_int64, C.POINTER(OkenvCnnRecord), C.c_uint32]
    L.okenv_cnn_act_host.argtypes = [C.POINTER(OkenvCnnConfig), vp, i32, vp, vp, vp, vp, vp, vp]
    L.okenv_world_lds_bytes.argtypes = [C.POINTER(OkenvWorldConfig)]
    L.okenv_world_lds_bytes.restype = C.c_int64
    L.okenv_world_plan.argtypes = [C.POINTER(OkenvWorldConfig), vp]
    L.okenv_world_workspace_bytes.argtypes = [C.POINTER(OkenvWorldConfig), i32]
    L.okenv_world_workspace_bytes.restype = C.c_int64
    L.okenv_world_create.argtypes = [vp, C.POINTER(OkenvWorldConfig)]
    L.okenv_world_num_params.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.okenv_world_set_params.argtypes = [vp, i32, vp]
    L.okenv_world_get_params.argtypes = [vp, i32, vp]
    L.okenv_world_act.argtypes = [vp, vp, C.c_int64, C.POINTER(OkenvWorldRecord)]
    L.okenv_world_set_lane_widths.argtypes = [vp, vp, vp, i32]
    L.okenv_world_score_begin.argtypes = [vp]
    L.okenv_world_score.argtypes = [vp]
    L.okenv_world_fitness.argtypes = [vp, vp]
    L.okenv_world_fitness_device.argtypes = [vp, C.POINTER(vp)]
    L.okenv_debug_world_stages.argtypes = [vp, vp, C.c_int64, C.POINTER(OkenvWorldRecord), C.c_uint32]
    L.okenv_world_act_host.argtypes = [C.POINTER(OkenvWorldConfig), vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.okenv_world_score_host.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    wc, mc = C.POINTER(OkenvWorldConfig), C.POINTER(OkenvMemoryConfig)
    L.okenv_memory_lds_bytes.argtypes = [wc, mc]
    L.okenv_memory_lds_bytes.restype = C.c_int64
    L.okenv_memory_plan.argtypes = [wc, mc, vp]
    L.okenv_memory_workspace_bytes.argtypes = [wc, mc, i32]
    L.okenv_memory_workspace_bytes.restype = C.c_int64
    L.okenv_memory_create.argtypes = [vp, mc]
    L.okenv_memory_num_params.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.okenv_memory_set_params.argtypes = [vp, i32, vp]
    L.okenv_memory_get_params.argtypes = [vp, i32, vp]
    L.okenv_memory_reset.argtypes = [vp]
    L.okenv_memory_set_hidden.argtypes = [vp, vp]
    L.okenv_memory_get_hidden.argtypes = [vp, vp]
    L.okenv_memory_act.argtypes = [vp, vp, C.c_int64, C.POINTER(OkenvMemoryRecord)]
    L.okenv_debug_memory_stages.argtypes = [vp, vp, C.c_int64, C.POINTER(OkenvMemoryRecord), C.c_uint32]
    L.okenv_memory_act_host.argtypes = [wc, mc, vp, vp, vp, i32, vp, vp, vp, vp, vp, C.POINTER(OkenvMemoryRecord)]
    lc = C.POINTER(OkenvMemoryLearnerConfig)
    L.okenv_memory_learner_workspace_bytes.argtypes = [wc, mc, lc]
    L.okenv_memory_learner_workspace_bytes.restype = C.c_int64
    L.okenv_memory_learner_lds_bytes.argtypes = [wc, mc]
    L.okenv_memory_learner_lds_bytes.restype = C.c_int64
    L.okenv_memory_learner_create.argtypes = [vp, lc]
    L.okenv_memory_learner_reset.argtypes = [vp]
    L.okenv_memory_learner_get_state.argtypes = [vp, C.POINTER(OkenvMemoryLearnerState)]
    L.okenv_memory_update.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, C.POINTER(OkenvMemoryLearnerOutput)]
    L.okenv_memory_eval.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, vp]
    L.okenv_memory_update_host.argtypes = [wc, mc, lc, C.POINTER(OkenvMemoryLearnerState), vp, vp, i32, vp, i32, i32, i32, i32, vp, vp,
                                           C.POINTER(OkenvMemoryLearnerOutput)]
    L.okenv_memory_eval_host.argtypes = [wc, mc, lc, vp, vp, vp, i32, vp, i32, i32, i32, vp]
    L.okenv_memory_window_host.argtypes = [wc, mc, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    qc, i64 = C.POINTER(OkenvQcnnConfig), C.c_int64
    L.okenv_qcnn_lds_bytes.argtypes = [qc]
    L.okenv_qcnn_lds_bytes.restype = C.c_int64
    L.okenv_qcnn_plan.argtypes = [qc, vp]
    L.okenv_qcnn_create.argtypes = [vp, qc]
    L.okenv_qcnn_num_params.argtypes = [vp, C.POINTER(i32)]
    L.okenv_qcnn_set_params.argtypes = [vp, vp]
    L.okenv_qcnn_get_params.argtypes = [vp, vp]
    L.okenv_qcnn_set_epsilon.argtypes = [vp, C.c_float]
    L.okenv_qcnn_set_draw_offset.argtypes = [vp, vp]
    L.okenv_qcnn_act.argtypes = [vp, vp, i64, C.POINTER(OkenvQcnnRecord)]
    L.okenv_debug_qcnn_stages.argtypes = [vp, vp, i64, C.POINTER(OkenvQcnnRecord), C.c_uint32]
    L.okenv_qcnn_ring_create.argtypes = [vp, i32, C.c_uint32]
    L.okenv_qcnn_ring_reset.argtypes = [vp]
    L.okenv_qcnn_ring_size.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.okenv_qcnn_ring_get.argtypes = [vp, C.POINTER(OkenvQcnnRing)]
    L.okenv_qcnn_push.argtypes = [vp, C.POINTER(OkenvQcnnRecord), vp, vp, i64, vp]
    L.okenv_qcnn_batch.argtypes = [vp, i32, i32, i64, C.POINTER(OkenvQcnnBatchOut)]
    L.okenv_qcnn_act_host.argtypes = [qc, vp, i32, vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.okenv_qcnn_push_host.argtypes = [C.POINTER(OkenvQcnnRing), i32, i32, C.POINTER(C.c_uint64), C.c_uint32, i32, vp, vp, vp, vp, vp, vp, vp, i32]
    L.okenv_qcnn_batch_host.argtypes = [C.POINTER(OkenvQcnnRing), i32, i32, C.c_uint64, C.c_uint32, i32, i32, i64, C.POINTER(OkenvQcnnBatchOut)]
    L.okenv_debug_qcnn_grey_host.argtypes = [i32, i32, vp, vp]
    L.okenv_debug_qcnn_forward_planes_host.argtypes = [qc, vp, i32, vp, vp]
    L.okenv_vit_lds_bytes.argtypes = [C.POINTER(OkenvVitConfig)]
    L.okenv_vit_lds_bytes.restype = C.c_int64
    L.okenv_vit_create.argtypes = [vp, C.POINTER(OkenvVitConfig)]
    L.okenv_vit_num_params.argtypes = [vp, C.POINTER(i32)]
    L.okenv_vit_set_params.argtypes = [vp, vp]
    L.okenv_vit_get_params.argtypes = [vp, vp]
    L.okenv_vit_act.argtypes = [vp, vp, i64, C.POINTER(OkenvVitRecord)]
    L.okenv_vit_act_host.argtypes = [C.POINTER(OkenvVitConfig), vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.okenv_debug_vit_attend.argtypes = [i32, i32, i32, i32, i32, vp, vp]
    L.okenv_vit_embed.argtypes = [vp, vp, i32, i64, vp]
    L.okenv_vit_head_lds_bytes.argtypes = [i32, i32, i32]
    L.okenv_vit_head_lds_bytes.restype = C.c_int64
    L.okenv_vit_head_learner_create.argtypes = [vp, C.POINTER(OkenvVitHeadParams)]
    L.okenv_vit_head_learner_reset.argtypes = [vp]
    L.okenv_vit_head_learner_get_state.argtypes = [vp, C.POINTER(OkenvVitHeadState)]
    L.okenv_vit_head_update.argtypes = [vp, vp, vp, i32, i32, i32, vp, C.POINTER(OkenvVitHeadOutput)]
    L.okenv_vit_head_eval.argtypes = [vp, vp, vp, i32, i32, vp]
    L.okenv_vit_head_update_host.argtypes = [C.POINTER(OkenvVitHeadParams), i32, i32, i32, C.c_float, C.POINTER(OkenvVitHeadState), vp, vp, i32, i32, i32, vp,
                                             C.POINTER(OkenvVitHeadOutput)]
    L.okenv_vit_head_eval_host.argtypes = [C.POINTER(OkenvVitHeadParams), i32, i32, i32, C.c_float, vp, vp, vp, i32, i32, vp]
    _lib = L
    return L


def check(rc, handle=None):
    if rc != OKENV_OK:
        msg = load().okenv_last_error(handle)
        raise OkenvError(rc, msg.decode() if msg else "")
    return rc


def ptr(a):
    """Raw pointer of a numpy array, a torch tensor (host or device) or an int address."""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):  # torch tensor
        assert a.is_contiguous()
        return C.c_void_p(a.data_ptr())
    raise TypeError("unsupported buffer type %r" % type(a))
