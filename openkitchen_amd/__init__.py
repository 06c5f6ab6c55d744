"""openkitchen_amd -- MI355X-native batched implementation of OpenKitchen's Environment step path.

The product is libokenv.so (hand-written HIP kernels for gfx950 behind the C ABI of include/okenv.h, plus
the C++ Environment/Agent/CollisionChecker facade of include/Environment/).  This package is the Python
host side: it builds and loads that library and exposes typed wrappers.  Nothing here computes on the CPU
in its place.
"""
from . import _capi as capi  # noqa: F401
from .buildlib import build  # noqa: F401
from .env import (BatchedEnvironment, Track, actor_act_host, actor_act_dropout_host, reinforce_update_host, debug_logf, debug_reinforce_mask, ddpg_act_host, ddpg_replay_push_host, ddpg_ring, ddpg_update_host, batch_prepare_host, ppo_update_host, debug_adam, debug_atan2f, debug_expert_normalize_angle, debug_expf,  # noqa: F401
                  debug_sincos, debug_math, debug_adam_device, default_ray_fan, dqn_update_host, expert_act_host, replay_push_host, replay_ring, track_path,
                  debug_normal, gauss_act_host, gauss_update_host, gcl_act_host, gcl_cost_host, gcl_cost_update_host, gcl_policy_update_host)

__all__ = ["BatchedEnvironment", "Track", "actor_act_host", "actor_act_dropout_host", "reinforce_update_host", "debug_logf", "debug_reinforce_mask", "ddpg_act_host", "ddpg_replay_push_host", "ddpg_ring", "ddpg_update_host", "batch_prepare_host", "ppo_update_host", "build", "capi", "debug_adam", "debug_atan2f", "debug_expert_normalize_angle", "debug_expf",
           "debug_sincos", "debug_math", "debug_adam_device",
           "default_ray_fan", "dqn_update_host", "expert_act_host", "replay_push_host", "replay_ring", "track_path",
           "debug_normal", "gauss_act_host", "gauss_update_host", "gcl_act_host", "gcl_cost_host", "gcl_cost_update_host",
           "gcl_policy_update_host"]
