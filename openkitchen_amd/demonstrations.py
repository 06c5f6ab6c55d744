"""Batched demonstration recording: the loop of the reference's data collector for N agents at once.

FieldNavigators/collect_data/collect_data_random.cpp:160-186 drives ONE agent behind a window: resetAgent with the chosen
randomisation, one Environment::step for the initial observation, then per step { goal point, updateAction, saveMeasurement,
Environment::step }.  `collect_demonstrations` runs the same loop for every agent of a VectorEnvironment with the expert on the
device (okenv_expert_act writes the action AND the step's record slots, so no copy kernel runs), and returns the samples as
`[T, N, ...]` device tensors; openkitchen_amd/dataset.py turns them into the reference's two file formats.

What is not carried over: the reference ends an agent's trajectory after kTrajLength goal points or when it overshoots, and
re-places it (:177-183); here every agent runs for `steps` steps, crashed agents are re-placed by the environment's auto-reset
if it is on, and `alive` tells which samples the reference's `while (... && !agent->crashed_)` would have recorded.
"""
import torch

from . import _capi as capi


def collect_demonstrations(venv, steps, images=False, reset_flags=capi.RESET_RANDOM_POINT | capi.RESET_RANDOM_LANE | capi.RESET_RANDOM_HEADING,
                           seed=0, epoch=0):
    """Records `steps` steps of the expert attached to `venv` (VectorEnvironment.enable_expert; enable_camera too when
    `images`).  Returns a dict of device tensors: actions [T,N,2], dist [T,N,R], rel_xy [T,N,R,2] (float32), alive [T,N]
    (uint8, !crashed_) and, with images, frames [T,N,H,W,4] or [T,N,H,W] (uint8).  Slot t holds the observation (and the
    frame of the state) the action of slot t was computed from: the reference saves before env.step().  Nothing here
    synchronises; the tensors are valid in stream order."""
    T, N, R, dev = int(steps), venv.num_envs, venv.num_rays, venv.device
    if T <= 0:
        raise ValueError("steps must be positive")
    if not hasattr(venv, "expert_params"):
        raise capi.OkenvError(-5, "collect_demonstrations: call enable_expert first")
    if images and not hasattr(venv, "camera_shape"):
        raise capi.OkenvError(-5, "collect_demonstrations: images need enable_camera first")
    with torch.cuda.device(dev):
        out = {"actions": torch.empty((T, N, 2), dtype=torch.float32, device=dev),
               "dist": torch.empty((T, N, R), dtype=torch.float32, device=dev),
               "rel_xy": torch.empty((T, N, R, 2), dtype=torch.float32, device=dev),
               "alive": torch.empty((T, N), dtype=torch.uint8, device=dev)}
        if images:
            out["frames"] = torch.empty((T,) + tuple(venv.camera_shape), dtype=torch.uint8, device=dev)
        # env.resetAgent(agent, kResetAgentsRandomly, kRandomizeLaneOnReset, kRandomizeHeadingOnReset); env.step()  (:163,172)
        venv.env.reset_random(None, int(reset_flags), int(seed), int(epoch), venv.agent_base)
        venv.env.step(1)
        for t in range(T):
            venv.env.expert_act({"action": out["actions"][t], "dist": out["dist"][t], "rel_xy": out["rel_xy"][t], "alive": out["alive"][t]})
            if images:
                venv.camera(out=out["frames"][t])
            venv.env.step(1)
    return out
