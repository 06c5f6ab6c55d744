"""The step-form table: one row per step-kernel launch of openkitchen_amd/csrc/okenv_capi.hip (launchStep's switch over enum
okenv_step_form of include/okenv.h), plus rows for the variants of a site (front / back images on and off, episode list or none, controller
parameters in LDS or in global memory) and for a handle with several policies attached.  Plain data: tests/test_step_form_table.py
imports it without a GPU, tests/test_gpu_step_forms.py runs every row against the oracle.

A row's population is given relative to the device's compute units C (okenv_info.compute_units) so that it forces its form in any
partition mode of an MI355X (SPX 256 CUs, DPX 128, CPX 32): n = (k, b) means N = k * C + b.

Row keys:
  id      the test id
  form    the form the row is written for; it must run
  forms   every form the row may run (anything else that runs fails the row)
  track, n, R (rays of the default fan), flags (okenv_create), env (OKENV_* knobs set before create)
  driver  the call sequence (tests/test_gpu_step_forms.py: DRIVERS)
  attrs   {attribute: "all" | "some" | "none"} over the launches of `form`
"""

FORMS = ["tail_q", "tail_mlp32", "tail_mlp15", "tail_mlp", "coop_q", "coop_ctrl", "coop_mlp32", "coop_mlp", "coop_packed_direct",
         "coop_packed", "coop_direct", "coop_g64_random", "coop_g64", "coop", "resident_direct", "resident", "lds", "lds_mlp", "global",
         "global_mlp", "brute", "brute_mlp"]

# the kernel each form launches (as the launch site spells it, spaces removed)
KERNELS = {
    "tail_q": "okStepTailKernel<kPolicyQ,0>", "tail_mlp32": "okStepTailKernel<kPolicyMlp,32>",
    "tail_mlp15": "okStepTailKernel<kPolicyMlp,15>", "tail_mlp": "okStepTailKernel<kPolicyMlp,0>",
    "coop_q": "okStepCoopKernel<kPolicyQ>", "coop_ctrl": "okStepCoopKernel<kPolicyCtrl>",
    "coop_mlp32": "okStepCoopKernel<kPolicyMlp,false,false,false,32>", "coop_mlp": "okStepCoopKernel<kPolicyMlp>",
    "coop_packed_direct": "okStepCoopKernel<kPolicyNone,true,false,true>", "coop_packed": "okStepCoopKernel<kPolicyNone,true>",
    "coop_direct": "okStepCoopKernel<kPolicyNone,false,false,true>",
    "coop_g64_random": "okStepCoopKernel<kPolicyNone,false,false,false,64,true>",
    "coop_g64": "okStepCoopKernel<kPolicyNone,false,false,false,64>", "coop": "okStepCoopKernel<kPolicyNone>",
    "resident_direct": "okStepCoopKernel<kPolicyNone,true,true,true>", "resident": "okStepCoopKernel<kPolicyNone,true,true>",
    "lds": "okStepKernel<kGridLds,kPolicyNone>", "lds_mlp": "okStepKernel<kGridLds,kPolicyMlp>",
    "global": "okStepKernel<kGridGlobal,kPolicyNone>", "global_mlp": "okStepKernel<kGridGlobal,kPolicyMlp>",
    "brute": "okStepKernel<kGridBrute,kPolicyNone>", "brute_mlp": "okStepKernel<kGridBrute,kPolicyMlp>",
}

NO_TAIL = {"OKENV_TAIL_MAX_AGENTS": "0"}
NO_FB = {"OKENV_FRONT_BACK": "0"}


def _row(id, form, driver, track, n, R, forms=None, env=None, flags=0, attrs=None, **kw):
    r = dict(id=id, form=form, forms=sorted(forms or {form}), driver=driver, track=track, n=n, R=R, env=dict(env or {}), flags=flags,
             attrs=dict(attrs or {}))
    r.update(kw)
    return r


ROWS = [
    # ---- tail forms: episode lists short enough for one agent per workgroup (N <= C: one round of workgroups on any device)
    _row("tail_q", "tail_q", "q_episode", "Silverstone", (0, 24), 16, attrs={"list": "all"}),
    _row("tail_mlp32", "tail_mlp32", "ga_episode", "Monza", (0, 24), 32, attrs={"list": "all", "front_back": "all"}),
    _row("tail_mlp32_combined_image", "tail_mlp32", "ga_episode", "Monza", (0, 24), 32, env=NO_FB, attrs={"list": "all", "front_back": "none"}),
    _row("tail_mlp15", "tail_mlp15", "ga_episode", "Austin", (0, 24), 15, attrs={"list": "all"}),
    _row("tail_mlp", "tail_mlp", "ga_episode", "Spa", (0, 23), 9, attrs={"list": "all"}),
    # ---- cooperative forms
    _row("coop_q_episode", "coop_q", "q_episode", "Austin", (0, 48), 5, env=NO_TAIL, attrs={"list": "some"}),
    _row("coop_q_plain", "coop_q", "q_plain", "Silverstone", (0, 40), 16, attrs={"list": "none", "front_back": "all"}),
    _row("coop_q_plain_combined_image", "coop_q", "q_plain", "Silverstone", (0, 40), 16, env=NO_FB, attrs={"list": "none", "front_back": "none"}),
    # a list launched with wider lane groups than the handle's (the handle's groups forced narrow; N * 2 * 32 <= 512 * C)
    _row("coop_q_widened", "coop_q", "q_episode", "Silverstone", (2, 37), 16, env=dict(NO_TAIL, OKENV_LANES_PER_AGENT="16"),
         attrs={"list": "some", "widened": "some"}),
    _row("coop_ctrl_lds", "coop_ctrl", "ctrl", "Silverstone", (0, 300), 5, hidden=16, attrs={"ctrl_lds": "all", "list": "none"}),
    _row("coop_ctrl_global", "coop_ctrl", "ctrl", "Spa", (0, 40), 64, hidden=64, attrs={"ctrl_lds": "none", "list": "none"}),
    _row("coop_ctrl_episode", "coop_ctrl", "ctrl_episode", "Austin", (0, 96), 5, hidden=16, attrs={"list": "some"}),
    # 32 rays in the handle's natural 32-lane groups: N * 2 * 32 > 512 * C (a window of the population against the oracle)
    _row("coop_mlp32", "coop_mlp32", "ga_window", "Monza", (8, 40), 32, attrs={"list": "none"}),
    _row("coop_mlp32_episode", "coop_mlp32", "ga_episode", "Monza", (0, 96), 32, env=dict(NO_TAIL, OKENV_LANES_PER_AGENT="32"),
         attrs={"list": "some"}),
    _row("coop_mlp_episode", "coop_mlp", "ga_episode", "Austin", (0, 64), 16, env=NO_TAIL, attrs={"list": "some"}),
    _row("coop_mlp_plain", "coop_mlp", "ga_plain", "Silverstone", (0, 33), 15, attrs={"list": "none"}),
    _row("coop_packed_direct", "coop_packed_direct", "packed", "Austin", (0, 15), 5, env={"OKENV_RESIDENT": "0"},
         attrs={"agents_per_block": "all"}),
    _row("coop_packed", "coop_packed", "packed", "Silverstone", (0, 20), 64, env={"OKENV_RESIDENT": "0"}),
    _row("coop_direct", "coop_direct", "step", "Austin", (0, 48), 16, attrs={"front_back": "all"}),
    _row("coop_direct_combined_image", "coop_direct", "step", "Austin", (0, 48), 16, env=NO_FB, attrs={"front_back": "none"}),
    _row("coop_direct_one_agent_per_workgroup", "coop_direct", "step", "Monza", (0, 15), 5, attrs={"agents_per_block": "all"}),
    _row("coop_g64_random", "coop_g64_random", "random", "Silverstone", (0, 96), 64, attrs={"front_back": "all"}),
    _row("coop_g64_random_combined_image", "coop_g64_random", "random", "Silverstone", (0, 96), 64, env=NO_FB, attrs={"front_back": "none"}),
    # the headline instantiation with every CU's waves full: a window of the population against the oracle
    _row("coop_g64_random_full", "coop_g64_random", "random_window", "Silverstone", (16, 0), 64, attrs={"front_back": "all"}),
    _row("coop_g64_random_small_workgroups", "coop_g64_random", "random", "Spa", (0, 70), 64, env={"OKENV_BLOCK_THREADS": "128"}),
    _row("coop_g64", "coop_g64", "step", "Silverstone", (0, 40), 64),
    _row("coop_g64_two_agents_per_workgroup", "coop_g64", "step", "Spa", (0, 30), 64, env={"OKENV_AGENTS_PER_BLOCK": "2"},
         attrs={"agents_per_block": "all"}),
    # 32-lane groups with phase 1: N * 2 * 32 > 512 * C, a ragged last workgroup (a window against the oracle)
    _row("coop", "coop", "random_window", "Monza", (8, 37), 32),
    _row("coop_lanes_knob", "coop", "step", "Austin", (0, 40), 20, env={"OKENV_LANES_PER_AGENT": "32"}),
    _row("coop_phase1_knob", "coop", "step", "Spa", (0, 40), 24, env={"OKENV_LANES_PER_AGENT": "32", "OKENV_PHASE1_RANGE": "20"}),
    # ---- resident forms (a hand-over nobody answers in time is redone by a packed launch: those forms may run too)
    _row("resident_direct", "resident_direct", "resident", "Austin", (0, 15), 5, forms={"resident_direct", "coop_packed_direct"},
         env={"OKENV_RESIDENT": "1"}),
    _row("resident", "resident", "resident", "Silverstone", (0, 20), 64, forms={"resident", "coop_packed"}, env={"OKENV_RESIDENT": "1"}),
    # ---- generic forms: every lane walks its own rays
    _row("lds_no_coop", "lds", "step", "Austin", (0, 32), 16, env={"OKENV_COOP": "0"}),
    _row("lds_wide_fan", "lds", "step", "Silverstone", (0, 12), 100),
    _row("lds_mlp", "lds_mlp", "ga_episode", "Austin", (0, 48), 15, env={"OKENV_COOP": "0"}, attrs={"list": "some"}),
    _row("global", "global", "step", "Silverstone", (0, 32), 16, flags=1),
    _row("global_mlp", "global_mlp", "ga_episode", "Austin", (0, 48), 15, flags=1, attrs={"list": "some"}),
    _row("brute", "brute", "step", "Monza", (0, 24), 16, flags=2),
    _row("brute_mlp", "brute_mlp", "ga_episode", "Monza", (0, 20), 8, flags=2, attrs={"list": "some"}),
]

# A handle with the MLP, Q-learning and controller policies all attached, running each kind of episode: it must run the same
# forms, list and tail limit as the single-policy handle of the same shape (the row named by `like`), and equal the oracle.
MULTI_ROWS = [
    dict(id="multi_mlp_episode", like="tail_mlp15", kind="mlp"),
    dict(id="multi_q_episode", like="tail_q", kind="q"),
    dict(id="multi_ctrl_episode", like="coop_ctrl_episode", kind="ctrl"),
]


def population(row, C):
    k, b = row["n"]
    return k * C + b


def pow2ceil(v):
    p = 1
    while p < v:
        p *= 2
    return p


def handle_shape(N, R, C, env=None, flags=0):
    """A handle's launch shape (openkitchen_amd/csrc/okenv_capi.hip): okPlanLanes' lanes per agent G and phase 1, okPlanGeometry's
    grid form (assuming the track image fits the LDS, as the four tracks' do at the default cell), workgroup size, cooperative
    kernel and agents per workgroup.  env: the OKENV_* knobs as readKnobs finds them."""
    env = env or {}
    G = min(64, pow2ceil(R))
    natural = G
    while G < 64 and N * 2 * G <= 512 * C:
        G *= 2
    g = int(env.get("OKENV_LANES_PER_AGENT", 0))
    if 1 <= g <= 64 and g & (g - 1) == 0:
        G = g
    phase1 = 0.0 if G > natural else 48.0
    rays_per_lane = (R + G - 1) // G
    if G == 16 and rays_per_lane == 1:
        phase1 = 32.0
    if "OKENV_PHASE1_RANGE" in env and float(env["OKENV_PHASE1_RANGE"]) >= 0:
        phase1 = float(env["OKENV_PHASE1_RANGE"])
    grid = "brute" if flags & 2 else ("global" if flags & 1 else "lds")
    per_block = ((N * G + C - 1) // C + 63) // 64 * 64
    per_block = min(max(per_block, 256), 1024)
    bt = int(env.get("OKENV_BLOCK_THREADS", 0))
    if 64 <= bt <= 1024 and bt % 64 == 0 and bt % G == 0:
        per_block = bt
    coop = grid == "lds" and rays_per_lane == 1 and int(env.get("OKENV_COOP", 1)) != 0
    apb = 1 if coop and G == 64 and N <= C and per_block == 256 else 0
    if "OKENV_AGENTS_PER_BLOCK" in env and coop and 0 <= int(env["OKENV_AGENTS_PER_BLOCK"]) and int(env["OKENV_AGENTS_PER_BLOCK"]) * G <= per_block:
        apb = int(env["OKENV_AGENTS_PER_BLOCK"])
    return dict(N=N, R=R, C=C, G=G, phase1=phase1, rays_per_lane=rays_per_lane, grid=grid, coop=coop, block_threads=per_block,
                agents_per_block=apb, tail_max=int(env.get("OKENV_TAIL_MAX_AGENTS", -1)),
                resident_mode=int(env.get("OKENV_RESIDENT", -1)))


def tail_limit(shape, fit):
    """okTailLimit (okenv_capi.hip) for a track image of which `fit` tail workgroups share a CU's LDS (1 or 2 for the four
    tracks; the exact figure needs the image, which only okenv_create builds): 0 without the cooperative kernel."""
    if shape["grid"] != "lds" or not shape["coop"] or shape["tail_max"] == 0:
        return 0
    if ((shape["R"] * 8 + 63) // 64) * 64 > 512:
        return 0
    lim = fit * shape["C"]
    return min(shape["tail_max"], lim) if shape["tail_max"] > 0 else lim


def first_form(shape, call, fit):
    """The form of a call's first step launch (okPlanStep of okenv_capi.hip; okResidentShape and okenv_step_packed for the choice of
    the resident kernel).  call: step, random, packed, resident, ga_plain, ga_episode, q_plain, q_episode,
    ctrl, ctrl_episode.  An episode's first launch is listed when the population fits the tail kernel (okPrelist)."""
    mlp = call.startswith("ga")
    episode = call.endswith("episode")
    if shape["grid"] != "lds" or not shape["coop"]:
        name = {"lds": "lds", "global": "global", "brute": "brute"}[shape["grid"]]
        return name + "_mlp" if mlp else name
    direct = shape["phase1"] <= 0 and shape["G"] >= 2 * shape["R"]
    if episode and call != "ctrl_episode" and shape["N"] <= tail_limit(shape, fit):
        if call == "q_episode":
            return "tail_q"
        return {32: "tail_mlp32", 15: "tail_mlp15"}.get(shape["R"], "tail_mlp")
    if call.startswith("q"):
        return "coop_q"
    if call.startswith("ctrl"):
        return "coop_ctrl"
    if mlp:
        return "coop_mlp32" if shape["G"] == 32 and shape["R"] == 32 else "coop_mlp"
    if call == "resident":
        assert shape["agents_per_block"] == 1 and shape["N"] <= 64 and shape["resident_mode"] != 0
        return "resident_direct" if direct else "resident"
    if call == "packed":
        return "coop_packed_direct" if direct else "coop_packed"
    if direct:
        return "coop_direct"
    if shape["G"] == 64 and call == "random":
        return "coop_g64_random"
    if shape["G"] == 64:
        return "coop_g64"
    return "coop"


DRIVER_CALL = {"q_episode": "q_episode", "q_plain": "q_plain", "ga_episode": "ga_episode", "ga_plain": "ga_plain", "ga_window": "ga_plain",
               "ctrl": "ctrl", "ctrl_episode": "ctrl_episode", "packed": "packed", "resident": "resident", "step": "step",
               "random": "random", "random_window": "random"}
