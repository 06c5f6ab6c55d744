"""The step-form table (tests/_step_forms.py) stays complete: every hipLaunchKernelGGL of a step kernel in okenv_capi.hip sits
under the case label of one form of enum okenv_step_form, the enum, the Python names and the GPU rows agree one to one, and every
row's shape implies its form under the launcher's rules for a device of 32, 128 or 256 compute units (the partition modes of an
MI355X) -- asked of the library's own launch policy (okenv_debug_plan_step: okPlanLanes, okPlanGeometry, okPlanStep of okenv_capi.hip
run on the host) and of its independent restatement in tests/_step_forms.py.  No GPU needed."""
import os
import re

import pytest

import _step_forms as T
from openkitchen_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "openkitchen_amd", "csrc", "okenv_capi.hip")
HDR = os.path.join(ROOT, "include", "okenv.h")

LAUNCH = re.compile(r"hipLaunchKernelGGL\(\s*\(?\s*(okStep\w*Kernel(?:<[^>]*>)?)\s*\)?\s*,")
CASE = re.compile(r"case\s+OKENV_FORM_(\w+):\s*$")


def launch_sites(src):
    """[(form or None, kernel)] for every step-kernel launch: the form of the `case OKENV_FORM_...:` label right before it (only
    blanks and comments between them) in launchStep's switch over the plan's form -- which countForm has counted just before the
    switch --, None when there is none."""
    src = re.sub(r"//[^\n]*", "", src)
    sites = []
    for m in LAUNCH.finditer(src):
        c = CASE.search(src[:m.start()].rstrip())
        sites.append((c.group(1).lower() if c else None, re.sub(r"\s+", "", m.group(1))))
    return sites


def enum_forms(hdr):
    body = re.search(r"enum okenv_step_form\s*\{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n[len("OKENV_FORM_"):].lower() for n in re.findall(r"\b(OKENV_FORM_\w+)", body)]


def test_every_step_launch_is_counted_once_as_its_form():
    src = open(SRC).read()
    sites = launch_sites(src)
    assert len(sites) == 22
    uncounted = [k for f, k in sites if f is None]
    assert not uncounted, "step-kernel launches without a form's case label in front of them: %s" % uncounted
    assert len(re.findall(r"\bcountForm\(h, plan\.form, p\);", src)) == 1, "the plan's form is counted once, before the switch"
    forms = [f for f, _ in sites]
    assert sorted(forms) == sorted(T.FORMS), "each form is counted at exactly one launch site"
    for f, k in sites:
        assert T.KERNELS[f] == k, "OKENV_FORM_%s counts a launch of %s" % (f.upper(), k)


def test_an_uncounted_launch_fails_the_check():
    """what the check above catches: a copy of the source with one more, uncounted instantiation"""
    src = open(SRC).read()
    at = src.index("    OK_HIP(h, hipGetLastError());\n    return endTiming(h, ev);")
    bad = src[:at] + "    hipLaunchKernelGGL((okStepCoopKernel<kPolicyNone, true, true, false, 32>), grid, block, lds, h->stream, p, off, 0.F);\n" + src[at:]
    sites = launch_sites(bad)
    assert len(sites) == 23 and [k for f, k in sites if f is None] == ["okStepCoopKernel<kPolicyNone,true,true,false,32>"]


def test_enum_python_names_and_table_agree():
    assert enum_forms(open(HDR).read()) == capi.STEP_FORMS == T.FORMS
    assert sorted(T.KERNELS) == sorted(T.FORMS)
    attrs = re.search(r"enum okenv_step_form_attr\s*\{(.*?)\};", open(HDR).read(), re.S).group(1)
    attrs = re.sub(r"/\*.*?\*/", "", attrs, flags=re.S)
    assert [a[len("OKENV_FORM_ATTR_"):].lower() for a in re.findall(r"\b(OKENV_FORM_ATTR_\w+)", attrs)] == capi.STEP_FORM_ATTRS


def test_every_form_has_a_row():
    assert {r["form"] for r in T.ROWS} == set(T.FORMS)
    ids = [r["id"] for r in T.ROWS] + [r["id"] for r in T.MULTI_ROWS]
    assert len(ids) == len(set(ids))
    for r in T.ROWS:
        assert r["form"] in r["forms"] and set(r["forms"]) <= set(T.FORMS), r["id"]
        assert r["driver"] in T.DRIVER_CALL, r["id"]
        assert set(r["attrs"]) <= set(capi.STEP_FORM_ATTRS) and set(r["attrs"].values()) <= {"all", "some", "none"}, r["id"]
        assert all(k.startswith("OKENV_") for k in r["env"]), r["id"]
    for m in T.MULTI_ROWS:
        assert m["like"] in ids and m["kind"] in ("mlp", "q", "ctrl")
    assert {m["kind"] for m in T.MULTI_ROWS} == {"mlp", "q", "ctrl"}


@pytest.mark.parametrize("C", [32, 128, 256])
def test_row_shapes_imply_their_forms_in_every_partition_mode(C):
    """The launch policy, restated (tests/_step_forms.py: handle_shape, tail_limit, first_form) and real (okenv_debug_plan_step): each
    row's population, fan and knobs pick its form whatever the device's CU count, and whether one or two tail workgroups share a
    CU."""
    for r in T.ROWS:
        N = T.population(r, C)
        shape = T.handle_shape(N, r["R"], C, r["env"], r["flags"])
        for fit in (1, 2):
            call = T.DRIVER_CALL[r["driver"]]
            got = T.first_form(shape, call, fit)
            assert got == r["form"], (r["id"], C, fit, got, shape)
            real = plan(N, r["R"], C, r["env"], r["flags"], call, fit)
            assert real["form"] == r["form"], (r["id"], C, fit, real)
            assert real["tail_limit"] in (0, fit * C) or r["env"].get("OKENV_TAIL_MAX_AGENTS"), (r["id"], C, fit, real)


# Track-image sizes of which one / two tail workgroups fit a CU's 160 KiB of LDS, with or without the Q-learning kernel's centre
# line (Q_BYTES) and table behind them; the front / back images a little larger than the combined one, as the four tracks' are.
IMAGE_BYTES = {1: 100000, 2: 60000}
Q_BYTES = 12000
# how each driver call of tests/_step_forms.py reaches the launcher: the action source (OkActionSource of okenv_kernels.h) and what
# else the call says
CALLS = {"step": dict(action_source=0), "random": dict(action_source=1), "packed": dict(action_source=0, packed=1),
         "resident": dict(action_source=0, packed=1, resident_launch=1),
         "ga_plain": dict(action_source=2), "ga_episode": dict(action_source=2, n_listed=capi.PLAN_FIRST_ROLLOUT),
         "q_plain": dict(action_source=3), "q_episode": dict(action_source=3, n_listed=capi.PLAN_FIRST_ROLLOUT),
         "ctrl": dict(action_source=4, ctrl_num_params=117), "ctrl_episode": dict(action_source=4, ctrl_num_params=117,
                                                                                  n_listed=capi.PLAN_FIRST_ROLLOUT)}
KNOBS = {"OKENV_LANES_PER_AGENT": "lanes_per_agent", "OKENV_BLOCK_THREADS": "block_threads", "OKENV_COOP": "coop",
         "OKENV_AGENTS_PER_BLOCK": "agents_per_block", "OKENV_TAIL_MAX_AGENTS": "tail_max_agents", "OKENV_RESIDENT": "resident",
         "OKENV_FRONT_BACK": "front_back"}


def plan(N, R, C, env, flags, call, fit):
    """The library's own answer for a handle of this shape (knobs as the OKENV_* strings of a row) and this driver call."""
    knobs = {KNOBS[k]: int(v) for k, v in env.items() if k in KNOBS}
    if "OKENV_PHASE1_RANGE" in env:
        knobs["phase1_range"] = float(env["OKENV_PHASE1_RANGE"])
    assert set(env) <= set(KNOBS) | {"OKENV_PHASE1_RANGE"}
    return capi.plan_step(num_agents=N, num_rays=R, compute_units=C, flags=flags, image_bytes=IMAGE_BYTES[fit],
                          front_back_bytes=IMAGE_BYTES[fit] + 6000, q_bytes=Q_BYTES, **dict(knobs, **CALLS[call]))


def sweep_populations(C):
    ns = {1, 2, 15, 50, 64, 65, C - 1, C, C + 1, 2 * C, 2 * C + 37, 4 * C, 4 * C + 1, 8 * C, 8 * C + 37, 16 * C, 16 * C + 1, 17 * C + 5}
    for G in (1, 2, 4, 8, 16, 32, 64):  # where the lane groups stop widening: N * 2G <= 512 * C
        ns |= {256 * C // G, 256 * C // G + 1}
    return sorted(ns)


# every knob unset, then one at a time at a value the library takes and at one it ignores (a switch has no ignored value: both of its)
KNOB_SETTINGS = [{}] + [{k: v} for k, vs in {
    "OKENV_LANES_PER_AGENT": ("16", "3"), "OKENV_BLOCK_THREADS": ("128", "100"), "OKENV_COOP": ("0", "1"),
    "OKENV_AGENTS_PER_BLOCK": ("2", "-1"), "OKENV_TAIL_MAX_AGENTS": ("40", "0"), "OKENV_PHASE1_RANGE": ("20", "-3"),
    "OKENV_RESIDENT": ("1", "0"), "OKENV_FRONT_BACK": ("0", "1")}.items() for v in vs]


@pytest.mark.parametrize("C", [32, 128, 256])
def test_launch_policy_equals_its_restatement_on_a_sweep_of_shapes(C):
    """The library's launch policy (okenv_debug_plan_step) and tests/_step_forms.py agree far from the rows too: populations from 1 to
    beyond 16 agents per CU with the edges of every rule, fans on both sides of every power of two and beyond 64 rays, each knob
    unset, taken and ignored, the three grid forms, every driver call, one and two tail workgroups per CU.  (The restatement assumes
    that the track image fits the LDS; so does the sweep.)"""
    checked = 0
    for N in sweep_populations(C):
        for R in (1, 5, 15, 16, 17, 32, 33, 64, 65, 200):
            for env, flags in [(e, 0) for e in KNOB_SETTINGS] + [({}, 1), ({}, 2)]:
                shape = T.handle_shape(N, R, C, env, flags)
                may_stay = shape["agents_per_block"] == 1 and N <= 64 and shape["resident_mode"] != 0
                for call in CALLS:
                    if call == "resident" and not (may_stay and shape["coop"]):
                        continue  # (okenv_step_packed starts the resident kernel on no other handle)
                    for fit in (1, 2):
                        real = plan(N, R, C, env, flags, call, fit)
                        want = dict(form=T.first_form(shape, call, fit), lanes_per_agent=shape["G"], phase1_range=shape["phase1"],
                                    rays_per_lane=shape["rays_per_lane"], block_threads=shape["block_threads"],
                                    agents_per_block=shape["agents_per_block"], coop=int(shape["coop"]),
                                    tail_limit=T.tail_limit(shape, fit), resident_eligible=int(may_stay))
                        got = {k: real[k] for k in want}
                        assert got == want, (N, R, C, env, flags, call, fit)
                        checked += 1
    assert checked > 50000


def test_shape_rules_restate_the_launcher():
    """spot checks of the mirror against figures the launcher's comments and other tests state"""
    s = T.handle_shape(4096, 64, 256)                                   # C2: one agent per wave, 16 waves per CU
    assert (s["G"], s["block_threads"], s["agents_per_block"], s["phase1"]) == (64, 1024, 0, 48.0)
    s = T.handle_shape(16384, 16, 256)                                  # C5: four agents to a wave, phase 1 of 32 px
    assert (s["G"], s["phase1"]) == (16, 32.0)
    s = T.handle_shape(50, 15, 256)                                     # the reference's 50 agents: one per workgroup
    assert (s["G"], s["agents_per_block"], s["phase1"], s["block_threads"]) == (64, 1, 0.0, 256)
    assert T.handle_shape(50, 15, 32)["agents_per_block"] == 0          # ... but not on a CPX partition of 32 CUs
    assert T.tail_limit(T.handle_shape(200, 32, 256), 1) == 256
    assert T.tail_limit(T.handle_shape(200, 32, 256, {"OKENV_TAIL_MAX_AGENTS": "40"}), 2) == 40
    assert T.tail_limit(T.handle_shape(200, 32, 256, {"OKENV_COOP": "0"}), 2) == 0
    assert T.tail_limit(T.handle_shape(200, 64, 256), 2) == 512 and T.tail_limit(T.handle_shape(20, 65, 256), 2) == 0
