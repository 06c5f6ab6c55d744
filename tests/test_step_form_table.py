"""The step-form table (tests/_step_forms.py) stays complete: every hipLaunchKernelGGL of a step kernel in okenv_capi.hip is
counted as one form of enum okenv_step_form, the enum, the Python names and the GPU rows agree one to one, and every row's shape
implies its form under the launcher's rules for a device of 32, 128 or 256 compute units (the partition modes of an MI355X).
No GPU needed."""
import os
import re

import pytest

import _step_forms as T
from openkitchen_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "openkitchen_amd", "csrc", "okenv_capi.hip")
HDR = os.path.join(ROOT, "include", "okenv.h")

LAUNCH = re.compile(r"hipLaunchKernelGGL\(\s*\(?\s*(okStep\w*Kernel(?:<[^>]*>)?)\s*\)?\s*,")
COUNT = re.compile(r"countForm\(h,\s*OKENV_FORM_(\w+),\s*p\);\s*$")


def launch_sites(src):
    """[(form or None, kernel)] for every step-kernel launch: the form of the countForm(h, OKENV_FORM_..., p) statement right
    before it (only blanks between them), None when there is none."""
    src = re.sub(r"//[^\n]*", "", src)
    sites = []
    for m in LAUNCH.finditer(src):
        c = COUNT.search(src[:m.start()].rstrip())
        sites.append((c.group(1).lower() if c else None, re.sub(r"\s+", "", m.group(1))))
    return sites


def enum_forms(hdr):
    body = re.search(r"enum okenv_step_form\s*\{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n[len("OKENV_FORM_"):].lower() for n in re.findall(r"\b(OKENV_FORM_\w+)", body)]


def test_every_step_launch_is_counted_once_as_its_form():
    sites = launch_sites(open(SRC).read())
    assert len(sites) == 22
    uncounted = [k for f, k in sites if f is None]
    assert not uncounted, "step-kernel launches without a countForm in front of them: %s" % uncounted
    forms = [f for f, _ in sites]
    assert sorted(forms) == sorted(T.FORMS), "each form is counted at exactly one launch site"
    for f, k in sites:
        assert T.KERNELS[f] == k, "OKENV_FORM_%s counts a launch of %s" % (f.upper(), k)


def test_an_uncounted_launch_fails_the_check():
    """what the check above catches: a copy of the source with one more, uncounted instantiation"""
    src = open(SRC).read()
    at = src.index("    OK_HIP(h, hipGetLastError());\n    h->resident = true;")
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
    """okenv_create and launchStep restated (tests/_step_forms.py: handle_shape, tail_limit, first_form): each row's population,
    fan and knobs pick its form whatever the device's CU count, and whether one or two tail workgroups share a CU."""
    for r in T.ROWS:
        N = T.population(r, C)
        shape = T.handle_shape(N, r["R"], C, r["env"], r["flags"])
        for fit in (1, 2):
            got = T.first_form(shape, T.DRIVER_CALL[r["driver"]], fit)
            assert got == r["form"], (r["id"], C, fit, got, shape)


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
