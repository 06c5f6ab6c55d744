"""examples/flow_racer.py runs to the end at its smallest sizes (64 agents, 32 x 32 frames, one epoch, 16 driven steps): demonstrations
with frames from the device expert, PyTorch training, the hand-over and the drive; on the recorded first step the device sampler
agrees with flow.sample on the trained trunk from the same noise and condition."""
import copy
import importlib.util
import os

import pytest
import torch

from test_flow_rule import HOST_VS_MIRROR_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--agents", "64", "--frame-size", "32", "--demo-steps", "16", "--epochs", "1", "--steps", "16", "--episodes", "1"]
# flow.sample in fp32 on the GPU sums its Linear layers in the BLAS library's order, on cat([x, t, embedding]): its own rounding on top
# of the device's.  Measured on the MI355X over the three runs below: 1.6e-7 .. 2.4e-7 against the fp32 module, 2.1e-7 .. 2.5e-7 against
# the trunk's float64 copy (34 % of the outputs on the clamp) -- both inside the bound of tests/test_flow_rule.py (4 x 2.75e-7), which
# is what both are held to.


def example_main():
    spec = importlib.util.spec_from_file_location("flow_racer", os.path.join(ROOT, "examples", "flow_racer.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.main


@pytest.mark.parametrize("extra", [(), ("--torch-sampler",), ("--graph-chunk", "0")])
def test_example_runs(gpu, extra, capsys):
    from openkitchen_amd import flow
    out = example_main()(ARGS + list(extra))
    printed = capsys.readouterr().out
    print(printed)
    assert "trained 1 epochs" in printed and "episode 0: 64 agents, 16 steps" in printed and "actions finite True" in printed
    cfg, first = out["config"], out["first"]
    lo, hi = (torch.tensor(list(v), device="cuda") for v in (cfg.action_lo, cfg.action_hi))
    for action in (first["action"], torch.stack([out["throttle"], out["steering"]], dim=1)):
        assert bool(torch.isfinite(action).all()) and bool((action >= lo).all()) and bool((action <= hi).all())
    assert 0.0 <= out["survival"][0] <= 1.0
    # the recorded iteration against the PyTorch loop from the same x0 and cond: the trunk's float64 copy, then the fp32 module itself
    trunk64 = copy.deepcopy(out["model"].action_flow_trunk).double()
    want64 = flow.sample(trunk64, first["cond"].double(), first["x0"].double(), cfg.steps)
    want32 = flow.sample(out["model"], first["cond"], first["x0"], cfg.steps)
    err64 = float((first["x"].double() - want64).abs().max())
    err32 = float((first["x"] - want32).abs().max())
    on_clamp = float((want64.abs() == 1.0).float().mean())
    print("device vs float64 sampler %.3g, vs fp32 sampler %.3g; %.0f %% of the outputs on the clamp" % (err64, err32, 100 * on_clamp))
    assert on_clamp < 0.5
    assert err64 <= HOST_VS_MIRROR_TOL
    assert err32 <= HOST_VS_MIRROR_TOL
