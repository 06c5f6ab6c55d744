"""examples/flow_racer.py --device-encoder runs to the end at its smallest sizes (64 agents, 32 x 32 frames, one epoch, 16 driven steps),
in graph chunks and eagerly: the trained encoder handed over beside the trunk, no PyTorch op in the driving loop; on the first step the
device encoder's condition agrees with the PyTorch encoder's on the same frames."""
import importlib.util
import os

import pytest
import torch

from test_gpu_bev_encoder import TORCH_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--agents", "64", "--frame-size", "32", "--demo-steps", "16", "--epochs", "1", "--steps", "16", "--episodes", "1", "--device-encoder"]


def example_main():
    spec = importlib.util.spec_from_file_location("flow_racer", os.path.join(ROOT, "examples", "flow_racer.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.main


@pytest.mark.parametrize("extra", [(), ("--graph-chunk", "0")])
def test_example_runs_with_the_device_encoder(gpu, extra, capsys):
    out = example_main()(ARGS + list(extra))
    printed = capsys.readouterr().out
    print(printed)
    assert "trained 1 epochs" in printed and "actions finite True" in printed
    assert "episode 0: 64 agents, 16 steps with the device encoder and act" in printed and "survival" in printed
    assert 0.0 <= out["survival"][0] <= 1.0
    first = out["first"]
    assert tuple(first["cond"].shape) == (64, 128) and bool(torch.isfinite(first["cond"]).all()) and float(first["cond"].abs().max()) > 0
    diff = float((first["cond"] - first["cond_torch"]).abs().max())
    print("device vs PyTorch encoder on the first step: %.3e" % diff)
    assert diff <= TORCH_TOL
