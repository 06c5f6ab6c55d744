"""examples/bc_racer.py --device-policy runs to the end at small sizes (64 agents, 48 x 48 frames, 16 demonstration steps, one epoch, 16
driven steps), in graph chunks and eagerly: the trained policy handed over, no PyTorch op in the driving loop; on the first step the
device's output agrees with the PyTorch forward's on the same frames."""
import importlib.util
import os

import pytest
import torch

from test_gpu_cnn import TORCH_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--agents", "64", "--frame-size", "48", "--demo-steps", "16", "--epochs", "1", "--steps", "16", "--episodes", "1", "--device-policy"]


def example_main():
    spec = importlib.util.spec_from_file_location("bc_racer", os.path.join(ROOT, "examples", "bc_racer.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.main


@pytest.mark.parametrize("extra", [(), ("--graph-chunk", "0")])
def test_example_runs_with_the_device_policy(gpu, extra, capsys):
    out = example_main()(ARGS + list(extra))
    printed = capsys.readouterr().out
    print(printed)
    assert "trained 1 epochs" in printed and "actions finite True" in printed
    assert "episode 0: 64 agents, 16 steps with the device policy" in printed and "survival" in printed
    assert 0.0 <= out["survival"][0] <= 1.0
    first = out["first"]
    assert tuple(first["out"].shape) == (64,) and bool(torch.isfinite(first["out"]).all()) and float(first["out"].abs().max()) > 0
    diff = float((first["out"] - first["out_torch"]).abs().max())
    print("device vs PyTorch forward on the first step: %.3e" % diff)
    assert diff <= TORCH_TOL
