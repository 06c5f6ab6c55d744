"""examples/dqn_cnn_racer.py --device-policy runs to the end at small sizes (64 agents, 48 x 48 frames, two episodes of 16 steps, one
sequential pass in batches of 64), eagerly and in graph chunks: the ring filled and emptied, epsilon lowered, the parameters updated in
PyTorch and handed over, no PyTorch op in the acting loop; on the first step the device's Q-values agree with the PyTorch forward's."""
import importlib.util
import os

import pytest
import torch

from test_gpu_qcnn import TORCH_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--agents", "64", "--frame-size", "48", "--episodes", "2", "--max-steps", "16", "--capacity", "2048", "--batch", "64", "--passes", "1",
        "--device-policy"]


def example_main():
    spec = importlib.util.spec_from_file_location("dqn_cnn_racer", os.path.join(ROOT, "examples", "dqn_cnn_racer.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.main


@pytest.mark.parametrize("extra", [(), ("--graph-chunk", "4")])
def test_example_runs_with_the_device_policy(gpu, extra, capsys):
    out = example_main()(ARGS + list(extra))
    printed = capsys.readouterr().out
    print(printed)
    assert "episode 0: eps 0.99, 16 steps" in printed and "episode 1: eps 0.98, 16 steps" in printed
    assert out["steps"] == [16, 16] and out["epsilon"] == [0.99, 0.98] and abs(out["final_epsilon"] - 0.97) < 1e-12
    # the ring was filled (every agent is alive on an episode's first step; crashed ones drop out later) and emptied
    for size, pushed in out["ring"]:
        assert 64 <= size == pushed <= 16 * 64
    assert out["ring_after"] == (0, 0)
    assert all(loss == loss and loss >= 0 for loss in out["loss"])
    # the update moved the parameters, and the device holds the module's
    assert not torch.equal(out["params"], out["params_first"]) and bool(torch.isfinite(out["params"]).all())
    assert torch.equal(out["device_params"], out["params"])
    q, q_torch = out["q"], out["q_torch"]
    assert tuple(q.shape) == (64, 5) and bool(torch.isfinite(q).all()) and float(q.abs().max()) > 0
    diff = float((q - q_torch).abs().max())
    print("device vs PyTorch Q-values on the first step: %.3e (largest |q| %.3f)" % (diff, float(q_torch.abs().max())))
    assert diff <= TORCH_TOL["reference"]
