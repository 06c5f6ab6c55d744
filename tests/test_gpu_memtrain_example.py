"""examples/worldmodel_racer.py --memory --device-encoder --device-update from end to end at tests/test_gpu_memory_example.py's smallest
settings: the memory is trained by okenv_memory_update (worldmodel.train_memory_device), its losses are finite and fall, and the
trained network vector drives a generation through okenv_memory_act."""
import numpy as np
import pytest
import torch

from test_gpu_memory_example import ARGS, example_main

pytestmark = pytest.mark.gpu


def test_example_with_the_memory_trained_on_the_device(gpu, capsys):
    args = list(ARGS)
    args[args.index("--generations") + 1] = "1"
    args[args.index("--memory-epochs") + 1] = "4"
    out = example_main()(args + ["--device-update"])
    printed = capsys.readouterr().out
    print(printed)
    assert "trained the memory (H = 32, 2 layers) 4 epochs on the device" in printed and "fitness finite True" in printed
    assert "generation 0: 8 candidates" in printed and "with the device encoder" in printed
    losses = out["memory_losses"]
    assert len(losses) == 4 and np.isfinite(losses).all() and losses[-1] < losses[0], losses
    vector = out["memory"]
    assert torch.is_tensor(vector) and bool(torch.isfinite(vector).all())
    assert all((out["memory_stats"][k] > 0).all() for k in ("z_std", "a_std"))
    assert len(out["best"]) == 1 and np.isfinite(out["fitness"]).all()
    assert not np.array_equal(out["means"][0], out["means"][-1])
