"""worldmodel.WorldModelRacers with the device encoder at small sizes (32 x 32 frames, 32 candidates, two generations) and
examples/worldmodel_racer.py --device-encoder from end to end at that size: frames recorded, the VAE trained, the encoder handed over,
generations run with no PyTorch op in the loop."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--population", "32", "--frame-size", "32", "--base-ch", "16", "--latent", "16", "--demo-agents", "32", "--demo-steps", "8", "--epochs", "1",
        "--generations", "2", "--max-steps", "64", "--track", "Austin", "--device-encoder"]


def test_two_generations_with_the_device_encoder(gpu):
    from openkitchen_amd import worldmodel as wm
    torch.manual_seed(0)
    racers = wm.WorldModelRacers("Austin", 32, wm.Encoder(32, 16, (16, 32, 64, 128)), seed=0, encoder="device", max_steps=64, graph_chunk=8)
    assert racers.num_params == (18 * 16 + 16) + (16 * 8 + 8) + (8 + 1) and racers.config.skip_crashed == 1
    mean0 = racers.solver.mean.copy()
    tops = []
    for _ in range(2):
        top, steps = racers.run_generation()
        assert 0 < steps <= 64 and steps % 8 == 0
        assert racers.fitness.shape == (32,) and np.isfinite(racers.fitness).all() and top == racers.fitness.max()
        tops.append(top)
    assert max(tops) > 0
    assert not np.array_equal(racers.solver.mean, mean0) and np.isfinite(racers.solver.mean).all()
    assert racers.generation == 2
    racers.venv.close()


def example_main():
    spec = importlib.util.spec_from_file_location("worldmodel_racer", os.path.join(ROOT, "examples", "worldmodel_racer.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.main


def test_example_runs_with_the_device_encoder(gpu, capsys):
    out = example_main()(ARGS)
    printed = capsys.readouterr().out
    print(printed)
    assert "trained 1 epochs" in printed and "fitness finite True" in printed
    assert "generation 1: 32 candidates" in printed and "with the device encoder" in printed
    assert len(out["best"]) == 2 and max(out["best"]) > 0 and np.isfinite(out["fitness"]).all()
    assert not np.array_equal(out["means"][0], out["means"][-1])
    first = out["first"]
    diff = float((first["mu"] - first["mu_torch"])[first["mu"].abs().sum(dim=1) > 0].abs().max())
    print("device vs PyTorch module on the first frames: %.3e on mu up to %.3f" % (diff, float(first["mu_torch"].abs().max())))
    # a trained encoder's BatchNorm is folded in: fp32 sums of a few thousand terms of size below 1 in another order (1e-5 is a
    # hundred float32 ulps of 1 and a thousand times below a wrong term)
    assert diff <= 1e-5
