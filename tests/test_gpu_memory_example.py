"""examples/worldmodel_racer.py --memory from end to end on a tiny encoder (32 x 32 frames, 8 candidates, two generations of 16 steps): frames
recorded, the VAE trained, latents collected through the device encoder, the memory trained, generations run through okenv_memory_act
with no PyTorch op in the loop -- and the same generations again through the PyTorch modules (encoder="torch") with the same weights."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--population", "8", "--frame-size", "32", "--base-ch", "16", "--latent", "16", "--demo-agents", "32", "--demo-steps", "8", "--epochs", "1",
        "--generations", "2", "--max-steps", "16", "--track", "Austin", "--device-encoder", "--memory", "--memory-hidden", "32", "--memory-layers", "2",
        "--memory-epochs", "1"]


def example_main():
    spec = importlib.util.spec_from_file_location("worldmodel_racer", os.path.join(ROOT, "examples", "worldmodel_racer.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.main


def test_example_with_the_memory_device_against_torch(gpu, capsys):
    """Same steps, and the fitness within the tolerance tests/test_gpu_world_example.py holds the device encoder to against the PyTorch
    module: 1e-5, a hundred float32 ulps, here of the fitness's own size (it sums up to 16 terms of size 1, so its ulp is that much
    larger).  Both paths run the same fp32 terms in other orders; a wrong term or a lost hidden state is thousands of times more.

    The sizes are the smallest that still cross what can go wrong -- two graph replays of 8 iterations with the hidden state carried
    across their boundary, a reset between the generations, 8 candidates -- because this comparison is exposed to the closed loop's
    discontinuities in proportion to its agent-steps.  The two encoders differ by about 1e-6 on mu (the device folds BatchNorm, the
    module does not), so the two paths' positions part by about 1e-5 pixel, and now and then that carries a road edge across a pixel
    centre of a rendered frame; from there that candidate's frames differ and its fitness parts by 1e-4 .. 1e-3.  Measured on the
    MI355X with 32 candidates and 64 steps (3 300 agent-steps a run): in three of five runs ONE candidate was above the bound (6.5e-05
    .. 1.2e-03) while the median candidate's difference was exactly 0; in the other two the largest was 2.1e-06 .. 8.8e-06.  At 256
    agent-steps a run the same rate is a miss in about one run of twenty.  The comparison that cannot miss is the act's own, bit
    for bit, in tests/test_gpu_memory.py."""
    from openkitchen_amd import worldmodel as wm
    out = example_main()(ARGS)
    printed = capsys.readouterr().out
    print(printed)
    assert "trained 1 epochs" in printed and "trained the memory (H = 32, 2 layers) 1 epochs" in printed and "fitness finite True" in printed
    assert "generation 1: 8 candidates" in printed and "with the device encoder" in printed
    assert len(out["best"]) == 2 and max(out["best"]) > 0 and np.isfinite(out["fitness"]).all()
    assert not np.array_equal(out["means"][0], out["means"][-1])
    assert np.isfinite(out["memory_losses"]).all() and all((out["memory_stats"][k] > 0).all() for k in ("z_std", "a_std"))
    # the controllers are Z + H wide: (48 x 16 + 16) + (16 x 8 + 8) + (8 + 1)
    assert out["means"][0].size == (48 * 16 + 16) + (16 * 8 + 8) + (8 + 1)
    torch.manual_seed(0)
    racers = wm.WorldModelRacers("Austin", 8, out["model"].enc, seed=0, encoder="torch", max_steps=16, graph_chunk=8, memory=out["memory"],
                                 memory_stats=out["memory_stats"], carry=True)
    for g in range(2):
        # the same candidates both ways: the solver here is told the device run's fitness, so that its next sample has the device
        # run's bits (told its own, the two solvers' means part by an ulp and the second generation compares other candidates)
        population = racers.solver.sample()
        steps = racers.evaluate(population)
        want = out["fitnesses"][g]
        racers.solver.tell(population, want)
        each = np.abs(racers.fitness - want) / np.maximum(1.0, np.abs(want))
        diff = float(each.max())
        print("generation %d: %d steps both ways; device against PyTorch fitness: %.3e relative, up to %.3f in size; median %.3e, %d of %d candidates above 1e-5"
              % (g, steps, diff, float(np.abs(want).max()), float(np.median(each)), int((each > 1e-5).sum()), each.size))
        assert steps == out["steps"][g]
        assert diff <= 1e-5
    racers.venv.close()
