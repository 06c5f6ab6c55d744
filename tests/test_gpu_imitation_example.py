"""examples/imitation_racer.py --small runs to the end: demonstrations from the device expert, two epochs of PyTorch training, the
hand-over and 64 driven steps; on the first driven step the device act agrees with the module's float64 forward from the same
weights within the bound of tests/test_lidar_rule.py."""
import os
import re
import subprocess
import sys

import pytest

from test_lidar_rule import HOST_VS_MIRROR_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [(), ("--torch-driver",)])
def test_example_runs(gpu, extra):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "imitation_racer.py"), "--small"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "trained 2 epochs" in r.stdout and "drove 64 agents for 64 steps" in r.stdout and "actions finite True" in r.stdout
    m = re.search(r"first step: max \|device - float64 module\| = (\S+) \(normalised outputs up to (\S+)\)", r.stdout)
    assert m, r.stdout
    assert float(m.group(2)) > 0.05, "the outputs are too small for an absolute bound to say anything"
    assert float(m.group(1)) <= HOST_VS_MIRROR_TOL
