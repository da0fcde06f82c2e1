"""The command-line example (examples/run_swmhd.py) carries particles (--particles N --track ...), in a periodic box and in a channel,
and writes their samples."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra,names,samples", [(["--track", "A,h", "--frames", "0.05"], ["x", "y", "A", "h"], 3),
                                                 (["--formulation", "divergence", "--ic", "gaussians", "--track", "A,uh"], ["x", "y", "A", "uh"], 2),
                                                 (["--channel", "--gradients", "-0.05", "--drag", "0.05", "--track", "v,h"], ["x", "y", "v", "h"], 2)],
                         ids=["periodic", "conservative", "channel"])
def test_example_carries_particles(tmp_path, extra, names, samples):
    """64^2 for ten steps with a 10 x 10 lattice: the samples exist, are finite, stay in the box, and the particles have moved"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.1", "--every", "5",
           "--particles", "97", "--out", str(tmp_path)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "particles: a 10 x 10 lattice" in r.stdout
    z = np.load(os.path.join(str(tmp_path), "particles.npz"))
    assert list(z["names"]) == names and z["samples"].shape == (samples, len(names), 100) and z["samples"].dtype == np.float64
    assert list(z["iterations"]) == ([0, 5, 10] if samples == 3 else [0, 10])
    s = z["samples"]
    assert np.isfinite(s).all() and np.all(np.abs(s[:, :2]) <= 5.0)
    assert np.array_equal(s[0, 0, :10], -5.0 + (np.arange(10) + 0.5)) and not np.array_equal(s[-1, :2], s[0, :2])
    if "A" in names:
        assert "A along the trajectories: drift max" in r.stdout     # (the frozen-in flux: printed, not held to a number)
