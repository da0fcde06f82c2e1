"""The command-line example (examples/run_swmhd.py) runs over a hill (--bump) and under a Kolmogorov force (--body-force), alone and
beside the drag, the beta plane and the stirring."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra,says", [(["--bump", "0.3,1.5"], "bathymetry"),
                                        (["--bump", "0.3,1.5", "--formulation", "divergence", "--ic", "gaussians"], "bathymetry"),
                                        (["--body-force", "0.5,1.2566", "--drag", "0.05", "--beta", "0.2", "--stir", "0.01,3"], "Source(0.5 sin(1.2566 y))"),
                                        (["--channel", "--gradients", "-0.01", "--bump", "0.2,1.0", "--body-force", "0.1,0.6283"], "bathymetry")],
                         ids=["bump", "bump-conservative", "body-force", "channel"])
def test_example_runs_with_a_source(tmp_path, extra, says):
    """64^2 for a few steps: the progress lines, the dump and its fields exist and are finite; the thickness over the hill starts as 1 - b."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "run_swmhd.py"), "--size", "64", "--stop-time", "0.1", "--every", "5",
           "--dump-every", "0.1", "--out", str(tmp_path)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert says in r.stdout
    lines = [l for l in r.stdout.splitlines() if l.startswith("Time:")]
    assert len(lines) >= 2
    if "--bump" in extra:
        height = float(extra[extra.index("--bump") + 1].split(",")[0])
        assert abs(float(lines[0].split("min(h):")[1].split(",")[0]) - (1.0 - height)) < 0.05 * height      # (the centre lies between cells)
    z = np.load(os.path.join(str(tmp_path), "fields_0000010.npz"))
    for n in (("uh", "vh") if "divergence" in extra else ("u", "v")) + ("h", "A"):
        assert np.isfinite(z[n]).all()
