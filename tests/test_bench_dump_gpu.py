"""bench.py --dump-outputs on the GPU: the dumped arrays are the state the timed steps left (the same model stepped in this process
the same number of times from the same initial condition), --steps sets the number of timed steps, and the line carries ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_hold_the_last_timed_step(swmhd, tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    N, K, W = 128, 3, 2
    argv = ["--gpus", "1", "--size", str(N), "--steps", str(K), "--warmup", str(W), "--cpu-seconds", "0"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, BENCH] + argv + ["--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == K and line["ms_per_step"] > 0 and line["outputs_dump"]["sample"] is None

    # the same workload stepped here: 40 spin-up + W warm-up + K timed steps
    args = bench.parse(argv)
    cfg, Nx, Nyg, _, form, _, ydom = bench.workload(args, 1)
    dec = swmhd.SlabDecomposition(Nyg, 1, 0)
    g = dec.local_grid(swmhd.RectilinearGrid, Nx, x=cfg["domain"]["x"], y=ydom, halo=dec.ring_halo())
    dt = 0.2 * min(g.dx, g.dy) / 4.2
    m = swmhd.ShallowWaterModel(g, 9.81, 1.0, formulation=form, decomp=dec)
    n1, n2 = m.names[:2]
    m.set(**{n1: cfg["u"], n2: cfg["v"], "h": lambda X, Y: cfg["h"](X, Y) + 0 * X, "A": cfg["A"]})
    for _ in range(40 + W + K):
        m.time_step(dt)
    m.synchronize()
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in m.names)
    for n, f in zip(m.names, m.fields):
        got = np.load(tmp_path / f"{n}.npy", allow_pickle=False)
        want = f.interior().cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (N, N)
        assert np.isfinite(got).all() and np.array_equal(got, want), n
    m.close()
    torch.cuda.synchronize()
