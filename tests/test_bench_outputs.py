"""bench.py --dump-outputs: the files it writes (names, dtype, the seeded sample
above the size limit), and on the GPU that a plain run prints the headline line
alone and dumps exactly what ops.mpc_solve returns for the same problems."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch


def test_dump_outputs_whole_and_sampled(tmp_path):
    import bench
    T, B = 3, 40
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, B, 5, generator=g)
    u = torch.randn(T, B, 1, generator=g)
    cost = torch.randn(B, generator=g)
    arrays = {"x": (x, 1), "u": (u, 1), "cost": (cost, 0)}
    total = sum(t.numel() * 4 for t, _ in arrays.values())
    # under the limit: every array whole, float32
    bench.dump_outputs(str(tmp_path / "whole"), arrays, limit=total)
    assert sorted(os.listdir(tmp_path / "whole")) == ["cost.npy", "u.npy", "x.npy"]
    for name, (t, _) in arrays.items():
        a = np.load(tmp_path / "whole" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.numpy())
    # above it: the same ascending sample of problems of every array, the same from run to run,
    # and the files together within the limit
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), arrays, limit=total // 4)
    got = {n: np.load(tmp_path / "s1" / f"{n}.npy") for n in arrays}
    keep = got["cost"].shape[0]
    assert 1 <= keep <= B // 4 and sum(a.nbytes for a in got.values()) <= total // 4
    idx = [int(np.flatnonzero(cost.numpy() == v)[0]) for v in got["cost"]]
    assert idx == sorted(idx) and len(set(idx)) == keep
    assert np.array_equal(got["x"], x.numpy()[:, idx]) and np.array_equal(got["u"], u.numpy()[:, idx])
    for n in arrays:
        assert np.array_equal(got[n], np.load(tmp_path / "s2" / f"{n}.npy"))
    # rank r of N > 1 writes its own files and shares the limit
    bench.dump_outputs(str(tmp_path / "r"), arrays, rank=1, world=2, limit=total)
    assert sorted(os.listdir(tmp_path / "r")) == ["cost_rank1.npy", "u_rank1.npy", "x_rank1.npy"]
    assert np.load(tmp_path / "r" / "cost_rank1.npy").shape[0] <= B // 2


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run: --steps sets the timed steps, the line holds the headline
    keys and none of what --full adds, and the dumped arrays are, bit for bit,
    what ops.mpc_solve returns for the same problems."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B, it = 1000, 10
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--batch", str(B), "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["dtype"] == "f32"
    assert line["unit"] == "problem-iters/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(B * it / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"roofline", "roofline_steady_iteration", "roofline_dense_cost", "riccati_roofline", "secondary",
                "cpu_baseline"} & set(line)
    import bench
    from dilqr import ops
    from dilqr import _native as N
    x0n, q, p = bench.make_problems(B)
    dev = torch.device("cuda:0")
    T = bench.T_HORIZON
    C = torch.diag(torch.tensor(q)).repeat(T, B, 1, 1).to(dev).contiguous()
    c = torch.tensor(p).repeat(T, B, 1).to(dev).contiguous()
    theta = torch.tensor([9.8, 1.0, 0.1, 0.5], device=dev)
    x, u, cost, du, _ = ops.mpc_solve(N.MODEL_CARTPOLE, theta, torch.tensor(x0n, device=dev), C, c, T, lqr_iter=it,
                                      eps=0.0, linesearch_decay=0.5, max_linesearch_iter=2, not_improved_lim=10 ** 9)
    assert sorted(os.listdir(tmp_path)) == ["cost.npy", "du.npy", "u.npy", "x.npy"]
    for name, want in (("x", x), ("u", u), ("cost", cost), ("du", du)):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, want.cpu().numpy()), name
