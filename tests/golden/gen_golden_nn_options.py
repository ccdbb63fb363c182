#!/usr/bin/env python3
"""Generate tests/golden/nn_options_f64.npz and nn_options_f32.npz from the
reference: mpc.MPC (GradMethods.ANALYTIC) on an NNDynamics with a slew-rate
penalty or with delta_u, forward and backward.

TEST INFRASTRUCTURE ONLY, as gen_golden.py: it imports the reference
implementation (mounted read-only at /root/reference) in the build container
with the same recipe (flat imports, no bytecode, an empty stand-in for casadi)
and writes data.  It never runs on the GPU box; only the .npz files travel.

Settings are those of gen_golden.py's case J: T = 10, B = 8, lqr_iter = 4,
linesearch_decay 0.2, max_linesearch_iter 10, default eps, exit_unconverged and
detach_unconverged False.  Costs are dense SPD (C = L L^T + I per (t, b)) with
a random c, x0 ~ 0.3 N(0, 1).

Networks (seeded; the fp32 network is the fp64 one cast):
  s32     (5,1) [32]    sigmoid
  s16x8   (5,1) [16, 8] sigmoid
  r16x8   (5,1) [16, 8] relu
  r16np   (4,2) [16]    relu, no passthrough
Cases:
  slew        gamma 0.5, no bounds
  slew_box    gamma 0.5, +-0.2
  slew_prev   gamma 0.5, +-1, prev_ctrl [B,m] ~ 0.2 N(0, 1)
  delta_u     +-1, delta_u 0.05
  delta_u_big +-1, delta_u 0.3
Stored per network: W{i}, b{i}, x0, C, c, wx, wu, prev.  Per network and case:
x, u, costs and the gradients of sum(wx x) + sum(wu u) into x_init (dx0), C
(dC), c (dc) and every weight and bias (dW{i}, db{i}); in the fp32 file also
the reference's own fp32-vs-fp64 spread of x, u and costs (spread_x, spread_u,
spread_costs: max |a32 - a64| / max(1, max |a64|), the tests' relerr).

Condition, checked here: every stored case has a cost spread below 1e-5.  A
draw that does not gets another seed (SEEDS); the bound is not widened.

Usage:  python tests/golden/gen_golden_nn_options.py
"""
import contextlib
import io
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)

if REF not in sys.path:
    sys.path.insert(0, REF)
sys.modules.setdefault("casadi", types.ModuleType("casadi"))
import util  # noqa: E402,F401
import pnqp  # noqa: E402,F401
import mpc as ref_mpc  # noqa: E402  (before lqr_step: the two import each other)
import lqr_step  # noqa: E402,F401
import dynamics as ref_dyn  # noqa: E402

T, B = 10, 8
COST_SPREAD_MAX = 1e-5
MAX_FILE_BYTES = 1 << 20

# tag -> (n, m, hidden, activation, passthrough)
NETS = {
    "s32": (5, 1, [32], "sigmoid", True),
    "s16x8": (5, 1, [16, 8], "sigmoid", True),
    "r16x8": (5, 1, [16, 8], "relu", True),
    "r16np": (4, 2, [16], "relu", False),
}
# tag -> (torch seed of the weights, numpy seed of the problem)
SEEDS = {"s32": (3, 41), "s16x8": (5, 42), "r16x8": (7, 43), "r16np": (11, 44)}
# case -> (slew_rate_penalty, bound, uses prev_ctrl, delta_u)
CASES = {
    "slew": (0.5, None, False, None),
    "slew_box": (0.5, 0.2, False, None),
    "slew_prev": (0.5, 1.0, True, None),
    "delta_u": (None, 1.0, False, 0.05),
    "delta_u_big": (None, 1.0, False, 0.3),
}


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def np_(t):
    return t.detach().cpu().numpy()


def network(tag, dt):
    n, m, hidden, act, pt = NETS[tag]
    torch.manual_seed(SEEDS[tag][0])
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        dx = ref_dyn.NNDynamics(n, m, hidden_sizes=list(hidden), activation=act, passthrough=pt)
    finally:
        torch.set_default_dtype(old)
    return dx.to(dt)


def problem(tag):
    n, m = NETS[tag][:2]
    d = n + m
    rng = np.random.RandomState(SEEDS[tag][1])
    L = rng.normal(size=(T, B, d, d)) * 0.3
    return dict(x0=0.3 * rng.normal(size=(B, n)), C=L @ np.swapaxes(L, -1, -2) + np.eye(d),
                c=0.1 * rng.normal(size=(T, B, d)), wx=rng.normal(size=(T, B, n)), wu=rng.normal(size=(T, B, m)),
                prev=0.2 * rng.normal(size=(B, m)))


def run(tag, case, dt, p):
    n, m = NETS[tag][:2]
    gamma, bound, prev, delta_u = CASES[case]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        dx = network(tag, dt)
        X0 = torch.tensor(p["x0"], dtype=dt, requires_grad=True)
        C = torch.tensor(p["C"], dtype=dt, requires_grad=True)
        c = torch.tensor(p["c"], dtype=dt, requires_grad=True)
        with contextlib.redirect_stdout(io.StringIO()):
            solver = ref_mpc.MPC(n, m, T, lqr_iter=4, grad_method=ref_mpc.GradMethods.ANALYTIC,
                                 u_lower=None if bound is None else -bound, u_upper=bound, n_batch=B,
                                 exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2,
                                 max_linesearch_iter=10, slew_rate_penalty=gamma, delta_u=delta_u,
                                 prev_ctrl=torch.tensor(p["prev"], dtype=dt) if prev else None)
            x, u, costs = solver(X0, ref_mpc.QuadCost(C, c), dx)
            ((x * torch.tensor(p["wx"], dtype=dt)).sum() + (u * torch.tensor(p["wu"], dtype=dt)).sum()).backward()
        out = dict(x=np_(x), u=np_(u), costs=np_(costs), dx0=np_(X0.grad), dC=np_(C.grad), dc=np_(c.grad))
        for i, fc in enumerate(dx.fcs):
            out[f"dW{i}"], out[f"db{i}"] = np_(fc.weight.grad), np_(fc.bias.grad)
    finally:
        torch.set_default_dtype(old)
    return out


def main():
    files = {torch.float64: {}, torch.float32: {}}
    for tag in NETS:
        p = problem(tag)
        for dt, out in files.items():
            npdt = np.float64 if dt == torch.float64 else np.float32
            for i, fc in enumerate(network(tag, dt).fcs):
                out[f"{tag}_W{i}"], out[f"{tag}_b{i}"] = np_(fc.weight), np_(fc.bias)
            out.update({f"{tag}_{k}": v.astype(npdt) for k, v in p.items()})
        for case in CASES:
            r64, r32 = run(tag, case, torch.float64, p), run(tag, case, torch.float32, p)
            spread = {k: relerr(r32[k], r64[k]) for k in r64}
            print(f"  {tag:6s} {case:12s} spread: " + ", ".join(f"{k} {v:.1e}" for k, v in spread.items()))
            assert spread["costs"] < COST_SPREAD_MAX, (
                f"{tag} {case}: the reference's own fp32 cost spread is {spread['costs']:.2e}; draw another seed")
            files[torch.float64].update({f"{tag}_{case}_{k}": v for k, v in r64.items()})
            files[torch.float32].update({f"{tag}_{case}_{k}": v for k, v in r32.items()})
            files[torch.float32].update({f"{tag}_{case}_spread_{k}": np.float64(spread[k])
                                         for k in ("x", "u", "costs")})
    for dt, out in files.items():
        path = os.path.join(OUT, f"nn_options_{'f64' if dt == torch.float64 else 'f32'}.npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(f"  wrote {os.path.basename(path)} ({size / 1024:.1f} KiB)")
        assert size <= MAX_FILE_BYTES, path


if __name__ == "__main__":
    main()
