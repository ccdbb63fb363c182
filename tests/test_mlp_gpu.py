"""GPU checks of the device MLP dynamics (csrc/tu_mlp.hip, dilqr_mlp_* in
include/dilqr.h) and of the MPC solve that runs on them.

Kernel-level oracle: the torch NNDynamics mirror (dilqr.dynamics, pinned to
autograd by tests/test_generic_cpu.py) evaluated in fp64 on the CPU.  Solver-
level oracle: the reference's own results in tests/golden (stepgen_f64 case M,
generic_f32 case J).  Tolerances are the project's: 2e-5 for a model's forward,
1e-4 for Jacobians, F, f, line-search results and costs, 5e-3 for the NN
problem's trajectories and gradients (the spread the reference shows against
its own fp64 run, tests/test_generic.py), all as relerr with the max(1, .)
normaliser of tests/test_generic.py.  All weights and inputs are seeded on
the CPU.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def gpu(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV, requires_grad=grad)


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_models(n, m, H, act, pt, seed):
    """The same network three times: fp32 on the GPU (whose storage the kernels
    read), and its fp64 copy on the CPU (the oracle)."""
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(seed)
    dx32 = NNDynamics(n, m, hidden_sizes=[H], activation=act, passthrough=pt)
    return copy.deepcopy(dx32).to(DEV), copy.deepcopy(dx32).double()


def golden_model(g):
    from dilqr.dynamics import NNDynamics
    dx = NNDynamics(5, 1, hidden_sizes=[32], activation="sigmoid").to(DEV)
    with torch.no_grad():
        for i, fc in enumerate(dx.fcs):
            fc.weight.copy_(gpu(g[f"nn_W{i}"]))
            fc.bias.copy_(gpu(g[f"nn_b{i}"]))
    return dx


def draw_rows(dx64, rows, n, m, relu):
    """Inputs [rows, n], [rows, m] in fp32-representable fp64.  For relu every
    pre-activation stays clear of 0 (|z| > 1e-3 in fp64), so the fp32 gate
    (a > 0) cannot legitimately differ from the oracle's: rows that come too
    close are drawn again."""
    x = torch.randn(rows, n).double()
    u = torch.randn(rows, m).double()
    if relu:
        W, b = dx64.fcs[0].weight.detach(), dx64.fcs[0].bias.detach()
        for _ in range(200):
            z = torch.cat((x, u), 1) @ W.t() + b
            bad = (z.abs() <= 1e-3).any(1)
            if not bool(bad.any()):
                break
            k = int(bad.sum())
            x[bad], u[bad] = torch.randn(k, n).double(), torch.randn(k, m).double()
        z = torch.cat((x, u), 1) @ W.t() + b
        assert float(z.abs().min()) > 1e-3
    return x, u


# ------------------------------------------------------------------ 1. row kernels
@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("H", [1, 33, 100])
@pytest.mark.parametrize("nm", [(5, 1), (4, 2), (2, 1)], ids=["5x1", "4x2", "2x1"])
def test_row_kernels(nm, H, act, pt):
    """Forward, Jacobian and linearisation of 65 rows (one full wave and a
    one-lane tail) against the fp64 mirror."""
    from dilqr import ops
    n, m = nm
    dxg, dx64 = make_models(n, m, H, act, pt, seed=1000 * n + 100 * m + H)
    x, u = draw_rows(dx64, 65, n, m, act == "relu")
    with torch.no_grad():
        ref = dx64(x, u)
        R, S = dx64.grad_input(x, u)
    D_ref = torch.cat((R, S), 2)
    f_ref = ref - (D_ref @ torch.cat((x, u), 1).unsqueeze(-1)).squeeze(-1)
    md = dxg.device_model(torch.zeros(1, device=DEV))
    assert md is not None and (md.n, md.m, md.H) == (n, m, H)
    xg, ug = x.float().to(DEV), u.float().to(DEV)
    out = ops.mlp_dynamics(md, xg, ug)
    D = ops.mlp_linear_dyn(md, xg, ug)
    F, f = ops.mlp_linearize(md, torch.stack((xg, xg)), torch.stack((ug, ug)))
    errs = {"forward": relerr(cpu(out), ref), "jacobian": relerr(cpu(D), D_ref), "F": relerr(cpu(F[0]), D_ref),
            "f": relerr(cpu(f[0]), f_ref)}
    print(f"\n[mlp rows n={n} m={m} H={H} {act} pt={pt}] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert out.shape == (65, n) and D.shape == (65, n, n + m) and F.shape == (1, 65, n, n + m)
    assert errs["forward"] < 2e-5, errs
    assert max(errs["jacobian"], errs["F"], errs["f"]) < 1e-4, errs
    # the linearisation's F is the Jacobian kernel's, bit for bit (one formula)
    assert torch.equal(F[0], D)


# ------------------------------------------------------------------ 2. linearise vs the reference
def test_linearize_against_reference(golden):
    from dilqr import ops
    g = golden("stepgen_f64")
    dx = golden_model(g)
    md = dx.device_model(torch.zeros(1, device=DEV))
    X, U = gpu(g["nn_X"]), gpu(g["nn_u"])
    F, f = ops.mlp_linearize(md, X, U)
    errs = {"F": relerr(cpu(F), g["nn_F"]), "f": relerr(cpu(f), g["nn_f"])}
    print(f"\n[mlp linearize vs reference] F {errs['F']:.2e}, f {errs['f']:.2e}")
    assert F.shape == g["nn_F"].shape and f.shape == g["nn_f"].shape
    assert max(errs.values()) < 1e-4, errs
    # T = 1: no rows, empty outputs, nothing launched
    F1, f1 = ops.mlp_linearize(md, X[:1], U[:1])
    B = X.shape[1]
    assert F1.shape == (0, B, 5, 6) and f1.shape == (0, B, 5)


# ------------------------------------------------------------------ 3. rollout
@pytest.mark.parametrize("T", [1, 3, 10])
def test_rollout(T):
    from dilqr import ops
    n, m, B = 5, 1, 65
    dxg, dx64 = make_models(n, m, 33, "sigmoid", True, seed=7)
    torch.manual_seed(70 + T)
    x0 = torch.randn(B, n).double()
    u = (0.5 * torch.randn(T, B, m)).double()
    xs = [x0]
    with torch.no_grad():
        for t in range(T - 1):
            xs.append(dx64(xs[t], u[t]))
    ref = torch.stack(xs)
    md = dxg.device_model(torch.zeros(1, device=DEV))
    x0g, ug = x0.float().to(DEV), u.float().to(DEV)
    x = ops.mlp_rollout(md, x0g, ug)
    err = relerr(cpu(x), ref)
    print(f"\n[mlp rollout T={T}] {err:.2e}")
    assert x.shape == (T, B, n)
    assert torch.equal(x[0], x0g)
    assert err < 2e-5 * T
    if T == 3:
        # the rollout is the dynamics kernel chained (one call per step of the
        # horizon), bit for bit
        xt = x0g
        for t in range(T - 1):
            xt = ops.mlp_dynamics(md, xt, ug[t])
            assert torch.equal(x[t + 1], xt), t


# ------------------------------------------------------------------ 4. line search through the ABI
def test_line_search_against_reference(golden):
    from dilqr import ops
    g = golden("stepgen_f64")
    dx = golden_model(g)
    md = dx.device_model(torch.zeros(1, device=DEV))
    X, U, C, c, F = (gpu(g[k]) for k in ("nn_X", "nn_u", "nn_C", "nn_c", "nn_F"))
    K, k, _ = ops.lqr_backward(C, c, F, 5, 1, x=X, u=U, u_lower=-1.0, u_upper=1.0)
    nx, nu, costs, du_sq, alpha = ops.lqr_forward(md, None, gpu(g["nn_x0"]), C, c, X, U, K, k, u_lower=-1.0,
                                                  u_upper=1.0, linesearch_decay=0.2, max_linesearch_iter=10)
    du = ops.quirk_norm(du_sq)
    errs = {name: relerr(cpu(a), g[f"nn_explicit_{name}"]) for name, a in
            (("nx", nx), ("nu", nu), ("costs", costs), ("du", du), ("malpha", alpha.mean()))}
    print("\n[mlp line search vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert max(errs.values()) < 1e-4, errs
    # MODEL_MLP with the descriptor as theta is the same call
    from dilqr import _native as N
    nx2, nu2, costs2, _, alpha2 = ops.lqr_forward(N.MODEL_MLP, md, gpu(g["nn_x0"]), C, c, X, U, K, k, u_lower=-1.0,
                                                  u_upper=1.0, linesearch_decay=0.2, max_linesearch_iter=10)
    assert torch.equal(nx, nx2) and torch.equal(nu, nu2) and torch.equal(costs, costs2) and torch.equal(alpha, alpha2)


# ------------------------------------------------------------------ 5-7. the MPC solve
B65 = 65


def solve65(g, dx):
    """generic_f32's eight NN problems tiled cyclically to 65 (problem b is
    golden problem b % 8), solved with the fixture's settings under no_grad."""
    import dilqr.mpc as cmpc
    from dilqr import QuadCost
    idx = np.arange(B65) % 8
    T = g["nn_C"].shape[0]
    m = cmpc.MPC(5, 1, T, lqr_iter=4, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0, u_upper=1.0,
                 n_batch=B65, exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2,
                 max_linesearch_iter=10)
    with torch.no_grad():
        return m(gpu(g["nn_x0"][idx]), QuadCost(gpu(g["nn_C"][:, idx]), gpu(g["nn_c"][:, idx])), dx)


def test_mpc_against_reference_b65(golden, monkeypatch):
    from dilqr import generic
    g = golden("generic_f32")
    dx = golden_model(g)
    idx = np.arange(B65) % 8
    assert generic.DEVICE_MLP is True
    x, u, costs = solve65(g, dx)
    errs = {"costs": relerr(cpu(costs), g["nn_analytic_costs"][idx]), "x": relerr(cpu(x), g["nn_analytic_x"][:, idx]),
            "u": relerr(cpu(u), g["nn_analytic_u"][:, idx])}
    print("\n[mlp MPC B=65 vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert errs["costs"] < 1e-4, errs
    assert max(errs["x"], errs["u"]) < 5e-3, errs
    # lanes are independent: every copy of a golden problem is the same bits
    first = torch.as_tensor(idx, device=DEV)
    assert torch.equal(x, x[:, first]) and torch.equal(u, u[:, first]) and torch.equal(costs, costs[first])
    # the torch loop on the same inputs
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    xt, ut, costs_t = solve65(g, dx)
    err = relerr(cpu(costs), cpu(costs_t))
    print(f"[mlp MPC B=65 device vs torch loop] costs {err:.2e}")
    assert err < 1e-4
    assert relerr(cpu(costs_t), g["nn_analytic_costs"][idx]) < 1e-4


def test_device_path_really_ran(golden, monkeypatch):
    """The device solve never evaluates the Module; the torch loop must."""
    from dilqr import generic
    from dilqr.dynamics import NNDynamics
    g = golden("generic_f32")
    dx = golden_model(g)

    def boom(self, x, u):
        raise AssertionError("NNDynamics.forward called")

    monkeypatch.setattr(NNDynamics, "forward", boom)
    x, u, costs = solve65(g, dx)
    assert relerr(cpu(costs), g["nn_analytic_costs"][np.arange(B65) % 8]) < 1e-4
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    with pytest.raises(AssertionError, match="forward called"):
        solve65(g, dx)


def test_backward_reaches_the_weights(golden):
    """tests/test_generic.py's analytic case at B = 8: the device solve, then
    the torch final_step (differentiable linearisation, classic adjoint);
    gradients into the network, the cost and x_init against the reference."""
    import dilqr.mpc as cmpc
    from dilqr import QuadCost, generic
    g = golden("generic_f32")
    dx = golden_model(g)
    T, B = g["nn_C"].shape[:2]
    assert generic.DEVICE_MLP is True and dx.device_model(torch.zeros(1, device=DEV)) is not None
    X0, C, c = gpu(g["nn_x0"], True), gpu(g["nn_C"], True), gpu(g["nn_c"], True)
    m = cmpc.MPC(5, 1, T, lqr_iter=4, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0, u_upper=1.0, n_batch=B,
                 exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=10)
    x, u, costs = m(X0, QuadCost(C, c), dx)
    assert relerr(cpu(costs), g["nn_analytic_costs"]) < 1e-4
    assert relerr(cpu(u), g["nn_analytic_u"]) < 5e-3
    assert relerr(cpu(x), g["nn_analytic_x"]) < 5e-3
    ((x * gpu(g["nn_wx"])).sum() + (u * gpu(g["nn_wu"])).sum()).backward()
    errs = {"dx0": relerr(cpu(X0.grad), g["nn_analytic_dx0"]), "dC": relerr(cpu(C.grad), g["nn_analytic_dC"]),
            "dc": relerr(cpu(c.grad), g["nn_analytic_dc"])}
    for i, fc in enumerate(dx.fcs):
        errs[f"dW{i}"] = relerr(cpu(fc.weight.grad), g[f"nn_analytic_dW{i}"])
        errs[f"db{i}"] = relerr(cpu(fc.bias.grad), g[f"nn_analytic_db{i}"])
    print("\n[mlp MPC backward vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert max(errs.values()) < 5e-3, errs
