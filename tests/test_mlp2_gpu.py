"""GPU checks of the two-hidden-layer device MLP dynamics (csrc/tu_mlp2.hip,
dilqr_mlp2_* in include/dilqr.h) and of the MPC solve that runs on them with
generic.DEVICE_MLP_DEEP on.

Kernel-level oracle: the torch NNDynamics mirror (dilqr.dynamics) evaluated in
fp64 on the CPU, as in tests/test_mlp_gpu.py.  Solver-level oracle: the torch
loop on the same module (the switch off).  Tolerances are the project's: 2e-5
for a model's forward, 1e-4 for Jacobians, F, f and costs, 5e-3 for the NN
problem's trajectories and gradients, all as relerr with the max(1, .)
normaliser.  All weights and inputs are seeded on the CPU; the inputs of the
row kernels are N(0, 1), at which the fp32 torch mirror on the CPU stays within
half of those tolerances of the fp64 one on every case below (measured on the
same seeds: forward <= 4.2e-7, Jacobian <= 1.1e-7, f <= 5.6e-7, the rollouts
<= 9.0e-8), so no smaller input scale is needed.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(5, 1), (4, 2), (2, 1)]
WIDTHS = [(1, 1), (33, 7), (7, 33), (64, 64), (256, 3)]      # (256, .): the 64 KiB LDS launch
ROWS = 65                                                     # one full wave and a one-lane tail


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


def make_cpu_models(n, m, widths, act, pt, seed):
    """The same seeded network in fp32 and in fp64 (the oracle), on the CPU."""
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(seed)
    dx32 = NNDynamics(n, m, hidden_sizes=list(widths), activation=act, passthrough=pt)
    return dx32, copy.deepcopy(dx32).double()


def pre_activations(dx64, x, u):
    """Every hidden pre-activation of a row, both layers, in fp64: [rows, H1 + H2]."""
    z, out = torch.cat((x, u), 1), []
    for fc in dx64.fcs[:-1]:
        z = z @ fc.weight.detach().t() + fc.bias.detach()
        out.append(z)
        z = torch.relu(z) if dx64.activation == "relu" else torch.sigmoid(z)
    return torch.cat(out, 1)


def draw_rows(dx64, rows, n, m, relu):
    """Inputs [rows, n], [rows, m] in fp32-representable fp64.  For relu every
    pre-activation of both layers stays clear of 0 (|z| > 1e-3 in fp64), so the
    fp32 gate (a > 0) cannot legitimately differ from the oracle's: rows that
    come too close are drawn again, 200 rounds at the most."""
    x = torch.randn(rows, n).double()
    u = torch.randn(rows, m).double()
    if relu:
        for _ in range(200):
            bad = (pre_activations(dx64, x, u).abs() <= 1e-3).any(1)
            if not bool(bad.any()):
                break
            k = int(bad.sum())
            x[bad], u[bad] = torch.randn(k, n).double(), torch.randn(k, m).double()
        assert float(pre_activations(dx64, x, u).abs().min()) > 1e-3
    return x, u


def row_case(n, m, widths, act, pt):
    """One row-kernel case: the CPU models, the rows and the fp64 reference."""
    dx32, dx64 = make_cpu_models(n, m, widths, act, pt, seed=100000 * n + 10000 * m + 300 * widths[0] + widths[1])
    x, u = draw_rows(dx64, ROWS, n, m, act == "relu")
    with torch.no_grad():
        ref = dx64(x, u)
        R, S = dx64.grad_input(x, u)
    D_ref = torch.cat((R, S), 2)
    f_ref = ref - (D_ref @ torch.cat((x, u), 1).unsqueeze(-1)).squeeze(-1)
    return dx32, dx64, x, u, ref, D_ref, f_ref


def deep_model(dxg):
    md = dxg.device_model(torch.zeros(1, device=DEV), deep=True)
    assert md is not None
    return md


# ------------------------------------------------------------------ 1. row kernels
@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("widths", WIDTHS, ids=[f"{a}-{b}" for a, b in WIDTHS])
@pytest.mark.parametrize("nm", SHAPES, ids=["5x1", "4x2", "2x1"])
def test_row_kernels(nm, widths, act, pt):
    """Forward, Jacobian and linearisation of 65 rows against the fp64 mirror."""
    from dilqr import ops
    n, m = nm
    dx32, dx64, x, u, ref, D_ref, f_ref = row_case(n, m, widths, act, pt)
    dxg = copy.deepcopy(dx32).to(DEV)
    md = deep_model(dxg)
    assert isinstance(md, ops.Mlp2Model) and (md.n, md.m, md.H1, md.H2) == (n, m) + widths
    xg, ug = x.float().to(DEV), u.float().to(DEV)
    out = ops.mlp_dynamics(md, xg, ug)
    D = ops.mlp_linear_dyn(md, xg, ug)
    F, f = ops.mlp_linearize(md, torch.stack((xg, xg)), torch.stack((ug, ug)))
    errs = {"forward": relerr(cpu(out), ref), "jacobian": relerr(cpu(D), D_ref), "F": relerr(cpu(F[0]), D_ref),
            "f": relerr(cpu(f[0]), f_ref)}
    print(f"\n[mlp2 rows n={n} m={m} H={widths} {act} pt={pt}] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert out.shape == (ROWS, n) and D.shape == (ROWS, n, n + m) and F.shape == (1, ROWS, n, n + m)
    assert f.shape == (1, ROWS, n)
    assert errs["forward"] < 2e-5, errs
    assert max(errs["jacobian"], errs["F"], errs["f"]) < 1e-4, errs
    # the linearisation's F is the Jacobian kernel's, bit for bit (one formula)
    assert torch.equal(F[0], D)


def test_linearize_t1_is_empty():
    from dilqr import ops
    dx32, _ = make_cpu_models(5, 1, (33, 7), "sigmoid", True, seed=3)
    md = deep_model(dx32.to(DEV))
    F1, f1 = ops.mlp_linearize(md, torch.zeros(1, ROWS, 5, device=DEV), torch.zeros(1, ROWS, 1, device=DEV))
    assert F1.shape == (0, ROWS, 5, 6) and f1.shape == (0, ROWS, 5)


# ------------------------------------------------------------------ 2. rollout
@pytest.mark.parametrize("T", [1, 3, 10])
def test_rollout(T):
    from dilqr import ops
    n, m, B = 5, 1, ROWS
    dx32, dx64 = make_cpu_models(n, m, (33, 7), "sigmoid", True, seed=7)
    torch.manual_seed(70 + T)
    x0 = torch.randn(B, n).double()
    u = (0.5 * torch.randn(T, B, m)).double()
    xs = [x0]
    with torch.no_grad():
        for t in range(T - 1):
            xs.append(dx64(xs[t], u[t]))
    ref = torch.stack(xs)
    md = deep_model(dx32.to(DEV))
    x0g, ug = x0.float().to(DEV), u.float().to(DEV)
    x = ops.mlp_rollout(md, x0g, ug)
    err = relerr(cpu(x), ref)
    print(f"\n[mlp2 rollout T={T}] {err:.2e}")
    assert x.shape == (T, B, n)
    assert torch.equal(x[0], x0g)
    assert err < 2e-5 * T
    if T == 3:
        # the rollout is the dynamics kernel chained (one call per step), bit for bit
        xt = x0g
        for t in range(T - 1):
            xt = ops.mlp_dynamics(md, xt, ug[t])
            assert torch.equal(x[t + 1], xt), t


# ------------------------------------------------------------------ 3. line search through the ABI
def test_line_search_through_the_abi(golden):
    """lqr_forward on the model: gains from the sweep on the kernel's own F; the
    model in place of model_id and MODEL_MLP with it as theta are one call; the
    cost it returns is the cost of the trajectory it returns."""
    from dilqr import _native as N
    from dilqr import ops
    g = golden("generic_f32")
    dxg = seeded_module()
    md = deep_model(dxg)
    idx = np.arange(B65) % 8
    x0, C, c = gpu(g["nn_x0"][idx]), gpu(g["nn_C"][:, idx]), gpu(g["nn_c"][:, idx])
    T = C.shape[0]
    torch.manual_seed(11)
    U = (0.3 * torch.randn(T, B65, 1)).to(DEV)
    X = ops.mlp_rollout(md, x0, U)
    F, _ = ops.mlp_linearize(md, X, U)
    K, k, _ = ops.lqr_backward(C, c, F, 5, 1, x=X, u=U, u_lower=-1.0, u_upper=1.0)
    kw = dict(u_lower=-1.0, u_upper=1.0, linesearch_decay=0.2, max_linesearch_iter=10)
    nx, nu, costs, du_sq, alpha = ops.lqr_forward(md, None, x0, C, c, X, U, K, k, **kw)
    nx2, nu2, costs2, du_sq2, alpha2 = ops.lqr_forward(N.MODEL_MLP, md, x0, C, c, X, U, K, k, **kw)
    assert torch.equal(nx, nx2) and torch.equal(nu, nu2) and torch.equal(costs, costs2)
    assert torch.equal(alpha, alpha2) and torch.equal(du_sq, du_sq2)
    assert float(nu.abs().max()) <= 1.0 and torch.equal(nx[0], x0)
    def own_cost(xs, us):
        tau = np.concatenate((cpu(xs), cpu(us)), 2)
        return (0.5 * np.einsum("tbi,tbij,tbj->tb", tau, cpu(C), tau) + np.einsum("tbi,tbi->tb", tau, cpu(c))).sum(0)

    err = relerr(cpu(costs), own_cost(nx, nu))
    print(f"\n[mlp2 line search] cost vs fp64 cost of its own trajectory {err:.2e}, mean alpha {float(alpha.mean()):.3f}")
    assert err < 1e-5
    # along -k the cost climbs, so the search has to backtrack: the passes after
    # the first run the same rollout, and the cost is still the trajectory's own
    bx, bu, bcosts, _, balpha = ops.lqr_forward(md, None, x0, C, c, X, U, K, -k, **kw)
    err = relerr(cpu(bcosts), own_cost(bx, bu))
    print(f"[mlp2 line search, -k] cost vs its own trajectory {err:.2e}, mean alpha {float(balpha.mean()):.2e}")
    assert float(balpha.min()) < 1.0
    assert err < 1e-5


# ------------------------------------------------------------------ 4-6. the MPC solve
B65 = 65


def seeded_module():
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(2024)
    return NNDynamics(5, 1, hidden_sizes=[32, 32]).to(DEV)


def solver(T, B):
    import dilqr.mpc as cmpc
    return cmpc.MPC(5, 1, T, lqr_iter=4, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0, u_upper=1.0,
                    n_batch=B, exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2,
                    max_linesearch_iter=10)


def solve65(g, dx):
    """generic_f32's eight NN problems tiled cyclically to 65 (problem b is
    golden problem b % 8), solved under no_grad."""
    from dilqr import QuadCost
    idx = np.arange(B65) % 8
    with torch.no_grad():
        return solver(g["nn_C"].shape[0], B65)(gpu(g["nn_x0"][idx]),
                                               QuadCost(gpu(g["nn_C"][:, idx]), gpu(g["nn_c"][:, idx])), dx)


@pytest.fixture(scope="module")
def torch_loop_solution(golden):
    """The torch loop's solve of the tiled problems (the switch off, as shipped), once."""
    from dilqr import generic
    assert generic.DEVICE_MLP_DEEP is False
    return tuple(t.clone() for t in solve65(golden("generic_f32"), seeded_module()))


def test_mpc_device_against_torch_loop(golden, torch_loop_solution, monkeypatch):
    from dilqr import generic
    g = golden("generic_f32")
    dx = seeded_module()
    xt, ut, costs_t = torch_loop_solution
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    x, u, costs = solve65(g, dx)
    per_problem = (cpu(costs) - cpu(costs_t))[:8] / np.maximum(1.0, np.abs(cpu(costs_t)[:8]))
    errs = {"costs": relerr(cpu(costs), cpu(costs_t)), "x": relerr(cpu(x), cpu(xt)), "u": relerr(cpu(u), cpu(ut))}
    print("\n[mlp2 MPC B=65 device vs torch loop] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items())
          + "; per problem cost diff " + " ".join(f"{v:+.1e}" for v in per_problem))
    assert errs["costs"] < 1e-4, errs
    assert max(errs["x"], errs["u"]) < 5e-3, errs
    # lanes are independent: every copy of a problem is the same bits
    first = torch.as_tensor(np.arange(B65) % 8, device=DEV)
    assert torch.equal(x, x[:, first]) and torch.equal(u, u[:, first]) and torch.equal(costs, costs[first])


def test_device_path_really_ran(golden, torch_loop_solution, monkeypatch):
    """The device solve never evaluates the Module; the torch loop must."""
    from dilqr import generic
    from dilqr.dynamics import NNDynamics
    g = golden("generic_f32")
    dx = seeded_module()

    def boom(self, x, u):
        raise AssertionError("NNDynamics.forward called")

    monkeypatch.setattr(NNDynamics, "forward", boom)
    with pytest.raises(AssertionError, match="forward called"):
        solve65(g, dx)
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    x, u, costs = solve65(g, dx)
    assert relerr(cpu(costs), cpu(torch_loop_solution[2])) < 1e-4


def test_backward_reaches_the_weights(golden, monkeypatch):
    """MPC.forward with gradients: the solve on device, the differentiable
    linearisation of the final step on the torch graph (grad_input); every
    gradient against the run with the switch off."""
    from dilqr import QuadCost, generic
    g = golden("generic_f32")
    idx = np.arange(B65) % 8
    T = g["nn_C"].shape[0]
    wx, wu = gpu(g["nn_wx"][:, idx]), gpu(g["nn_wu"][:, idx])

    def run():
        dx = seeded_module()
        X0, C, c = gpu(g["nn_x0"][idx], True), gpu(g["nn_C"][:, idx], True), gpu(g["nn_c"][:, idx], True)
        x, u, costs = solver(T, B65)(X0, QuadCost(C, c), dx)
        ((x * wx).sum() + (u * wu).sum()).backward()
        out = {"dx0": X0.grad, "dC": C.grad, "dc": c.grad}
        for i, fc in enumerate(dx.fcs):
            out[f"dW{i}"], out[f"db{i}"] = fc.weight.grad, fc.bias.grad
        assert all(v is not None for v in out.values())
        return {k: cpu(v) for k, v in out.items()}

    assert generic.DEVICE_MLP_DEEP is False
    ref = run()
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    got = run()
    errs = {k: relerr(got[k], ref[k]) for k in ref}
    print("\n[mlp2 MPC backward, device solve vs torch loop] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert len(errs) == 9 and max(errs.values()) < 5e-3, errs
