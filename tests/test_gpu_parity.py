"""GPU parity: the HIP path (through the C-ABI) against the oracle and the
reference's golden vectors.

Tolerances (fp32 kernels vs fp64 oracle / the reference's fp64 goldens on
identical inputs; every bar is relative to the array's max magnitude):
  * pointwise dynamics / Jacobians:  2e-5 / 5e-5 (atan2/sin/cos ulp differences)
  * Riccati sweeps, pnqp, rollouts, adjoint and implicit gradients: 1e-4 (the
    north-star bar; measured errors are printed, round 4: <= 2.5e-6)
  * MPC solves: by decision replay (check_against_forced_oracle) — the fp64
    oracle made to take the GPU's line-search / best-iterate decisions must
    reproduce its trajectories within 1e-4, and every decision the oracle makes
    differently on its own must be a near-tie (margin < 1e-5)
"""
import numpy as np
import pytest
import torch

from oracle import adjoint as oadj
from oracle import lqr as olqr
from oracle import models as omodels
from oracle import mpc as ompc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def gpu(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dilqr_models():
    from dilqr.env_dx.cartpole import CartpoleDx
    from dilqr.env_dx.pendulum import PendulumDx
    from dilqr.env_dx.rocket import RocketDx
    return {"cartpole": CartpoleDx, "pendulum": PendulumDx, "rocket": RocketDx,
            "pendulum_complex": lambda: PendulumDx(torch.tensor(omodels.PendulumComplex.default_params),
                                                   simple=False)}


# ------------------------------------------------------------------ dynamics
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "rocket"])
def test_dynamics_and_jacobian(golden, name):
    g = golden("models_f64")
    x, u = g[f"{name}_x"], g[f"{name}_u"]
    dx = dilqr_models()[name]()
    out = cpu(dx(gpu(x), gpu(u)))
    D = cpu(dx.get_linear_dyn(gpu(x), gpu(u)))
    assert relerr(out, g[f"{name}_fwd"]) < 2e-5
    assert relerr(D, g[f"{name}_D"]) < 5e-5


def test_pendulum_complex_dynamics_and_jacobian(golden):
    """The 5-parameter pendulum (pendulum.py simple=False) against the
    reference's forward and the autograd Jacobian its AUTO_DIFF path forms."""
    g = golden("complex_f64")
    dx = dilqr_models()["pendulum_complex"]()
    out = cpu(dx(gpu(g["x"]), gpu(g["u"])))
    D = cpu(dx.get_linear_dyn(gpu(g["x"]), gpu(g["u"])))
    e_f, e_d = relerr(out, g["fwd"]), relerr(D, g["jac"])
    print(f"\n[pendulum-complex] forward {e_f:.2e}, Jacobian {e_d:.2e}")
    assert e_f < 2e-5 and e_d < 5e-5


# ------------------------------------------------------------------ Riccati
SHAPES = {"pendulum": (3, 1, 10, 16), "cartpole": (5, 1, 25, 16)}


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("variant", ["", "zI_", "box_"])
def test_riccati_sweep_vs_golden(golden, name, variant):
    from dilqr import ops
    g = golden("riccati_f64")
    n, m, T, B = SHAPES[name]
    C, c, F, u = g[f"{name}_C"], g[f"{name}_c"], g[f"{name}_F"], g[f"{name}_u"]
    kw = {}
    if variant == "zI_":
        kw = dict(u_zero_I=torch.tensor(g[f"{name}_zI"], device=DEV))
    elif variant == "box_":
        kw = dict(u=gpu(u), u_lower=-1.0, u_upper=1.0)     # x=None: c is already c_back
    K, k, _ = ops.lqr_backward(gpu(C), gpu(c), gpu(F), n, m, **kw)
    assert relerr(cpu(K), g[f"{name}_{variant}K"]) < 1e-4
    assert relerr(cpu(k), g[f"{name}_{variant}k"]) < 1e-4


@pytest.mark.parametrize("n,m", [(5, 1), (3, 1), (4, 2)])
@pytest.mark.parametrize("with_x,box", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("T", [1, 9])
def test_sweep_batch_size_independent(n, m, with_x, box, T):
    """Problems are independent in the Riccati sweep (lqr_step_explicit.py:54-162
    is batch-independent): the same problems at B = 128
    (whole waves) and as the first 128 of B = 129 (a partial last wave) give
    bit-identical K, k and pnqp counts.  Every third problem has an asymmetric
    C (the non-SYM step).  (Guards any B-dependent kernel path, such as the
    LDS-DMA-staged sweep that was measured and rejected)"""
    from dilqr import ops
    g = torch.Generator().manual_seed(11)
    d, B0, B1 = n + m, 129, 128
    L = torch.randn(T, B0, d, d, generator=g) * (0.5 / d ** 0.5)
    C = L @ L.transpose(-1, -2) + 0.1 * torch.eye(d)
    C[:, ::3, 0, d - 1] += 0.05
    c = torch.randn(T, B0, d, generator=g)
    F = None
    if T > 1:
        A = torch.eye(n) + 0.05 * torch.randn(T - 1, B0, n, n, generator=g)
        F = torch.cat([A, 0.1 * torch.randn(T - 1, B0, n, m, generator=g)], -1)
    kw = {}
    if with_x:
        kw = dict(x=torch.randn(T, B0, n, generator=g), u=torch.randn(T, B0, m, generator=g))
    bnd = dict(u_lower=-0.5, u_upper=0.5) if box else {}

    def run(Bn):
        sl = lambda t: None if t is None else t[:, :Bn].contiguous().to(DEV)
        return ops.lqr_backward(sl(C), sl(c), sl(F), n, m, want_nqp=True,
                                **{k_: sl(v) for k_, v in kw.items()}, **bnd)
    Ka, ka, qa = run(B1)
    Kb, kb, qb = run(B0)
    assert torch.equal(Ka, Kb[:, :B1]) and torch.equal(ka, kb[:, :B1]) and torch.equal(qa, qb[:B1])
    assert torch.isfinite(Ka).all()


def test_riccati_m3_lindx_shape(golden):
    """(n,m)=(4,3): the m>1 gain solve (pinverse == inverse for SPD Q_uu) and the
    Cholesky+1e-6 engine variant."""
    from dilqr import _native as N
    from dilqr import ops
    g = golden("adjoint_f64")
    C, c, F = g["m3_C"], g["m3_c"], g["m3_F"]
    for solver, ms in ((N.SOLVE_INV, "pinv"), (N.SOLVE_CHOL, "chol")):
        K, k, _ = ops.lqr_backward(gpu(C), gpu(c), gpu(F), 4, 3, m_solver=solver)
        Ko, ko, _ = olqr.lqr_backward(C, c, F, 4, 3, m_solver=ms)
        assert relerr(cpu(K), Ko) < 1e-4 and relerr(cpu(k), ko) < 1e-4


# ------------------------------------------------------------------ one LQR step
@pytest.mark.parametrize("tag,bounds", [("unc", None), ("box", (-5.0, 5.0))])
def test_lqr_step_explicit(golden, tag, bounds):
    """One DiLQR LQR step (Riccati + line search, lqr_step_explicit.py:603-650)
    from the reference's fixture trajectory.  The step's per-problem step
    sizes are replayed in the fp64 oracle (its own choice must agree wherever
    it is not a near-tie): new trajectories within 1e-4 relative, costs 1e-5;
    costs and the batch-mean alpha also against the reference's output."""
    import dilqr
    from dilqr import ops
    from dilqr.env_dx.cartpole import CartpoleDx
    g = golden("lqrstep_f64")
    x0, u, x, F, f = (g[f"{tag}_{k}"] for k in ("x0", "u", "x", "F", "f"))
    T, B, _ = u.shape
    dx = CartpoleDx()
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV)
    c = p.repeat(T, B, 1).to(DEV)
    lo, hi = bounds if bounds else (None, None)
    step = dilqr.LQRStep(5, 1, T, u_lower=lo, u_upper=hi, true_cost=dilqr.QuadCost(C, c), true_dynamics=dx,
                         current_x=gpu(x), current_u=gpu(u), linesearch_decay=0.5, max_linesearch_iter=2)
    nx, nu, nqp, costs, du, malpha = step(gpu(x0), C, c, gpu(F), gpu(f), None)
    # the same step through the functional layer, for its per-problem alphas
    K, k, _ = ops.lqr_backward(C, c, gpu(F), 5, 1, x=gpu(x), u=gpu(u), u_lower=lo, u_upper=hi)
    nx2, nu2, costs2, _, alphas = ops.lqr_forward(dx.model_id, ops.theta_of(dx, C), gpu(x0), C, c, gpu(x), gpu(u),
                                                  K, k, u_lower=lo, u_upper=hi, linesearch_decay=0.5,
                                                  max_linesearch_iter=2)
    assert torch.equal(nu, nu2) and torch.equal(nx, nx2) and torch.equal(costs, costs2)
    M = omodels.Cartpole
    Co, co = ompc.expand_cost(np.diag(M.true_obj()[0]), M.true_obj()[1], T, B)
    Ko, ko, _ = olqr.lqr_backward(Co, olqr.c_back(Co, co, x, u), F, 5, 1, u=u, u_lower=lo, u_upper=hi,
                                  per_problem=True)
    mg = {}
    dyn = lambda xx, uu: M.forward(xx, uu)  # noqa: E731
    xo, uo, cso, *_, ao = olqr.lqr_forward(x0, Co, co, x, u, Ko, ko, dyn, u_lower=lo, u_upper=hi,
                                          linesearch_decay=0.5, max_linesearch_iter=2, margins=mg,
                                          force_alpha=cpu(alphas))
    a_gpu = cpu(alphas)
    dif = np.abs(ao - a_gpu) > 1e-6
    assert np.all(mg.get("linesearch", np.full(B, np.inf))[dif] < 1e-5), np.flatnonzero(dif)
    cerr = np.abs(cpu(costs) - cso) / np.maximum(1.0, np.abs(cso))
    uerr, xerr = relerr(cpu(nu), uo), relerr(cpu(nx), xo)
    gerr = np.abs(cpu(costs) - g[f"{tag}_costs"]) / np.maximum(1.0, np.abs(g[f"{tag}_costs"]))
    print(f"\n[lqrstep {tag}] forced oracle: cost {cerr.max():.2e}, u {uerr:.2e}, x {xerr:.2e}, flips {int(dif.sum())}/"
          f"{B}; vs reference costs {gerr.max():.2e}")
    assert cerr.max() < 1e-5 and uerr < 1e-4 and xerr < 1e-4
    assert gerr.max() < 1e-5
    if not dif.any():
        assert relerr(cpu(nu), g[f"{tag}_nu"]) < 1e-4 and relerr(cpu(du), g[f"{tag}_du"]) < 1e-4
        assert abs(float(malpha) - float(g[f"{tag}_malpha"])) < 1e-6


# ------------------------------------------------------------------ full MPC solves
MPC_CASES = {
    "cart_unc": ("cartpole", 25, 10, None, 0.0, 10 ** 9, 0.5, 2),
    "cart_box10": ("cartpole", 25, 10, (-10.0, 10.0), 0.0, 10 ** 9, 0.5, 2),
    "cart_il": ("cartpole", 25, 40, (-100.0, 100.0), 1e-4, 5, 0.5, 2),
    "pend_unc": ("pendulum", 10, 10, None, 0.0, 10 ** 9, 0.2, 5),
    "pend_box": ("pendulum", 10, 10, (-2.0, 2.0), 0.0, 10 ** 9, 0.2, 5),
    "rocket_unc": ("rocket", 30, 5, None, 0.0, 10 ** 9, 0.2, 5),
}


def device_cost(dx, T, B, cost):
    """The model's true diagonal objective repeated over (t, b), or cost = (C, c)
    ([T,B,d,d], [T,B,d] arrays) as contiguous fp32 device tensors."""
    if cost is None:
        q, p = dx.get_true_obj()
        return torch.diag(q).repeat(T, B, 1, 1).to(DEV).contiguous(), p.repeat(T, B, 1).to(DEV).contiguous()
    return gpu(cost[0]).contiguous(), gpu(cost[1]).contiguous()


def run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls, fused=True, cost=None):
    import dilqr
    from dilqr import ops
    dx = dilqr_models()[mname]()
    B = x0.shape[0]
    C, c = device_cost(dx, T, B, cost)
    lo, hi = bounds if bounds else (None, None)
    if fused:
        m = dilqr.MPC(dx.n_state, dx.n_ctrl, T, u_lower=lo, u_upper=hi, lqr_iter=it, eps=eps,
                      not_improved_lim=nil, linesearch_decay=decay, max_linesearch_iter=mls,
                      exit_unconverged=False, detach_unconverged=False)
        with torch.no_grad():
            x, u, costs = m(gpu(x0), dilqr.QuadCost(C, c), dx)
        return x, u, costs
    ws = ops.mpc_solve_unfused(dx.model_id, ops.theta_of(dx, C), gpu(x0), C, c, T, u_lower=lo, u_upper=hi,
                               lqr_iter=it, eps=eps, linesearch_decay=decay, max_linesearch_iter=mls,
                               not_improved_lim=nil)
    return ws.best_x, ws.best_u, ws.best_cost


def gpu_solve_with_decisions(x0, mname, T, it, bounds, eps, nil, decay, mls, cost=None, flags_out=None):
    """The device-resident solve run one iteration at a time (the stop-rule
    path), recording each iteration's per-problem decisions as the kernels
    took them: the accepted step size (S.alpha) and whether the iterate became
    the best one (S.improved != 0).  Returns best x, u, cost and the decisions
    of the iterations that ran.  cost = (C, c): that cost in place of the
    model's true objective; flags_out (a list): gets the solve's cost_sym [B]."""
    from dilqr import _native as N
    from dilqr import ops
    dx = dilqr_models()[mname]()
    B, n, m = x0.shape[0], dx.n_state, dx.n_ctrl
    C, c = device_cost(dx, T, B, cost)
    x0g = gpu(x0)
    theta = ops.theta_of(dx, x0g)
    lo, hi = bounds if bounds else (None, None)
    bd, _keep = N.make_bounds(lo, hi)
    sv = ops.MPCSolve(T, B, n, m, DEV)
    sv.begin(dx.model_id, theta, x0g)
    alphas, takes = [], []
    for i in range(it):
        sv.iterate(dx.model_id, theta, x0g, C, c, bd, decay, mls, i, 1e-4, eps, nil)
        alphas.append(cpu(sv.alpha))
        takes.append(cpu(sv.improved) != 0)
    ran = sv.iterations if sv.stopped else it
    x, u = sv.gather_best()
    if flags_out is not None:
        flags_out.append(cpu(sv.cost_sym).astype(int))
    return x, u, sv.best_cost.clone(), alphas[:ran], takes[:ran]


def check_against_forced_oracle(M, x0, T, bounds, decay, mls, x, u, costs, alphas, takes, label,
                                cost_tol=1e-5, traj_tol=1e-4, tie=1e-5, ref_spread=None, cost=None, detail=None):
    """Parity by decision replay.  (1) The fp64 oracle, made to take the GPU's
    decisions (its step sizes and best-iterate updates, oracle/mpc.py `force`),
    must reproduce the GPU's best trajectories and costs: what remains is fp32
    arithmetic, held to traj_tol relative (north star 1e-4) and cost_tol.
    (2) At every iteration, from that same state, the oracle's OWN decision
    must equal the GPU's unless the decision is a near-tie (its margin below
    `tie`: |cost_p - old| / |old| for a step size, |cost - (best + eps)| / |best|
    for the best-iterate test), where fp32 and fp64 may legitimately differ.
    Prints the measured errors and the count of near-tie flips.
    ref_spread (per problem, optional): the reference's own fp32-vs-fp64 cost
    difference on the same problem; a problem whose cost the reference itself
    cannot hold to cost_tol in fp32 is held to 3x that spread instead.
    cost = (C, c): that cost in place of the model's true objective.
    detail (a dict): gets the per-problem errors (cost [B]; u, x [B], each
    relative to the batch's max magnitude, as the assertions) and flip counts."""
    B = x0.shape[0]
    if cost is None:
        q, p = M.true_obj()
        Co, co = ompc.expand_cost(np.diag(q), p, T, B)
    else:
        Co, co = (np.asarray(a, np.float64) for a in cost)
    lo, hi = bounds if bounds else (None, None)
    trace = []
    xo, uo, cso, _ = ompc.mpc_forward(M, x0, Co, co, T, u_lower=lo, u_upper=hi, lqr_iter=len(alphas), eps=0.0,
                                      not_improved_lim=10 ** 9, linesearch_decay=decay, max_linesearch_iter=mls,
                                      per_problem=True, trace=trace,
                                      force=lambda i: (alphas[i].astype(np.float64), takes[i]))
    cerr = np.abs(cpu(costs) - cso) / np.maximum(1.0, np.abs(cso))
    uerr = np.abs(cpu(u) - uo).max() / max(1.0, np.abs(uo).max())
    xerr = np.abs(cpu(x) - xo).max() / max(1.0, np.abs(xo).max())
    flips = total = 0
    for i, tr in enumerate(trace):
        dif_a = np.abs(tr["alpha_free"] - alphas[i]) > 1e-6 * np.maximum(1.0, tr["alpha_free"])
        dif_t = tr["take_free"] != takes[i]
        total += 2 * B
        flips += int(dif_a.sum() + dif_t.sum())
        assert np.all(tr["ls_margin"][dif_a] < tie), (label, i, np.flatnonzero(dif_a), tr["ls_margin"][dif_a])
        assert np.all(tr["best_margin"][dif_t] < tie), (label, i, np.flatnonzero(dif_t), tr["best_margin"][dif_t])
    print(f"\n[{label}] forced-decision oracle: max rel cost err {cerr.max():.2e}, u {uerr:.2e}, x {xerr:.2e}; "
          f"near-tie decision flips {flips}/{total}")
    if detail is not None:
        detail.update(cost=cerr, u=np.abs(cpu(u) - uo).max(axis=(0, 2)) / max(1.0, np.abs(uo).max()),
                      x=np.abs(cpu(x) - xo).max(axis=(0, 2)) / max(1.0, np.abs(xo).max()), flips=flips, total=total)
    tol = np.full(B, cost_tol) if ref_spread is None else np.maximum(cost_tol, 3 * ref_spread)
    wide = np.flatnonzero(tol > cost_tol)
    if wide.size:
        print(f"[{label}] problems {wide} held to 3x the reference's own fp32 spread "
              f"{ref_spread[wide]}: errors {cerr[wide]}")
    assert np.all(cerr < tol), (np.flatnonzero(cerr >= tol), cerr.max())
    assert uerr < traj_tol and xerr < traj_tol, (uerr, xerr)
    return cso


@pytest.mark.parametrize("name", list(MPC_CASES))
def test_mpc_solve_vs_oracle(golden, name):
    """Full device-resident MPC solves (fused iteration + stop rule) against the
    fp64 oracle by decision replay (check_against_forced_oracle: trajectories
    within 1e-4 relative, costs within 1e-5, every differing decision a
    near-tie), and the costs against the reference's own fp64 solve (golden;
    its pnqp couples the batch, SURVEY.md §4 item 4: noise floor ~5e-6)."""
    g = golden("mpc_f64")
    mname, T, it, bounds, eps, nil, decay, mls = MPC_CASES[name]
    x0 = g[f"{name}_x0"]
    x, u, costs, alphas, takes = gpu_solve_with_decisions(x0, mname, T, it, bounds, eps, nil, decay, mls)
    # the same solve through the public API is the same computation
    x2, u2, costs2 = run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls)
    assert same_bits(x, x2) and same_bits(u, u2) and same_bits(costs, costs2)
    ref = g[f"{name}_costs"]
    # the reference's own fp32 solve of the same problems (B=64): its distance
    # from the fp64 solve measures each problem's fp32 conditioning (cart_box10
    # problem 32: 1.45e-4; every other problem of every case: <= 4.3e-6)
    spread = np.abs(golden("mpc_f32")[f"{name}_costs"] - ref) / np.maximum(1.0, np.abs(ref))
    check_against_forced_oracle(omodels.MODELS[mname], x0, T, bounds, decay, mls, x, u, costs, alphas, takes, name,
                                ref_spread=spread)
    rerr = np.abs(cpu(costs) - ref) / np.maximum(1.0, np.abs(ref))
    print(f"[{name}] vs the reference's fp64 costs: max rel {rerr.max():.2e}, median {np.median(rerr):.2e}")
    assert np.all(rerr < np.maximum(1e-4, 3 * spread)), (np.flatnonzero(rerr >= 1e-4), rerr.max())


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["cart_unc", "cart_box10", "pend_box"])
def test_mpc_iterates_vs_golden(golden, name, k):
    """The solve stopped after k = 1, 2, 3 iterations (lqr_iter = k) against the
    reference's own fp64 solves with the same lqr_iter (gen_golden.py
    MPC_ITERATE_CASES): the per-iteration path of mpc_explicit.py:228-299, not
    only its end point.  Costs within max(1e-4, 3x the reference's own
    fp32-vs-fp64 spread) relative, as test_mpc_solve_vs_oracle."""
    g = golden("mpc_f64")
    mname, T, it, bounds, eps, nil, decay, mls = MPC_CASES[name]
    x0 = g[f"{name}_x0"]
    _, _, costs = run_gpu_mpc(x0, mname, T, k, bounds, eps, nil, decay, mls)
    ref = g[f"{name}_it{k}_costs"]
    spread = np.abs(golden("mpc_f32")[f"{name}_it{k}_costs"] - ref) / np.maximum(1.0, np.abs(ref))
    rerr = np.abs(cpu(costs) - ref) / np.maximum(1.0, np.abs(ref))
    print(f"[{name} k={k}] max rel {rerr.max():.2e}, reference fp32 spread max {spread.max():.2e}")
    assert np.all(rerr < np.maximum(1e-4, 3 * spread)), (np.flatnonzero(rerr >= 1e-4), rerr.max())


COMPLEX_MPC = {"fixed": (20, 10, 0.0, 10 ** 9), "il": (20, 40, 1e-3, 5)}     # T, lqr_iter, eps, not_improved_lim


@pytest.mark.parametrize("name", list(COMPLEX_MPC))
def test_pendulum_complex_mpc_vs_golden(golden, name):
    """MPC solves of the 5-parameter pendulum (bounds +-2, decay 0.2, max_ls 5,
    the IL settings of pendulum.py:52-58) on the fused HIP iteration: by
    decision replay against the fp64 oracle, and against the reference's own
    fp64 solve (mpc_explicit.MPC with GradMethods.AUTO_DIFF, the path that runs
    for this model).  dilqr.MPC takes the same kernels with ANALYTIC and with
    AUTO_DIFF (its Jacobian is the autograd one): identical bits."""
    import dilqr
    g = golden("complex_f64")
    T, it, eps, nil = COMPLEX_MPC[name]
    x0 = g[f"{name}_x0"]
    x, u, costs, alphas, takes = gpu_solve_with_decisions(x0, "pendulum_complex", T, it, (-2.0, 2.0), eps, nil,
                                                          0.2, 5)
    x2, u2, c2 = run_gpu_mpc(x0, "pendulum_complex", T, it, (-2.0, 2.0), eps, nil, 0.2, 5)
    assert same_bits(x, x2) and same_bits(u, u2) and same_bits(costs, c2)
    dx = dilqr_models()["pendulum_complex"]()
    q, p = dx.get_true_obj()
    B = x0.shape[0]
    m = dilqr.MPC(3, 1, T, u_lower=-2.0, u_upper=2.0, lqr_iter=it, eps=eps, not_improved_lim=nil,
                  linesearch_decay=0.2, max_linesearch_iter=5, exit_unconverged=False, detach_unconverged=False,
                  grad_method=dilqr.GradMethods.AUTO_DIFF)
    with torch.no_grad():
        x3, u3, c3 = m(gpu(x0), dilqr.QuadCost(torch.diag(q).repeat(T, B, 1, 1).to(DEV), p.repeat(T, B, 1).to(DEV)),
                       dx)
    assert same_bits(u, u3) and same_bits(costs, c3)
    check_against_forced_oracle(omodels.PendulumComplex, x0, T, (-2.0, 2.0), 0.2, 5, x, u, costs, alphas, takes,
                                f"complex_{name}")
    ref = g[f"{name}_costs"]
    rerr = np.abs(cpu(costs) - ref) / np.maximum(1.0, np.abs(ref))
    print(f"[complex_{name}] vs the reference's fp64 costs: max rel {rerr.max():.2e}")
    assert np.max(rerr) < 1e-4, np.max(rerr)


def test_pendulum_complex_backward_refused():
    """No implicit backward for the 5-parameter pendulum (the reference's
    grad_input has no 5-parameter form, pendulum.py:157): a solve whose inputs
    carry gradients solves, and its backward raises instead of returning
    silently wrong gradients."""
    import dilqr
    dx = dilqr_models()["pendulum_complex"]()
    dx.params = dx.params.clone().to(DEV).requires_grad_(True)
    T, B = 5, 4
    q, p = dx.get_true_obj()
    m = dilqr.MPC(3, 1, T, u_lower=-2.0, u_upper=2.0, lqr_iter=3, exit_unconverged=False,
                  detach_unconverged=False)
    x, u, _ = m(gpu(np.tile([1.0, 0.0, 0.0], (B, 1))),
                dilqr.QuadCost(torch.diag(q).repeat(T, B, 1, 1).to(DEV), p.repeat(T, B, 1).to(DEV)), dx)
    with pytest.raises(NotImplementedError, match="5-parameter"):
        u.sum().backward()


def same_bits(a, b):
    """Equal element for element, NaN matching NaN (a diverged problem is NaN on
    both sides; its payload is not compared)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, 0.0, a), torch.where(nb, 0.0, b))


@pytest.mark.parametrize("name", ["cart_unc", "cart_box10", "cart_il", "pend_box"])
def test_fused_iteration_equals_unfused(golden, name):
    """The fused iteration kernel (F computed on the fly, never stored) gives the
    same iterates, bit for bit, as the unfused linearize -> Riccati -> rollout
    pipeline.  For cartpole this also pins the fused sweep's Jacobian shortcut:
    it takes cos/sin of the integrated angle from the rollout's x_{t+1}
    (Cartpole::jacobian_next) where the unfused k_linearize recomputes atan2,
    cos and sin (Cartpole::jacobian) — equal only while every slot trajectory
    is exactly forward(x_t, u_t), the invariant stated at dilqr_mpc_state."""
    g = golden("mpc_f64")
    mname, T, it, bounds, eps, nil, decay, mls = MPC_CASES[name]
    x0 = g[f"{name}_x0"]
    a = run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls, fused=True)
    b = run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls, fused=False)
    for ta, tb in zip(a, b):
        assert same_bits(ta, tb), relerr(cpu(ta), cpu(tb))


# ------------------------------------------------------------------ classic adjoint
@pytest.mark.parametrize("mname", ["pendulum", "cartpole"])
def test_packed_cost_paths_bit_identical(mname):
    """The solve's packed cost copy (diagonal / symmetric / none, each possibly
    time-invariant, chosen per problem by iteration 0) changes only what is
    read, never the arithmetic: a batch mixing time-invariant diagonal,
    diagonal, time-invariant dense, dense symmetric and asymmetric C gives
    bit-identical trajectories and costs with and without the packed copy."""
    from dilqr import _native as N
    from dilqr import ops
    dx = dilqr_models()[mname]()
    n, m, T, B = dx.n_state, dx.n_ctrl, 12, 256
    d = n + m
    g = torch.Generator().manual_seed(3)
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1)
    L = torch.randn(T, B // 2, d, d, generator=g) * (0.3 / d ** 0.5)
    C[:, B // 2:] = C[:, B // 2:] + L @ L.transpose(-1, -2)                       # dense symmetric
    C[:, 3 * B // 4:, 0, 1] += 1e-3                                               # asymmetric
    c = p.repeat(T, B, 1) + 0.01 * torch.randn(T, B, d, generator=g)
    c[:, :B // 4] = c[0, :B // 4]                                                 # time-invariant diagonal
    C[:, B // 2:5 * B // 8] = C[0, B // 2:5 * B // 8]                             # time-invariant dense
    c[:, B // 2:5 * B // 8] = c[0, B // 2:5 * B // 8]
    C, c = C.to(DEV).contiguous(), c.to(DEV).contiguous()
    rng = np.random.RandomState(0)
    if mname == "pendulum":
        th = rng.uniform(-np.pi / 2, np.pi / 2, B)
        x0 = np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, B)], 1)
    else:
        th = rng.uniform(-np.pi, np.pi, B)
        x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                       rng.uniform(-1, 1, B)], 1)
    # diverged problems: an infinite state in a diagonal, a dense and an
    # asymmetric cost problem (NaN costs on every path, see nonfinite_probe)
    x0[[5, B // 2 + 7, 3 * B // 4 + 2], 0] = np.inf
    x0 = gpu(x0)
    theta = ops.theta_of(dx, x0)
    nb, _ = N.make_bounds(None, None)
    out = []
    for packed in (True, False):
        sv = ops.MPCSolve(T, B, n, m, DEV, packed_cost=packed)
        sv.begin(dx.model_id, theta, x0)
        for i in range(6):
            sv.iterate(dx.model_id, theta, x0, C, c, nb, 0.5, 4, i, 1e-4, 0.0, 10 ** 9)
        x, u = sv.gather_best()
        out.append((x, u, sv.best_cost.clone()))
        if packed:
            flags = cpu(sv.cost_sym)
            assert (flags[:B // 4] == 7).all() and (flags[B // 4:B // 2] == 3).all()
            assert (flags[B // 2:5 * B // 8] == 5).all() and (flags[5 * B // 8:3 * B // 4] == 1).all()
            assert (flags[3 * B // 4:] == 0).all()
    for a, b in zip(*out):
        assert same_bits(a, b)
    assert torch.isnan(out[0][2][[5, B // 2 + 7, 3 * B // 4 + 2]]).all()


@pytest.mark.parametrize("tag,bounds", [("m1", None), ("m3", None), ("m1box", (-0.5, 0.5)),
                                        ("m3box", (-0.5, 0.5))])
def test_classic_adjoint_vs_golden(golden, tag, bounds):
    from dilqr import mpc as cmpc
    from dilqr.definitions import LinDx, QuadCost
    g = golden("adjoint_f64")
    C, c, F, f, x0 = (g[f"{tag}_{k}"] for k in ("C", "c", "F", "f", "x0"))
    T, B, d = c.shape
    n = x0.shape[1]
    m = d - n
    Ct, ct, Ft, ft, x0t = (gpu(a).requires_grad_(True) for a in (C, c, F, f, x0))
    lo, hi = bounds if bounds else (None, None)
    mpc_ = cmpc.MPC(n, m, T, u_lower=lo, u_upper=hi, lqr_iter=1, n_batch=B, detach_unconverged=False,
                    exit_unconverged=False, verbose=-1)
    x, u, _ = mpc_(x0t, QuadCost(Ct, ct), LinDx(Ft, ft))
    assert relerr(cpu(x), g[f"{tag}_x"]) < 1e-4 and relerr(cpu(u), g[f"{tag}_u"]) < 1e-4
    loss = (x * gpu(g[f"{tag}_wx"])).sum() + (u * gpu(g[f"{tag}_wu"])).sum()
    loss.backward()
    # the adjoint kernel alone: the oracle's backward at the GPU's own solution
    xg, ug = cpu(x), cpu(u)
    od = oadj.classic_backward(g[f"{tag}_wx"], g[f"{tag}_wu"], x0, C, c, F, f, xg, ug, lo, hi)
    e_own = {k: relerr(cpu(t.grad), o) for (k, t), o in zip((("dx0", x0t), ("dC", Ct), ("dc", ct), ("dF", Ft),
                                                             ("df", ft)), od)}
    e_ref = {k: relerr(cpu(t.grad), g[f"{tag}_{k}"]) for k, t in (("dx0", x0t), ("dC", Ct), ("dc", ct),
                                                                   ("dF", Ft), ("df", ft))}
    print(f"\n[classic adjoint {tag}] x {relerr(xg, g[f'{tag}_x']):.2e} u {relerr(ug, g[f'{tag}_u']):.2e}; "
          f"at the GPU solution: " + ", ".join(f"{k} {v:.2e}" for k, v in e_own.items()) +
          "; vs the golden: " + ", ".join(f"{k} {v:.2e}" for k, v in e_ref.items()))
    # measured (round 4): <= 2.5e-7 at the GPU's solution, <= 7.2e-7 against the golden
    assert max(e_own.values()) < 1e-5, e_own
    assert max(e_ref.values()) < 1e-4, e_ref


# ------------------------------------------------------------------ the reference's datasets
def test_dataset_cartpole_known_answer(golden):
    """data/cartpole.pkl expert trajectories (made by the reference solver, fp32)."""
    g = golden("datasets")
    tau = np.concatenate([g["cartpole_train_data"], g["cartpole_val_data"], g["cartpole_test_data"]])
    T = int(g["cartpole_mpc_T"])
    x0 = tau[:, 0, :5]
    x, u, _ = run_gpu_mpc(x0, "cartpole", T, int(g["cartpole_lqr_iter"]),
                          (float(g["cartpole_lower"]), float(g["cartpole_upper"])), float(g["cartpole_mpc_eps"]),
                          5, float(g["cartpole_linesearch_decay"]), int(g["cartpole_max_linesearch_iter"]))
    got = np.concatenate([cpu(x), cpu(u)], 2).transpose(1, 0, 2)
    print(f"\n[dataset cartpole] max |got - reference| {np.max(np.abs(got - tau)):.2e}")
    # the reference reproduces this dataset bit for bit; the fp32
    # GPU solve (other summation orders, v_rcp gains) is measured at 9.3e-6
    assert np.max(np.abs(got - tau)) < 1e-4


def test_dataset_pendulum_known_answer(golden):
    """data/pendulum.pkl: 120 expert trajectories, T=20, lqr_iter=500, bounds +-2."""
    g = golden("datasets")
    tau = np.concatenate([g["pendulum_train_data"], g["pendulum_val_data"], g["pendulum_test_data"]])
    T = int(g["pendulum_mpc_T"])
    x0 = tau[:, 0, :3]
    x, u, _ = run_gpu_mpc(x0, "pendulum", T, int(g["pendulum_lqr_iter"]),
                          (float(g["pendulum_lower"]), float(g["pendulum_upper"])), float(g["pendulum_mpc_eps"]),
                          5, float(g["pendulum_linesearch_decay"]), int(g["pendulum_max_linesearch_iter"]))
    got = np.concatenate([cpu(x), cpu(u)], 2).transpose(1, 0, 2)
    err = np.abs(got - tau).max(axis=(1, 2))
    print(f"\n[dataset pendulum] per-trajectory max err: median {np.median(err):.2e}, 99% {np.quantile(err, .99):.2e}, "
          f"max {err.max():.2e}, within 1e-4: {np.mean(err < 1e-4):.3f}")
    # the reference reproduces its own dataset only to 7e-4 (500
    # iterations with eps 1e-3 on saturated controls); measured here: median
    # 1.2e-6, 91% of trajectories within 1e-4, max 3.7e-4
    assert np.median(err) < 1e-5 and np.mean(err < 1e-4) >= 0.85 and err.max() < 1e-3, \
        (np.median(err), np.mean(err < 1e-4), err.max())


# ------------------------------------------------------------------ full-size properties
def test_full_size_batch_independence():
    """Config 2 shape (cartpole T=25, B=65536): problems are independent, so
    solving a 256-problem slice alone gives bit-identical iterates."""
    B, T = 65536, 25
    rng = np.random.RandomState(0)
    th = rng.uniform(-np.pi, np.pi, B)
    x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                   rng.uniform(-1, 1, B)], 1)
    full = run_gpu_mpc(x0, "cartpole", T, 3, None, 0.0, 10 ** 9, 0.5, 2)
    part = run_gpu_mpc(x0[4096:4352], "cartpole", T, 3, None, 0.0, 10 ** 9, 0.5, 2)
    assert torch.equal(full[1][:, 4096:4352], part[1])
    assert torch.equal(full[2][4096:4352], part[2])
    assert torch.isfinite(full[2]).all()


@pytest.mark.parametrize("bounds", [None, (-10.0, 10.0)])
def test_max_batch_one_gpu(bounds):
    """Config 5's whole batch (B = 524 288, 8x a GPU's shard) on one GPU, the
    solve and the implicit backward: the last 256 problems (the highest record
    offsets, where a 32-bit index would wrap first) solved alone give the same
    iterates and gradients bit for bit."""
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    B, T, S = 524288, 25, 256
    rng = np.random.RandomState(3)
    th = rng.uniform(-np.pi, np.pi, B)
    x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                   rng.uniform(-1, 1, B)], 1)
    full = run_gpu_mpc(x0, "cartpole", T, 3, bounds, 0.0, 10 ** 9, 0.5, 2)
    part = run_gpu_mpc(x0[B - S:], "cartpole", T, 3, bounds, 0.0, 10 ** 9, 0.5, 2)
    assert torch.equal(full[1][:, B - S:], part[1]) and torch.equal(full[2][B - S:], part[2])
    assert torch.isfinite(full[2]).all()
    dx = dilqr_models()["cartpole"]()
    q, p = dx.get_true_obj()
    lo, hi = bounds if bounds else (None, None)
    g = torch.Generator(device=DEV).manual_seed(4)
    wx = torch.randn(T, B, 5, device=DEV, generator=g)
    wu = torch.randn(T, B, 1, device=DEV, generator=g)
    out = []
    for sl in (slice(0, B), slice(B - S, B)):
        Bs = sl.stop - sl.start
        C = torch.diag(q).repeat(T, Bs, 1, 1).to(DEV)
        c = p.repeat(T, Bs, 1).to(DEV)
        x, u = full[0][:, sl].contiguous(), full[1][:, sl].contiguous()
        F = ops.linearize(dx.model_id, ops.theta_of(dx, C), x, u)[0]
        K, _, _ = ops.lqr_backward(C, c, F, 5, 1, x=x, u=u, u_lower=lo, u_upper=hi)
        out.append(implicit_backward(dx, wx[:, sl].contiguous(), wu[:, sl].contiguous(), C, c, None, None, x, u, K,
                                     lo, hi, None))
        del C, c, F
    (dC, dc, dth), (dC2, dc2, dth2) = out
    assert torch.equal(dth[B - S:], dth2) and torch.equal(dC[:, B - S:], dC2) and torch.equal(dc[:, B - S:], dc2)
    assert torch.isfinite(dth).all()


@pytest.mark.parametrize("name", ["cart_unc", "cart_box10", "pend_box", "rocket_unc"])
def test_fixed_count_solve_equals_stop_rule_path(golden, name):
    """A solve whose stop rule cannot fire (eps <= 0, not_improved_lim >= the
    iteration count) runs as a fixed-count solve: one launch per iteration and
    best_du formed at the end (dilqr_mpc_iterate_fixed_f32 / finish).  Best
    trajectories, best costs and best_du equal, bit for bit, those of the
    per-iteration stop-rule path on the same problems."""
    from dilqr import _native as N
    from dilqr import ops
    g = golden("mpc_f64")
    mname, T, it, bounds, _eps, _nil, decay, mls = MPC_CASES[name]
    dx = dilqr_models()[mname]()
    x0 = gpu(g[f"{name}_x0"])
    B, n, m = x0.shape[0], dx.n_state, dx.n_ctrl
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV).contiguous()
    c = p.repeat(T, B, 1).to(DEV).contiguous()
    theta = ops.theta_of(dx, x0)
    lo, hi = bounds if bounds else (None, None)
    bd, _keep = N.make_bounds(lo, hi)
    a = ops.MPCSolve(T, B, n, m, x0.device)
    a.begin(dx.model_id, theta, x0)
    for i in range(it):
        a.iterate(dx.model_id, theta, x0, C, c, bd, decay, mls, i, 1e-4, 0.0, 10 ** 9)
    xa, ua = a.gather_best()
    xb, ub, cost_b, du_b, sv = ops.mpc_solve(dx.model_id, theta, x0, C, c, T, u_lower=lo, u_upper=hi, lqr_iter=it,
                                             eps=0.0, linesearch_decay=decay, max_linesearch_iter=mls,
                                             not_improved_lim=10 ** 9)
    assert sv.fixed_iters == it and sv.iterations == it
    assert torch.equal(xa, xb) and torch.equal(ua, ub)
    assert torch.equal(a.best_cost, cost_b) and torch.equal(a.best_du, du_b)
    assert torch.isfinite(du_b).all()
    # full_du_norm: the last iteration's quirk rows on both paths
    assert torch.equal(a.full_du_norm, sv.full_du_norm)


@pytest.mark.parametrize("mname", ["cartpole", "pendulum"])
def test_tensor_bounds_whole_solve(golden, mname):
    """Per-(t,b) bounds ([T,B,m] tensors, mpc_explicit.py:186-201) through the
    whole-solve launch: equal to scalar bounds when every entry equals them
    (bit for bit), and per-(t,b) random bounds equal the unfused pipeline
    (linearise -> Riccati+pnqp -> line search kernels) bit for bit."""
    from dilqr import ops
    g = golden("mpc_f64")
    name = "cart_box10" if mname == "cartpole" else "pend_box"
    _m, T, it, (lo, hi), _eps, _nil, decay, mls = MPC_CASES[name]
    dx = dilqr_models()[mname]()
    x0 = gpu(g[f"{name}_x0"])
    B, m = x0.shape[0], dx.n_ctrl
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV).contiguous()
    c = p.repeat(T, B, 1).to(DEV).contiguous()
    theta = ops.theta_of(dx, x0)
    kw = dict(lqr_iter=it, eps=0.0, linesearch_decay=decay, max_linesearch_iter=mls, not_improved_lim=10 ** 9)
    xs, us, cs, *_ = ops.mpc_solve(dx.model_id, theta, x0, C, c, T, u_lower=lo, u_upper=hi, **kw)
    lo_t = torch.full((T, B, m), lo, device=DEV)
    hi_t = torch.full((T, B, m), hi, device=DEV)
    xt, ut, ct, *_ = ops.mpc_solve(dx.model_id, theta, x0, C, c, T, u_lower=lo_t, u_upper=hi_t, **kw)
    assert same_bits(xs, xt) and same_bits(us, ut) and same_bits(cs, ct)
    gen = torch.Generator().manual_seed(11)
    lo_r = (lo * (0.3 + 0.7 * torch.rand(T, B, m, generator=gen))).to(DEV)
    hi_r = (hi * (0.3 + 0.7 * torch.rand(T, B, m, generator=gen))).to(DEV)
    xf, uf, cf, *_ = ops.mpc_solve(dx.model_id, theta, x0, C, c, T, u_lower=lo_r, u_upper=hi_r, **kw)
    ws = ops.mpc_solve_unfused(dx.model_id, theta, x0, C, c, T, u_lower=lo_r, u_upper=hi_r, **kw)
    assert same_bits(xf, ws.best_x) and same_bits(uf, ws.best_u) and same_bits(cf, ws.best_cost)
    assert bool(((uf >= lo_r) & (uf <= hi_r)).all())
    assert not same_bits(uf, us)                       # the per-(t,b) bounds took effect


@pytest.mark.parametrize("T,B,bounds", [(48, 100, None), (40, 77, (-10.0, 10.0)), (3, 130, None)])
def test_whole_solve_hbm_gains_and_ragged_batch(T, B, bounds):
    """The whole-solve launch off the headline shape: T = 48 puts the gain
    records in HBM (74 KB per workgroup: over the 64 KiB a launch takes
    without opting in), T = 40 keeps them in LDS only because the small grid
    fits the chip in one round (61 KB per workgroup, more than four per CU
    allow), B not a multiple of 64 leaves idle lanes in the last wave, T = 3 is
    nearly all peeled steps — each bit-identical to the per-iteration launches,
    with and without bounds."""
    from dilqr import _native as N
    from dilqr import ops
    from dilqr.env_dx.cartpole import CartpoleDx
    dx = CartpoleDx()
    rng = np.random.RandomState(T * 1000 + B)
    th = rng.uniform(-np.pi, np.pi, B)
    x0 = gpu(np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                       rng.uniform(-1, 1, B)], 1))
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV).contiguous()
    c = p.repeat(T, B, 1).to(DEV).contiguous()
    theta = ops.theta_of(dx, x0)
    lo, hi = bounds if bounds else (None, None)
    bd, _keep = N.make_bounds(lo, hi)
    it = 6
    a = ops.MPCSolve(T, B, 5, 1, x0.device, fixed_iters=it)
    a.begin(dx.model_id, theta, x0)
    for i in range(it):
        a.iterate_fixed(dx.model_id, theta, x0, C, c, bd, 0.5, 2, i, 1e-4)
    a.finish_fixed(it)
    b = ops.MPCSolve(T, B, 5, 1, x0.device, fixed_iters=it)
    b.solve_fixed(dx.model_id, theta, x0, C, c, bd, 0.5, 2, 1e-4)
    for key in ("slot", "cost", "alpha", "improved", "best_cost", "best_du", "full_du_norm", "best_iter"):
        assert same_bits(getattr(a, key).float(), getattr(b, key).float()), key
    xa, ua = a.gather_best()
    xb, ub = b.gather_best()
    assert torch.equal(xa, xb) and torch.equal(ua, ub)
    assert torch.isfinite(b.best_cost).all()


@pytest.mark.parametrize("name,warm", [("cart_unc", False), ("cart_box10", True), ("pend_box", False),
                                       ("pend_unc", True), ("rocket_unc", False)])
def test_whole_solve_launch_equals_per_iteration_launches(golden, name, warm):
    """dilqr_mpc_solve_fixed_f32 (begin + every iteration in ONE launch for the
    single-lane models, each lane iterating its own problem) leaves exactly the
    state of begin + one iterate_fixed launch per iteration + finish_fixed:
    slots, costs, step sizes, improved flags, best iterate, best_iter, best_du,
    full_du_norm — bit for bit, with and without a warm start u_init."""
    from dilqr import _native as N
    from dilqr import ops
    g = golden("mpc_f64")
    mname, T, it, bounds, _eps, _nil, decay, mls = MPC_CASES[name]
    dx = dilqr_models()[mname]()
    x0 = gpu(g[f"{name}_x0"])
    B, n, m = x0.shape[0], dx.n_state, dx.n_ctrl
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV).contiguous()
    c = p.repeat(T, B, 1).to(DEV).contiguous()
    theta = ops.theta_of(dx, x0)
    lo, hi = bounds if bounds else (None, None)
    bd, _keep = N.make_bounds(lo, hi)
    u0 = 0.3 * torch.randn(T, B, m, generator=torch.Generator().manual_seed(5)).to(DEV) if warm else None
    a = ops.MPCSolve(T, B, n, m, x0.device, fixed_iters=it)
    a.begin(dx.model_id, theta, x0, u0)
    for i in range(it):
        a.iterate_fixed(dx.model_id, theta, x0, C, c, bd, decay, mls, i, 1e-4)
    a.finish_fixed(it)
    b = ops.MPCSolve(T, B, n, m, x0.device, fixed_iters=it)
    b.solve_fixed(dx.model_id, theta, x0, C, c, bd, decay, mls, 1e-4, u0)
    for key in ("slot", "cost", "alpha", "improved", "best_cost", "best_du", "full_du_norm", "best_iter"):
        assert same_bits(getattr(a, key).float(), getattr(b, key).float()), key
    xa, ua = a.gather_best()
    xb, ub = b.gather_best()
    assert torch.equal(xa, xb) and torch.equal(ua, ub)
    assert a.iterations == b.iterations == it


# ------------------------------------------------------------------ DiLQR implicit backward
IMPLICIT = {"cart_unc": ("cartpole", None), "cart_box": ("cartpole", (-5.0, 5.0)),
            "pend_box": ("pendulum", (-2.0, 2.0)), "rock_unc": ("rocket", None),
            "rock_box": ("rocket", (-10.0, 10.0)),
            # config 4's own horizon, cartpole T=25, B=8 (gen_golden.py IMPLICIT25_CASES)
            "cart25_unc": ("cartpole", None), "cart25_box10": ("cartpole", (-10.0, 10.0)),
            "cart25_box100": ("cartpole", (-100.0, 100.0))}


def implicit_file(tag, prec="f64"):
    return f"implicit25_{prec}" if tag.startswith("cart25") else f"implicit_{prec}"


@pytest.mark.parametrize("tag,prec", [(t, "f64") for t in IMPLICIT] +
                         [(t, "f32") for t in IMPLICIT if t.startswith("cart25")])
def test_implicit_backward_vs_golden(golden, tag, prec):
    """LQRStep(no_op_forward=True) at the reference's solution; backward
    through the fused implicit kernel vs the reference's dC, dc, dtheta.
    Tolerance 1e-4 of the max magnitude (the reference's own fp32 result is
    within ~3e-5 of its fp64 result, see tests/golden).  The T=25 cases are
    also checked against the reference's own fp32 run (its fp32 MPC solution
    and fp32 gradients, lqr_step_explicit.py:653-712).  There dtheta (from
    torch.linalg.solve, :570) is always compared; dC and dc come from the
    reference's fp32 lstsq on the 150x150 KKT matrix (:578, :585), which for the
    unconstrained T=25 problems departs from the reference's OWN fp64 result by
    0.98 (dC) and 0.74 (dc) of the max magnitude (the box-10 case: 1e-5) — so
    the fp32 dC, dc goldens are compared only where the reference's fp32 agrees
    with its fp64 to 1e-4 (the fp64 cases hold dC, dc for every tag)."""
    import dilqr
    g = golden(implicit_file(tag, prec))
    g64 = golden(implicit_file(tag, "f64"))
    mname, bounds = IMPLICIT[tag]
    dx = dilqr_models()[mname]()
    x, u, Q, P, F, f, x0 = (gpu(g[f"{tag}_{k}"]) for k in ("x", "u", "Q", "P", "F", "f", "x0"))
    T, B, n = x.shape
    m = u.shape[2]
    theta = dx.params.clone().to(DEV).requires_grad_(True)
    Qg, Pg = Q.clone().requires_grad_(True), P.clone().requires_grad_(True)
    lo, hi = bounds if bounds else (None, None)
    step = dilqr.LQRStep(n, m, T, u_lower=lo, u_upper=hi, true_cost=dilqr.QuadCost(Qg, Pg), true_dynamics=dx,
                         current_x=x, current_u=u, no_op_forward=True)
    x2, u2 = step(x0, Qg, Pg, F, f, theta)
    loss = (x2 * gpu(g[f"{tag}_wx"])).sum() + (u2 * gpu(g[f"{tag}_wu"])).sum()
    loss.backward()
    assert relerr(cpu(theta.grad), g[f"{tag}_dtheta"]) < 1e-4
    ref_self = max(relerr(g[f"{tag}_dQ"], g64[f"{tag}_dQ"]), relerr(g[f"{tag}_dP"], g64[f"{tag}_dP"]))
    if prec == "f64" or ref_self < 1e-4:
        assert relerr(cpu(Qg.grad), g[f"{tag}_dQ"]) < 1e-4
        assert relerr(cpu(Pg.grad), g[f"{tag}_dP"]) < 1e-4
    else:
        print(f"\n[{tag} f32] reference fp32 dC/dc off its own fp64 by {ref_self:.2f}: ours "
              f"{relerr(cpu(Qg.grad), g[f'{tag}_dQ']):.2e} / {relerr(cpu(Pg.grad), g[f'{tag}_dP']):.2e} from its fp32")
    # per-problem dtheta straight from the kernel
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    K, _, _ = ops.lqr_backward(Q, P, F, n, m, x=x, u=u, u_lower=lo, u_upper=hi)
    _, _, dth = implicit_backward(dx, gpu(g[f"{tag}_wx"]), gpu(g[f"{tag}_wu"]), Q, P, F, f, x, u, K, lo, hi,
                                  None)
    assert relerr(cpu(dth), g[f"{tag}_dtheta_b"]) < 1e-4


def test_mpc_end_to_end_gradient(golden):
    """dilqr.MPC forward (device loop) + implicit backward, as il_exp.py uses it
    (gradients into the cost and the model parameters), vs the reference."""
    import dilqr
    g = golden("implicit_f64")
    tag = "cart_box"
    dx = dilqr_models()["cartpole"]()
    dx.params = dx.params.clone().to(DEV).requires_grad_(True)
    x0 = gpu(g[f"{tag}_x0"])
    B, T = x0.shape[0], 10
    Q, P = gpu(g[f"{tag}_Q"]).requires_grad_(True), gpu(g[f"{tag}_P"]).requires_grad_(True)
    mpc = dilqr.MPC(5, 1, T, u_lower=-5.0, u_upper=5.0, lqr_iter=30, eps=1e-6, linesearch_decay=0.5,
                    max_linesearch_iter=2, exit_unconverged=False, detach_unconverged=False)
    x, u, _ = mpc(x0, dilqr.QuadCost(Q, P), dx)
    assert relerr(cpu(u), g[f"{tag}_u"]) < 1e-4
    loss = (x * gpu(g[f"{tag}_wx"])).sum() + (u * gpu(g[f"{tag}_wu"])).sum()
    loss.backward()
    print(f"\n[end-to-end] u {relerr(cpu(u), g[f'{tag}_u']):.2e}, dtheta "
          f"{relerr(cpu(dx.params.grad), g[f'{tag}_dtheta']):.2e}, dQ {relerr(cpu(Q.grad), g[f'{tag}_dQ']):.2e}")
    assert relerr(cpu(dx.params.grad), g[f"{tag}_dtheta"]) < 1e-4
    assert relerr(cpu(Q.grad), g[f"{tag}_dQ"]) < 1e-4


def test_implicit_backward_full_size():
    """Config 4 shape (cartpole T=25, B=65536, bounds +-10): finite gradients,
    a 128-problem slice gives bit-identical per-problem results, and an
    8-problem slice matches the fp64 oracle's fast algebra run on the same fp32
    solution (1e-4 of the max magnitude; oracle/adjoint.py is pinned to the
    reference's T=25 gradients by test_oracle_golden.py[cart25_*])."""
    import dilqr
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    B, T = 65536, 25
    rng = np.random.RandomState(0)
    th = rng.uniform(-np.pi, np.pi, B)
    x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                   rng.uniform(-1, 1, B)], 1)
    x, u, _ = run_gpu_mpc(x0, "cartpole", T, 10, (-10.0, 10.0), 0.0, 10 ** 9, 0.5, 2)
    dx = dilqr_models()["cartpole"]()
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV)
    c = p.repeat(T, B, 1).to(DEV)
    wx = torch.randn(T, B, 5, device=DEV)
    wu = torch.randn(T, B, 1, device=DEV)
    F = ops.linearize(dx.model_id, ops.theta_of(dx, C), x, u)[0]
    K, _, _ = ops.lqr_backward(C, c, F, 5, 1, x=x, u=u, u_lower=-10.0, u_upper=10.0)
    dC, dc, dth = implicit_backward(dx, wx, wu, C, c, None, None, x, u, K, -10.0, 10.0, None)
    assert torch.isfinite(dC).all() and torch.isfinite(dc).all() and torch.isfinite(dth).all()
    # an 8-problem slice spread over the batch (one problem from each of 8
    # different waves) against the fp64 oracle on the same fp32 solution
    so = [3, 8191, 16384, 20000, 33333, 47000, 60001, 65535]
    f64 = lambda a: cpu(a[:, so]).astype(np.float64)  # noqa: E731
    n_act = int(((u[:, so].abs() - 10.0).abs() <= 1e-8).sum())
    rdC, rdc, rdth = oadj.implicit_backward_fast(omodels.Cartpole, f64(wx), f64(wu), f64(C), f64(c), f64(F), None,
                                                 f64(x), f64(u), f64(K)[::-1].copy(), -10.0, 10.0)
    print(f"\n[cartpole implicit full size] {n_act} active controls in the slice; vs fp64 oracle: dtheta "
          f"{relerr(cpu(dth[so]), rdth):.2e}, dc {relerr(cpu(dc[:, so]), rdc):.2e}, dC {relerr(cpu(dC[:, so]), rdC):.2e}")
    assert relerr(cpu(dth[so]), rdth) < 1e-4
    assert relerr(cpu(dc[:, so]), rdc) < 1e-4
    assert relerr(cpu(dC[:, so]), rdC) < 1e-4
    sl = slice(1000, 1128)
    dC2, dc2, dth2 = implicit_backward(dx, wx[:, sl].contiguous(), wu[:, sl].contiguous(), C[:, sl].contiguous(),
                                       c[:, sl].contiguous(), None, None, x[:, sl].contiguous(),
                                       u[:, sl].contiguous(), K[:, sl].contiguous(), -10.0, 10.0, None)
    assert torch.equal(dth[sl], dth2) and torch.equal(dC[:, sl], dC2)
    # 130 problems: a partial last wave — the same bits
    sl4 = slice(1000, 1130)
    dC4, dc4, dth4 = implicit_backward(dx, wx[:, sl4].contiguous(), wu[:, sl4].contiguous(), C[:, sl4].contiguous(),
                                       c[:, sl4].contiguous(), None, None, x[:, sl4].contiguous(),
                                       u[:, sl4].contiguous(), K[:, sl4].contiguous(), -10.0, 10.0, None)
    assert torch.equal(dth4[:128], dth2) and torch.equal(dC4[:, :128], dC2) and torch.equal(dc4[:, :128], dc2)
    # the same slice with every off-diagonal entry of C written as -0.0: not
    # bitwise a diagonal cost, so the backward re-reads C_t in its last pass
    # instead of taking the diagonal from registers — the same values, so the
    # same results bit for bit
    Cz = C[:, sl].clone()
    off = ~torch.eye(6, dtype=torch.bool, device=DEV)
    Cz[:, :, off] = -0.0
    dC3, dc3, dth3 = implicit_backward(dx, wx[:, sl].contiguous(), wu[:, sl].contiguous(), Cz.contiguous(),
                                       c[:, sl].contiguous(), None, None, x[:, sl].contiguous(),
                                       u[:, sl].contiguous(), K[:, sl].contiguous(), -10.0, 10.0, None)
    assert torch.equal(dth3, dth2) and torch.equal(dC3, dC2) and torch.equal(dc3, dc2)


@pytest.mark.parametrize("tag", ["cart_unc", "cart_box", "pend_box", "cart25_box10"])
@pytest.mark.parametrize("cost", ["diag", "varying"])
def test_implicit_backward_batch_independent(golden, tag, cost):
    """The golden problems tiled to B = 128 (two full waves) and 129 (a partial
    third wave): the first 128 problems' dC, dc, dtheta bit for bit, and the
    per-problem dtheta against the reference's at 1e-4.  "varying": C_t and
    c_t scaled per step, so pass D re-reads the caller's C and c instead of
    holding them in registers."""
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    g = golden(implicit_file(tag))
    mname, bounds = IMPLICIT[tag]
    dx = dilqr_models()[mname]()
    x, u, Q, P, F, x0, wx, wu = (gpu(g[f"{tag}_{k}"]) for k in ("x", "u", "Q", "P", "F", "x0", "wx", "wu"))
    T, B0, n = x.shape
    m = u.shape[2]
    lo, hi = bounds if bounds else (None, None)
    if cost == "varying":
        s = torch.linspace(0.5, 1.5, T, device=DEV)
        Q = Q * s[:, None, None, None]
        P = P * s[:, None, None]

    def tile(a, Bt):
        reps = [1] * a.dim()
        reps[1] = (Bt + B0 - 1) // B0
        return a.repeat(*reps)[:, :Bt].contiguous()

    out = {}
    for Bt in (128, 129):
        xt, ut, Qt, Pt, Ft = tile(x, Bt), tile(u, Bt), tile(Q, Bt), tile(P, Bt), tile(F, Bt)
        K, _, _ = ops.lqr_backward(Qt, Pt, Ft, n, m, x=xt, u=ut, u_lower=lo, u_upper=hi)
        out[Bt] = implicit_backward(dx, tile(wx, Bt), tile(wu, Bt), Qt, Pt, Ft, None, xt, ut, K, lo, hi, None)
    (dC, dc, dth), (dC1, dc1, dth1) = out[128], out[129]
    assert torch.equal(dth, dth1[:128]) and torch.equal(dC, dC1[:, :128]) and torch.equal(dc, dc1[:, :128])
    if cost == "diag":
        assert relerr(cpu(dth[:B0]), g[f"{tag}_dtheta_b"]) < 1e-4


@pytest.mark.parametrize("model", ["cartpole", "rocket"])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_implicit_backward_short_horizons(model, T):
    """The implicit backward at horizons of 1-3 steps (at T = 1 the passes
    degenerate: no dynamics step, the costate recursion and gradx carry never
    run, dtheta = 0), both kernels (one lane per problem; rocket's 16-lane
    groups), against the fp64 oracle's fast algebra on the same fp32 solution
    (1e-4 of the max magnitude; T = 1, which the reference's grad_input cannot
    form, against the one-step problem's closed form), with bounds active for
    cartpole."""
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    B = 64
    if model == "cartpole":
        rng = np.random.RandomState(T)
        th = rng.uniform(-np.pi, np.pi, B)
        x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                       rng.uniform(-1, 1, B)], 1)
        bounds, decay, mls, om = (-2.0, 2.0), 0.5, 2, omodels.Cartpole
    else:
        x0 = rocket_x0(B, seed=T)
        bounds, decay, mls, om = None, 0.2, 5, omodels.Rocket
    x, u, _ = run_gpu_mpc(x0, model, T, 5, bounds, 0.0, 10 ** 9, decay, mls)
    dx = dilqr_models()[model]()
    n, m = x.shape[2], u.shape[2]
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV)
    c = p.repeat(T, B, 1).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(T)
    wx = torch.randn(T, B, n, device=DEV, generator=g)
    wu = torch.randn(T, B, m, device=DEV, generator=g)
    lo, hi = bounds if bounds else (None, None)
    F = ops.linearize(dx.model_id, ops.theta_of(dx, C), x, u)[0] if T > 1 else None
    K, _, _ = ops.lqr_backward(C, c, F, n, m, x=x, u=u, u_lower=lo, u_upper=hi)
    dC, dc, dth = implicit_backward(dx, wx, wu, C, c, None, None, x, u, K, lo, hi, None)
    so = slice(0, 8)
    f64 = lambda a: cpu(a[:, so]).astype(np.float64)  # noqa: E731
    if T == 1:
        # the reference's grad_input stacks T-1 = 0 dynamics steps and raises,
        # as the oracle that mirrors it does; the one-step problem's closed
        # form: y_x = 0, y_u = C_uu^-1 g_u on the free controls (diagonal C
        # here), 0 on the active ones; dc = -y, dC = -(y tau^T + tau y^T)/2
        Cn, uu, gu = f64(C)[0], f64(u)[0], f64(wu)[0]
        act = np.zeros_like(uu, dtype=bool) if lo is None else (np.abs(uu - lo) <= 1e-8) | (np.abs(uu - hi) <= 1e-8)
        yu = np.where(act, 0.0, gu / np.diagonal(Cn, axis1=1, axis2=2)[:, n:])
        y = np.concatenate([np.zeros((8, n)), yu], 1)
        tau = np.concatenate([f64(x)[0], uu], 1)
        rdc = -y[None]
        rdC = (-0.5 * (y[:, :, None] * tau[:, None, :] + tau[:, :, None] * y[:, None, :]))[None]
        assert relerr(cpu(dC[:, so]), rdC) < 1e-5 and relerr(cpu(dc[:, so]), rdc) < 1e-5
        assert float(dth.abs().max()) == 0.0
        return
    rdC, rdc, rdth = oadj.implicit_backward_fast(om, f64(wx), f64(wu), f64(C), f64(c), f64(F), None, f64(x),
                                                 f64(u), f64(K)[::-1].copy(), lo, hi)
    assert relerr(cpu(dC[:, so]), rdC) < 1e-4 and relerr(cpu(dc[:, so]), rdc) < 1e-4
    assert relerr(cpu(dth[so]), rdth) < 1e-4


def rocket_x0(B, seed=0):
    """near-hover initial states, SURVEY.md §8(d) config 3"""
    rng = np.random.RandomState(seed)
    r = rng.uniform([0, -4, -2.5], [10, 4, 2.5], (B, 3))
    v = rng.normal(0, 0.1, (B, 3))
    q4 = np.array([1., 0, 0, 0]) + 0.05 * rng.normal(size=(B, 4))
    q4 /= np.linalg.norm(q4, axis=1, keepdims=True)
    w = rng.normal(0, 0.02, (B, 3))
    return np.concatenate([r, v, q4, w], 1)


@pytest.mark.parametrize("bounds", [None, (-10.0, 10.0)])
def test_implicit_backward_rocket_full_size(bounds):
    """Config 3 shape (rocket T=30, B=32768) through the 16-lane implicit kernel:
    finite gradients, a 64-problem slice gives bit-identical per-problem results,
    and a small slice matches the oracle's fast algebra run on the same fp32
    solution (fp64 oracle, 1e-4 of the max magnitude)."""
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    B, T, n, m = 32768, 30, 13, 3
    x0 = rocket_x0(B)
    x, u, _ = run_gpu_mpc(x0, "rocket", T, 10, bounds, 0.0, 10 ** 9, 0.2, 5)
    dx = dilqr_models()["rocket"]()
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV)
    c = p.repeat(T, B, 1).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    wx = torch.randn(T, B, n, device=DEV, generator=g)
    wu = torch.randn(T, B, m, device=DEV, generator=g)
    lo, hi = bounds if bounds else (None, None)
    F = ops.linearize(dx.model_id, ops.theta_of(dx, C), x, u)[0]
    K, _, _ = ops.lqr_backward(C, c, F, n, m, x=x, u=u, u_lower=lo, u_upper=hi)
    dC, dc, dth = implicit_backward(dx, wx, wu, C, c, None, None, x, u, K, lo, hi, None)
    assert torch.isfinite(dC).all() and torch.isfinite(dc).all() and torch.isfinite(dth).all()
    sl = slice(5000, 5064)
    cut = lambda a: a[:, sl].contiguous()  # noqa: E731
    dC2, dc2, dth2 = implicit_backward(dx, cut(wx), cut(wu), cut(C), cut(c), None, None, cut(x), cut(u), cut(K),
                                       lo, hi, None)
    assert torch.equal(dth[sl], dth2) and torch.equal(dC[:, sl], dC2) and torch.equal(dc[:, sl], dc2)
    so = slice(7, 11)
    f64 = lambda a: cpu(a[:, so]).astype(np.float64)  # noqa: E731
    K_rev = f64(K)[::-1].copy()
    rdC, rdc, rdth = oadj.implicit_backward_fast(omodels.Rocket, f64(wx), f64(wu), f64(C), f64(c), f64(F), None,
                                                 f64(x), f64(u), K_rev, lo, hi)
    print(f"\n[rocket implicit full size {bounds}] vs fp64 oracle: dtheta {relerr(cpu(dth[so]), rdth):.2e}, "
          f"dc {relerr(cpu(dc[:, so]), rdc):.2e}, dC {relerr(cpu(dC[:, so]), rdC):.2e}")
    assert relerr(cpu(dth[so]), rdth) < 1e-4          # measured (round 4): <= 1.6e-6
    assert relerr(cpu(dc[:, so]), rdc) < 1e-4
    assert relerr(cpu(dC[:, so]), rdC) < 1e-4


# ------------------------------------------------------------------ 16-lanes-per-problem kernels (rocket)
@pytest.mark.parametrize("variant", ["", "chol_", "zI_", "box_"])
def test_riccati_group_rocket_vs_golden(golden, variant):
    """(n,m)=(13,3): the group Riccati sweep against the reference's sweep on the
    same random LQR (riccati golden, rocket shape).  The bounded case is checked
    against the per-problem oracle (the reference's pnqp is batch-coupled) and
    against the golden at a looser bar."""
    from dilqr import _native as N
    from dilqr import ops
    g = golden("riccati_f64")
    n, m = 13, 3
    C, c, F, u = g["rocket_C"], g["rocket_c"], g["rocket_F"], g["rocket_u"]
    kw = {}
    if variant == "chol_":
        kw = dict(m_solver=N.SOLVE_CHOL)
    elif variant == "zI_":
        kw = dict(u_zero_I=torch.tensor(g["rocket_zI"], device=DEV))
    elif variant == "box_":
        kw = dict(u=gpu(u), u_lower=-1.0, u_upper=1.0)
    K, k, _ = ops.lqr_backward(gpu(C), gpu(c), gpu(F), n, m, **kw)
    # measured (round 4): per-problem errors <= 1e-6 on k and K in every variant
    tol = 1e-4
    if variant == "box_":
        mg = {}
        Ko, ko, _ = olqr.lqr_backward(C, c, F, n, m, u=u, u_lower=-1.0, u_upper=1.0, per_problem=True, margins=mg)
        ek = np.abs(cpu(k) - ko).max(axis=(0, 2)) / max(1.0, np.abs(ko).max())
        eK = np.abs(cpu(K) - Ko).max(axis=(0, 2, 3)) / max(1.0, np.abs(Ko).max())
        print(f"\n[rocket box riccati] per problem k err {np.array2string(ek, precision=1)}, K err "
              f"{np.array2string(eK, precision=1)}, pnqp margins {np.array2string(mg.get('pnqp'), precision=1)}")
        assert relerr(cpu(K), Ko) < tol and relerr(cpu(k), ko) < tol
    assert relerr(cpu(K), g[f"rocket_{variant}K"]) < tol
    assert relerr(cpu(k), g[f"rocket_{variant}k"]) < tol


@pytest.mark.parametrize("dyn", ["rocket", "lindx"])
@pytest.mark.parametrize("bounds", [None, (-0.5, 0.5)])
def test_lqr_forward_group_vs_oracle(dyn, bounds):
    """Group line-search rollout (row-distributed dynamics, shuffle-reduced
    costs) against the oracle's lqr_forward on one sweep's gains."""
    from dilqr import ops
    from dilqr.env_dx.rocket import RocketDx
    rng = np.random.RandomState(5)
    n, m, T, B = 13, 3, 30, 37                        # B not a multiple of 4: idle groups
    M = omodels.Rocket
    x0 = np.concatenate([rng.uniform(-1, 1, (B, 6)), np.tile([1., 0, 0, 0], (B, 1)) + 0.05 * rng.normal(size=(B, 4)),
                         rng.normal(0, 0.05, (B, 3))], 1)
    u = rng.uniform(-0.5, 0.5, (T, B, m))
    q, p = M.true_obj()
    C, c = ompc.expand_cost(np.diag(q), p, T, B)
    if dyn == "rocket":
        x = olqr.get_traj(T, u, x0, lambda xx, uu: M.forward(xx, uu))
        F, f = ompc.linearize(M, x, u)
        odyn = lambda xx, uu: M.forward(xx, uu)
    else:
        F = rng.normal(0, 0.03, (T, B, n, n + m)); F[..., :n] += 0.9 * np.eye(n)
        f = rng.normal(0, 0.1, (T, B, n))
        x = olqr.get_traj(T, u, x0, ("lin", F, f))
        odyn = ("lin", F, f)
    cb = olqr.c_back(C, c, x, u)
    lo, hi = bounds if bounds else (None, None)
    Ko, ko, _ = olqr.lqr_backward(C, cb, F, n, m, u=u, u_lower=lo, u_upper=hi, per_problem=True)
    xo, uo, co, *_ = olqr.lqr_forward(x0, C, c, x, u, Ko, ko, odyn, u_lower=lo, u_upper=hi,
                                     linesearch_decay=0.2, max_linesearch_iter=5)
    dx = RocketDx()
    mid = dx.model_id if dyn == "rocket" else 0
    nx, nu, cost, _, _ = ops.lqr_forward(mid, ops.theta_of(dx, gpu(x0)), gpu(x0), gpu(C), gpu(c), gpu(x), gpu(u),
                                         gpu(Ko), gpu(ko), F=gpu(F), f=gpu(f), u_lower=lo, u_upper=hi,
                                         linesearch_decay=0.2, max_linesearch_iter=5)
    uerr = np.abs(cpu(nu) - uo).max(axis=(0, 2)) / max(1.0, np.abs(uo).max())
    xerr = np.abs(cpu(nx) - xo).max(axis=(0, 2)) / max(1.0, np.abs(xo).max())
    print(f"\n[group LS {dyn} {bounds}] cost {relerr(cpu(cost), co):.2e}; u per problem max {uerr.max():.2e} "
          f"(worst {np.argsort(-uerr)[:3]} {np.sort(uerr)[-3:]}), x max {xerr.max():.2e}")
    assert relerr(cpu(cost), co) < 1e-4                # measured (round 4): <= 2.6e-7, u and x <= 1.1e-6
    assert relerr(cpu(nu), uo) < 1e-4
    assert relerr(cpu(nx), xo) < 1e-4


def test_rocket_fused_iteration_equals_unfused(golden):
    g = golden("mpc_f64")
    mname, T, it, bounds, eps, nil, decay, mls = MPC_CASES["rocket_unc"]
    x0 = g["rocket_unc_x0"]
    a = run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls, fused=True)
    b = run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls, fused=False)
    # the 16-lane fused iteration (on-the-fly Jacobian rows, the cost in
    # registers) and the unfused kernels (k_linearize -> F in HBM -> sweep ->
    # line search) do the same arithmetic: bit for bit
    for ta, tb in zip(a, b):
        assert same_bits(ta, tb), relerr(cpu(ta), cpu(tb))


@pytest.mark.parametrize("bounds", [(-10.0, 10.0), (-3.0, 3.0)])
def test_rocket_fused_iteration_equals_unfused_box(golden, bounds):
    """The bounded rocket MPC: the 8-lane sweep's box mode (pnqp once per lane,
    two gain columns per lane, the V columns from all of K) against the unfused
    16-lane kernels with F in HBM, bit for bit, and the box actually active."""
    g = golden("mpc_f64")
    mname, T, it, _b, eps, nil, decay, mls = MPC_CASES["rocket_unc"]
    x0 = g["rocket_unc_x0"]
    a = run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls, fused=True)
    b = run_gpu_mpc(x0, mname, T, it, bounds, eps, nil, decay, mls, fused=False)
    for ta, tb in zip(a, b):
        assert same_bits(ta, tb), relerr(cpu(ta), cpu(tb))
    u = cpu(a[1])
    at_bound = np.isclose(np.abs(u), bounds[1]).mean()
    print(f"\n[rocket box {bounds}] controls at a bound: {at_bound:.2f}")
    assert at_bound > 0.0 and np.abs(u).max() <= bounds[1]


def test_rocket_fused_iteration_equals_unfused_tensor_bounds(golden):
    """Per-(t, b) control bounds ([T, B, m] tensors, the reference's
    u_lower/u_upper as tensors) through the rocket MPC: the 8-lane sweep's box
    mode and the lane search read them per step and problem; bit for bit equal
    to the unfused kernels, with bounds active."""
    g = golden("mpc_f64")
    mname, T, it, _b, eps, nil, decay, mls = MPC_CASES["rocket_unc"]
    x0 = g["rocket_unc_x0"]
    B, m = x0.shape[0], 3
    rng = np.random.RandomState(11)
    half = torch.tensor(rng.uniform(2.0, 8.0, (T, B, m)), dtype=torch.float32)
    lo, hi = (-half).to(DEV).contiguous(), half.to(DEV).contiguous()
    a = run_gpu_mpc(x0, mname, T, it, (lo, hi), eps, nil, decay, mls, fused=True)
    b = run_gpu_mpc(x0, mname, T, it, (lo, hi), eps, nil, decay, mls, fused=False)
    for ta, tb in zip(a, b):
        assert same_bits(ta, tb), relerr(cpu(ta), cpu(tb))
    u = cpu(a[1])
    at_bound = np.isclose(np.abs(u), half.numpy(), rtol=0, atol=1e-6).mean()
    print(f"\n[rocket tensor box] controls at their bound: {at_bound:.2f}")
    assert at_bound > 0.0 and (np.abs(u) <= half.numpy() + 1e-6).all()


@pytest.mark.parametrize("B", [32768, 131072])
def test_rocket_mpc_full_size_batch_independence(B):
    """Config 3 shape (B=32768, T=30) and 4x that batch on one GPU: a solve
    over the whole batch returns, for a sample of problems (the last one
    included), what solving those problems alone returns.  At B = 32768 the
    sample is also held to the fp64 oracle by decision replay."""
    import dilqr
    from dilqr.env_dx.rocket import RocketDx
    T = 30
    rng = np.random.RandomState(3)
    x0 = np.concatenate([rng.uniform([0, -4, -2.5], [10, 4, 2.5], (B, 3)), rng.normal(0, 0.1, (B, 3)),
                         np.tile([1., 0, 0, 0], (B, 1)) + 0.05 * rng.normal(size=(B, 4)),
                         rng.normal(0, 0.02, (B, 3))], 1)
    dx = RocketDx()
    q, p = dx.get_true_obj()

    def solve(xs):
        Bs = xs.shape[0]
        C = torch.diag(q).repeat(T, Bs, 1, 1).to(DEV)
        c = p.repeat(T, Bs, 1).to(DEV)
        mpc = dilqr.MPC(13, 3, T, lqr_iter=5, eps=0.0, not_improved_lim=10 ** 9, linesearch_decay=0.2,
                        max_linesearch_iter=5, exit_unconverged=False, detach_unconverged=False)
        with torch.no_grad():
            return mpc(gpu(xs), dilqr.QuadCost(C, c), dx)

    x, u, cost = solve(x0)
    assert torch.isfinite(cost).all()
    idx = np.array([0, 1, 4097, 12345, B - 2, B - 1])
    xs, us, cs = solve(x0[idx])
    print(f"rocket batch independence: max |du| {float((u[:, idx] - us).abs().max()):.3e}, "
          f"max |dcost| {float((cost[idx] - cs).abs().max()):.3e}")
    # bit for bit, as cartpole's (fixed-count solves are batch-independent,
    # SURVEY.md §4 item 4): no path of the 8-lane sweep, the lane-pair search or
    # the gain-record layout may depend on B
    idx_t = torch.tensor(idx, device=DEV)
    assert torch.equal(cost[idx_t], cs) and torch.equal(u[:, idx_t], us) and torch.equal(x[:, idx_t], xs)
    if B == 32768:
        # the sampled problems against the fp64 oracle by decision replay: the
        # per-iteration path on them alone records the decisions and gives the
        # bits of the whole-batch solve
        xd, ud, cd, alphas, takes = gpu_solve_with_decisions(x0[idx], "rocket", T, 5, None, 0.0, 10 ** 9, 0.2, 5)
        assert same_bits(xd, xs) and same_bits(ud, us) and same_bits(cd, cs)
        check_against_forced_oracle(omodels.Rocket, cpu(gpu(x0[idx])), T, None, 0.2, 5, xd, ud, cd, alphas, takes,
                                    "rocket full size slice")


# ------------------------------------------------------------------ standalone fused iteration
@pytest.mark.parametrize("model,bounds,decay,mls", [("cartpole", None, 0.5, 2), ("cartpole", (-10.0, 10.0), 0.5, 2),
                                                    ("pendulum", None, 0.2, 5), ("pendulum", None, 0.2, 3)])
def test_fused_iteration_vs_oracle(model, bounds, decay, mls):
    """dilqr_ilqr_iterate_f32 (on-the-fly linearisation, Riccati, line search
    with passes rolled out in pairs) against the oracle's sequential
    linearize -> lqr_backward -> lqr_forward, from the trajectory of a few oracle
    MPC iterations (near convergence, where problems backtrack)."""
    from dilqr import _native as N
    from dilqr import ops
    M = omodels.MODELS[model]
    n, m = M.n_state, M.n_ctrl
    T, B = (25, 192) if model == "cartpole" else (10, 192)
    rng = np.random.RandomState(7)
    if model == "cartpole":
        th = rng.uniform(-np.pi, np.pi, B)
        x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                       rng.uniform(-1, 1, B)], 1)
    else:
        th = rng.uniform(-np.pi / 2, np.pi / 2, B)
        x0 = np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, B)], 1)
    q, p = M.true_obj()
    C, c = ompc.expand_cost(np.diag(q), p, T, B)
    dyn = lambda xx, uu: M.forward(xx, uu)
    lo, hi = bounds if bounds else (None, None)
    x, u, _, _ = ompc.mpc_forward(M, x0, C, c, T, u_lower=lo, u_upper=hi, lqr_iter=8, eps=0.0,
                                  not_improved_lim=10 ** 9, linesearch_decay=decay, max_linesearch_iter=mls,
                                  per_problem=True)
    F, f = ompc.linearize(M, x, u)
    Ko, ko, _ = olqr.lqr_backward(C, olqr.c_back(C, c, x, u), F, n, m, u=u, u_lower=lo, u_upper=hi,
                                  per_problem=True)
    xo, uo, co, _, _, _, ao = olqr.lqr_forward(x0, C, c, x, u, Ko, ko, dyn, u_lower=lo, u_upper=hi,
                                               linesearch_decay=decay, max_linesearch_iter=mls)
    assert np.any(ao < 1)                      # candidate B / later rounds are exercised
    th_ = torch.tensor(M.default_params, dtype=torch.float32, device=DEV)
    Cg, cg, xg, ug, x0g = gpu(C), gpu(c), gpu(x), gpu(u), gpu(x0)
    ws = torch.empty(T * B * ops.ilqr_ws_floats(n, m), device=DEV)
    nx, nu = torch.empty_like(xg), torch.empty_like(ug)
    cost, alpha = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    du_sq = torch.empty(T, m, B, device=DEV)
    bd, keep = N.make_bounds(lo, hi)
    mid = {"cartpole": N.MODEL_CARTPOLE, "pendulum": N.MODEL_PENDULUM}[model]
    N.call("dilqr_ilqr_iterate_f32", mid, T, B, N.ptr(th_), N.ptr(x0g), N.ptr(Cg), N.ptr(cg), N.ptr(xg), N.ptr(ug),
           bd, float(decay), int(mls), N.ptr(ws), N.ptr(nx), N.ptr(nu), N.ptr(cost), N.ptr(du_sq), N.ptr(alpha),
           None, N.stream(xg.device))
    torch.cuda.synchronize()
    # decisions whose margin |cost_p - old| is below fp32 resolution may flip;
    # every problem whose accept/reject margins are clear must match exactly
    old = olqr.quad_cost_terms(C, c, np.concatenate([x, u], -1)).sum(0)
    clear = np.ones(B, bool)
    a_p = 1.0
    for p_ in range(mls):
        _, _, cp, *_ = olqr.lqr_forward(x0, C, c, x, u, Ko, a_p * ko, dyn, u_lower=lo, u_upper=hi,
                                        max_linesearch_iter=1)
        reached = ao <= a_p * (1 + 1e-9)               # problems that evaluated pass p
        clear &= ~reached | (np.abs(cp - old) > 1e-5 * np.maximum(1.0, np.abs(old)))
        a_p *= decay
    assert np.mean(clear) > 0.5
    same = np.abs(cpu(alpha) - ao) < 1e-6 * np.maximum(1, ao)
    assert same[clear].all(), np.flatnonzero(clear & ~same)
    cerr = np.abs(cpu(cost) - co) / np.maximum(1.0, np.abs(co))
    uerr = np.abs(cpu(nu) - uo).max(axis=(0, 2)) / max(1.0, np.abs(uo).max())
    xerr = np.abs(cpu(nx) - xo).max(axis=(0, 2)) / max(1.0, np.abs(xo).max())
    print(f"\n[fused vs oracle {model} {bounds}] same {same.sum()}/{B}, clear {clear.sum()}; cost max "
          f"{cerr[same].max():.2e} med {np.median(cerr[same]):.2e}; u max {uerr[same].max():.2e}, x max "
          f"{xerr[same].max():.2e}; worst problems u {np.argsort(-uerr * same)[:4]} "
          f"{np.sort(uerr[same])[-4:]}")
    # measured (round 4): costs <= 1.8e-5, u and x <= 2.5e-6 on the problems with the oracle's step size
    assert np.median(cerr[same]) < 1e-5 and np.max(cerr[same]) < 1e-4
    assert relerr(cpu(nu)[:, same], uo[:, same]) < 1e-4
    assert relerr(cpu(nx)[:, same], xo[:, same]) < 1e-4


# ------------------------------------------------------------------ standalone pnqp (a4)
@pytest.mark.parametrize("m", [1, 3])
def test_pnqp_standalone_vs_golden(golden, m):
    """dilqr_pnqp_f32 against the reference's pnqp called per problem (golden
    x_pp / it_pp), and with a warm start and scalar bounds against the oracle's
    per-problem restatement (x, free mask, masked H, iteration index)."""
    from dilqr import ops
    g = golden("pnqp_f64")
    H, q, lo, hi, x0 = (g[f"m{m}_{k}"] for k in ("H", "q", "lo", "hi", "x0"))
    x, Hf, If, it = ops.pnqp(gpu(H), gpu(q), gpu(lo), gpu(hi))
    assert relerr(cpu(x), g[f"m{m}_x_pp"]) < 1e-4
    mg = {}
    olqr.pnqp(H, q, lo, hi, per_problem=True, margins=mg)
    dif = cpu(it) != g[f"m{m}_it_pp"]
    print(f"\n[pnqp m={m}] x {relerr(cpu(x), g[f'm{m}_x_pp']):.2e}; exit index differs on {dif.sum()}/{len(dif)}, "
          f"their decision margins {np.array2string(mg['pnqp'][dif], precision=1)}; smallest margin elsewhere "
          f"{mg['pnqp'][~dif].min():.1e}")
    # exit index: equal, except on a decision within 1e-4 of its threshold (the stop
    # test |dx| < 1e-4 sits there); measured (round 4): equal on every problem
    assert dif.sum() <= 2 and np.all(mg["pnqp"][dif] < 1e-4), np.flatnonzero(dif)
    x2, Hf2, If2, it2 = ops.pnqp(gpu(H), gpu(q), -0.7, 0.7, x_init=gpu(x0))
    mg2 = {}
    xo, Hfo, Ifo, ito = olqr.pnqp(H, q, -0.7, 0.7, x_init=x0, per_problem=True, margins=mg2)
    assert relerr(cpu(x2), xo) < 1e-4
    same = cpu(it2) == ito
    print(f"[pnqp m={m} warm] x {relerr(cpu(x2), xo):.2e}; exit index differs on {(~same).sum()}, margins "
          f"{np.array2string(mg2['pnqp'][~same], precision=1)}")
    assert (~same).sum() <= 2 and np.all(mg2["pnqp"][~same] < 1e-4), np.flatnonzero(~same)
    assert np.array_equal(cpu(If2)[same], Ifo[same])
    assert relerr(cpu(Hf2)[same], Hfo[same]) < 1e-5


# ------------------------------------------------------------------ model protocol: get_matrices, grad_input
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "rocket"])
def test_get_matrices_and_grad_input_vs_golden(golden, name):
    """env_dx get_matrices (cartpole.py:105-716, pendulum.py:152-382, rocket.py:
    258-261) and grad_input (cartpole.py:717-788, pendulum.py:383-443, rocket.py:
    263-323) on the GPU (dilqr_get_matrices_f32 / dilqr_grad_input_f32) against
    the reference's own outputs (golden 'gm' / 'gi', fp64): 1e-4 of each array's
    magnitude (fp32 arithmetic; the reference's fp32 run sits within 3e-5)."""
    g = golden("models_f64")
    dx = dilqr_models()[name]()
    X, U = g[f"{name}_x"][:16], g[f"{name}_u"][:16]
    got = dx.get_matrices(gpu(X), gpu(U))
    keys = ("D", "D_params", "D_x", "D_u", "x_theta", "x_xtm1", "x_utm1")
    errs = {k: relerr(cpu(a), g[f"{name}_gm_{k}"]) for k, a in zip(keys, got)}
    gi = dx.grad_input(gpu(g[f"{name}_gi_X"]), gpu(g[f"{name}_gi_U"]), gpu(g[f"{name}_gi_K"]))
    gkeys = ("grad_D", "grad_d", "D_x", "D_u", "D", "d_x", "d_u")
    errs.update({"gi_" + k: relerr(cpu(a), g[f"{name}_gi_{k}"]) for k, a in zip(gkeys, gi)})
    print(f"\n[{name}] get_matrices / grad_input max rel err: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


# ------------------------------------------------------------------ API options: delta_u, u_zero_I
def test_lqrstep_delta_u_vs_golden(golden):
    """LQRStep(delta_u=0.5) with bounds +-5 (lqr_step_explicit.py:132-135: the
    sweep's relative box clipped to +-delta_u; 205-213: the rollout's clamp to
    [max(lower, u - delta_u), min(upper, u + delta_u)]) against the reference."""
    import dilqr
    from dilqr.env_dx.cartpole import CartpoleDx
    g = golden("api_f64")
    x0, u, x, F, f = (g[f"dlt_{k}"] for k in ("x0", "u", "x", "F", "f"))
    T, B, _ = u.shape
    dx = CartpoleDx()
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV)
    c = p.repeat(T, B, 1).to(DEV)
    step = dilqr.LQRStep(5, 1, T, u_lower=-5.0, u_upper=5.0, delta_u=0.5, true_cost=dilqr.QuadCost(C, c),
                         true_dynamics=dx, current_x=gpu(x), current_u=gpu(u), linesearch_decay=0.5,
                         max_linesearch_iter=2)
    nx, nu, _, costs, _, malpha = step(gpu(x0), C, c, gpu(F), gpu(f), None)
    errs = (relerr(cpu(costs), g["dlt_costs"]), relerr(cpu(nu), g["dlt_nu"]), relerr(cpu(nx), g["dlt_nx"]))
    print(f"\n[delta_u] costs {errs[0]:.2e} u {errs[1]:.2e} x {errs[2]:.2e}")
    assert np.all(np.abs(cpu(nu) - u) <= 0.5 + 1e-6)          # the trust region holds
    assert errs[0] < 1e-5 and errs[1] < 1e-4 and errs[2] < 1e-4
    assert abs(float(malpha) - float(g["dlt_malpha"])) < 1e-6


@pytest.mark.parametrize("tag", ["zi_cart", "zi_cartbox", "zi_rock"])
def test_mpc_u_zero_I_vs_golden(golden, tag):
    """MPC(u_zero_I=mask): controls held at zero (the masked gain solve,
    lqr_step_explicit.py:98-129, and the zeroed rollout, 199-200, through the
    unfused HIP kernels) against the reference's mpc_explicit.MPC."""
    import dilqr
    g = golden("api_f64")
    mname = "rocket" if "rock" in tag else "cartpole"
    dx = dilqr_models()[mname]()
    x0, zI = g[f"{tag}_x0"], g[f"{tag}_zI"]
    T, B, m = zI.shape
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1).to(DEV)
    c = p.repeat(T, B, 1).to(DEV)
    lo, hi = (-10.0, 10.0) if tag == "zi_cartbox" else (None, None)
    decay, mls, it = (0.5, 2, 5) if mname == "cartpole" else (0.2, 5, 3)
    mpc = dilqr.MPC(dx.n_state, m, T, u_lower=lo, u_upper=hi, u_zero_I=torch.tensor(zI, device=DEV), lqr_iter=it,
                    eps=0.0, not_improved_lim=10 ** 9, linesearch_decay=decay, max_linesearch_iter=mls,
                    exit_unconverged=False, detach_unconverged=False)
    with torch.no_grad():
        x, u, costs = mpc(gpu(x0), dilqr.QuadCost(C, c), dx)
    assert torch.all(u[torch.tensor(zI, device=DEV)] == 0)
    errs = (relerr(cpu(costs), g[f"{tag}_costs"]), relerr(cpu(u), g[f"{tag}_u"]), relerr(cpu(x), g[f"{tag}_x"]))
    print(f"\n[{tag}] costs {errs[0]:.2e} u {errs[1]:.2e} x {errs[2]:.2e}")
    assert errs[0] < 1e-5 and errs[1] < 1e-4 and errs[2] < 1e-4


def test_implicit_backward_u_zero_I_vs_golden(golden):
    """The DiLQR no-op step with a u_zero_I mask (its masked Riccati gains feed
    grad_input's closed loop) + the implicit backward, against the reference."""
    import dilqr
    g = golden("api_f64")
    dx = dilqr_models()["cartpole"]()
    x0, u, x, zI = (g[f"zim_{k}"] for k in ("x0", "u", "x", "zI"))
    T, B, _ = u.shape
    q, p = dx.get_true_obj()
    Q = torch.diag(q).repeat(T, B, 1, 1).to(DEV).requires_grad_(True)
    P = p.repeat(T, B, 1).to(DEV).requires_grad_(True)
    from dilqr import ops
    F, f = ops.linearize(dx.model_id, ops.theta_of(dx, Q), gpu(x), gpu(u))
    theta = dx.params.clone().to(DEV).requires_grad_(True)
    step = dilqr.LQRStep(5, 1, T, u_zero_I=torch.tensor(zI, device=DEV), true_cost=dilqr.QuadCost(Q, P),
                         true_dynamics=dx, current_x=gpu(x), current_u=gpu(u), no_op_forward=True)
    x2, u2 = step(gpu(x0), Q, P, F, f, theta)
    ((x2 * gpu(g["zim_wx"])).sum() + (u2 * gpu(g["zim_wu"])).sum()).backward()
    errs = (relerr(cpu(theta.grad), g["zim_dtheta"]), relerr(cpu(Q.grad), g["zim_dQ"]), relerr(cpu(P.grad), g["zim_dP"]))
    print(f"\n[u_zero_I implicit] dtheta {errs[0]:.2e} dQ {errs[1]:.2e} dP {errs[2]:.2e}")
    assert max(errs) < 1e-4


@pytest.mark.parametrize("B,off", [(64, 40), (12288, 12256)])
def test_rocket_register_cost_bit_identical(B, off):
    """The 16-lane MPC kernel holds a time-invariant diagonal cost in two
    registers per lane (flag 7 from iteration 0) instead of reading the caller's
    16 x 16 rows every step and pass: the same values, so bit-identical
    trajectories and costs with and without the solve's cost record, on a batch
    that mixes flagged problems with a time-varying and a non-diagonal cost.
    At B = 12288 the dense problems are the batch's last: after iteration 0 the
    dense-cost sweep and search run on a small grid striding over the batch
    (kDenseGrid workgroups), which must reach them."""
    from dilqr import _native as N
    from dilqr import ops
    dx = dilqr_models()["rocket"]()
    T, n, m = 12, 13, 3
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1)
    c = p.repeat(T, B, 1).clone()
    C[:, off:off + 8, 0, 1] += 1e-3               # not diagonal
    C[:, off:off + 8, 1, 0] += 1e-3
    c[3, off + 8:off + 16] += 0.01                # not time-invariant
    C, c = C.to(DEV).contiguous(), c.to(DEV).contiguous()
    x0 = gpu(rocket_x0(B, seed=4))
    theta = ops.theta_of(dx, x0)
    nb, _ = N.make_bounds(None, None)
    out = []
    for packed in (True, False):
        sv = ops.MPCSolve(T, B, n, m, DEV, packed_cost=packed)
        sv.begin(dx.model_id, theta, x0)
        for i in range(4):
            sv.iterate(dx.model_id, theta, x0, C, c, nb, 0.2, 5, i, 1e-4, 0.0, 10 ** 9)
        x, u = sv.gather_best()
        out.append((x, u, sv.best_cost.clone()))
        if packed:
            flags = cpu(sv.cost_sym)
            assert (flags[:off] == 7).all() and (flags[off + 16:] == 7).all() and (flags[off:off + 16] == 0).all()
    for a, b in zip(*out):
        assert same_bits(a, b)
