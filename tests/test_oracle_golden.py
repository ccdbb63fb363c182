"""Pin the numpy oracle against golden vectors produced by the reference itself.

CPU-only.  The goldens (tests/golden/*.npz) were written by
tests/golden/gen_golden.py, which ran the reference in the build container.
fp64 goldens are compared tightly (the oracle restates the same algorithm, so
only summation-order rounding differs); fp32 goldens loosely.
"""
import numpy as np
import pytest

from oracle import adjoint, lqr, models, mpc

MODELS = models.MODELS


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


# ---------------------------------------------------------------- models
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "rocket"])
@pytest.mark.parametrize("prec,tol", [("f64", 1e-12), ("f32", 2e-5)])
def test_model_forward_and_jacobian(golden, name, prec, tol):
    g = golden(f"models_{prec}")
    dt = np.float64 if prec == "f64" else np.float32
    M = MODELS[name]
    x, u = g[f"{name}_x"].astype(dt), g[f"{name}_u"].astype(dt)
    assert rel(M.forward(x, u), g[f"{name}_fwd"]) < tol
    assert rel(M.get_linear_dyn(x, u), g[f"{name}_D"]) < tol * 10




@pytest.mark.parametrize("name", ["pendulum", "cartpole", "rocket"])
def test_model_get_matrices(golden, name):
    g = golden("models_f64")
    M = MODELS[name]
    x, u = g[f"{name}_x"][:16], g[f"{name}_u"][:16]
    mats = M.get_matrices(x, u)
    for key, val in zip(("D", "D_params", "D_x", "D_u", "x_theta", "x_xtm1", "x_utm1"), mats):
        ref = g[f"{name}_gm_{key}"]
        assert ref.shape == val.shape, (key, ref.shape, val.shape)
        assert rel(val, ref) < 1e-10, key


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "rocket"])
def test_model_grad_input(golden, name):
    g = golden("models_f64")
    M = MODELS[name]
    out = M.grad_input(g[f"{name}_gi_X"], g[f"{name}_gi_U"], g[f"{name}_gi_K"])
    for key, val in zip(("grad_D", "grad_d", "D_x", "D_u", "D", "d_x", "d_u"), out):
        ref = g[f"{name}_gi_{key}"]
        assert ref.shape == val.shape, (key, ref.shape, val.shape)
        assert rel(val, ref) < 1e-10, key


# ---------------------------------------------------------------- Riccati
SHAPES = {"pendulum": (3, 1, 10, 16), "cartpole": (5, 1, 25, 16), "rocket": (13, 3, 30, 8)}


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("variant", ["", "chol_", "zI_", "box_"])
def test_riccati(golden, name, variant):
    g = golden("riccati_f64")
    n, m, T, B = SHAPES[name]
    C, c, F, u = g[f"{name}_C"], g[f"{name}_c"], g[f"{name}_F"], g[f"{name}_u"]
    kw = {}
    if variant == "chol_":
        kw = dict(m_solver="chol")
    elif variant == "zI_":
        kw = dict(m_solver="chol", u_zero_I=g[f"{name}_zI"])
    elif variant == "box_":
        kw = dict(u=u, u_lower=-1.0, u_upper=1.0)
    K, k, _ = lqr.lqr_backward(C, c, F, n, m, **kw)
    assert rel(K, g[f"{name}_{variant}K"]) < 1e-9
    assert rel(k, g[f"{name}_{variant}k"]) < 1e-9


# ---------------------------------------------------------------- pnqp
@pytest.mark.parametrize("m", [1, 3])
def test_pnqp(golden, m):
    g = golden("pnqp_f64")
    H, q, lo, hi, x0 = (g[f"m{m}_{k}"] for k in ("H", "q", "lo", "hi", "x0"))
    x, _, If, it = lqr.pnqp(H, q, lo, hi)
    assert rel(x, g[f"m{m}_x"]) < 1e-10 and it == g[f"m{m}_it"]
    np.testing.assert_array_equal(If, g[f"m{m}_If"])
    x, _, If, it = lqr.pnqp(H, q, -0.7, 0.7, x_init=x0)
    assert rel(x, g[f"m{m}_xf"]) < 1e-10 and it == g[f"m{m}_itf"]
    x, _, _, its = lqr.pnqp(H, q, lo, hi, per_problem=True)
    assert rel(x, g[f"m{m}_x_pp"]) < 1e-10
    np.testing.assert_array_equal(its, g[f"m{m}_it_pp"])


# ---------------------------------------------------------------- one LQR step
@pytest.mark.parametrize("tag,bounds", [("unc", None), ("box", (-5.0, 5.0))])
def test_lqr_step(golden, tag, bounds):
    g = golden("lqrstep_f64")
    M = MODELS["cartpole"]
    x0, u, x = g[f"{tag}_x0"], g[f"{tag}_u"], g[f"{tag}_x"]
    T, B, _ = u.shape
    assert rel(lqr.get_traj(T, u, x0, M.forward), x) < 1e-12
    F, f = mpc.linearize(M, x, u)
    assert rel(F, g[f"{tag}_F"]) < 1e-12 and rel(f, g[f"{tag}_f"]) < 1e-12
    q, p = M.true_obj()
    C, c = mpc.expand_cost(np.diag(q), p, T, B)
    lo, hi = bounds if bounds else (None, None)
    K, k, _ = lqr.lqr_backward(C, lqr.c_back(C, c, x, u), F, 5, 1, u=u, u_lower=lo, u_upper=hi)
    nx, nu, costs, du, _, malpha, _ = lqr.lqr_forward(x0, C, c, x, u, K, k, M.forward, lo, hi, None, 0.5, 2)
    assert rel(nx, g[f"{tag}_nx"]) < 1e-10
    assert rel(nu, g[f"{tag}_nu"]) < 1e-10
    assert rel(costs, g[f"{tag}_costs"]) < 1e-10
    assert rel(du, g[f"{tag}_du"]) < 1e-10
    assert abs(malpha - g[f"{tag}_malpha"]) < 1e-12


# ---------------------------------------------------------------- MPC solves
MPC_CASES = {
    "cart_unc": ("cartpole", 25, 10, None, 0.0, 10 ** 9, 0.5, 2),
    "cart_box10": ("cartpole", 25, 10, (-10.0, 10.0), 0.0, 10 ** 9, 0.5, 2),
    "cart_il": ("cartpole", 25, 40, (-100.0, 100.0), 1e-4, 5, 0.5, 2),
    "pend_unc": ("pendulum", 10, 10, None, 0.0, 10 ** 9, 0.2, 5),
    "pend_box": ("pendulum", 10, 10, (-2.0, 2.0), 0.0, 10 ** 9, 0.2, 5),
    "rocket_unc": ("rocket", 30, 5, None, 0.0, 10 ** 9, 0.2, 5),
}


def run_oracle_mpc(g, name, dt, **over):
    mname, T, it, bounds, eps, nil, decay, mls = MPC_CASES[name]
    M = MODELS[mname]
    x0 = g[f"{name}_x0"].astype(dt)
    B = x0.shape[0]
    q, p = M.true_obj()
    C, c = mpc.expand_cost(np.diag(q).astype(dt), p.astype(dt), T, B)
    lo, hi = bounds if bounds else (None, None)
    kw = dict(u_lower=lo, u_upper=hi, lqr_iter=it, eps=eps, not_improved_lim=nil,
              linesearch_decay=decay, max_linesearch_iter=mls)
    kw.update(over)
    return mpc.mpc_forward(M, x0, C, c, T, **kw)


@pytest.mark.parametrize("name", list(MPC_CASES))
def test_mpc_f64(golden, name):
    g = golden("mpc_f64")
    x, u, costs, _ = run_oracle_mpc(g, name, np.float64)
    assert rel(x, g[f"{name}_x"]) < 1e-8
    assert rel(u, g[f"{name}_u"]) < 1e-8
    assert rel(costs, g[f"{name}_costs"]) < 1e-8


@pytest.mark.parametrize("name", ["cart_unc", "cart_box10", "pend_box"])
def test_mpc_iterates_f64(golden, name):
    g = golden("mpc_f64")
    if f"{name}_it1_u" not in g:
        pytest.skip("no per-iteration goldens for this case")
    for k in (1, 2, 3):
        x, u, costs, _ = run_oracle_mpc(g, name, np.float64, lqr_iter=k)
        assert rel(u, g[f"{name}_it{k}_u"]) < 1e-9, k


@pytest.mark.parametrize("name", ["cart_unc", "cart_box10", "pend_unc", "pend_box"])
def test_mpc_f32(golden, name):
    """fp32 oracle vs fp32 reference: same algorithm, different summation
    order; line-search/active-set decisions can flip on 1-ulp differences, so
    the bar is the trajectory cost."""
    g = golden("mpc_f32")
    x, u, costs, _ = run_oracle_mpc(g, name, np.float32)
    ref = g[f"{name}_costs"]
    assert np.max(np.abs(costs - ref) / np.maximum(1.0, np.abs(ref))) < 1e-3


# ---------------------------------------------------------------- 5-parameter pendulum
@pytest.mark.parametrize("prec,tol", [("f64", 1e-12), ("f32", 2e-5)])
def test_pendulum_complex_forward_and_jacobian(golden, prec, tol):
    """pendulum.py simple=False: forward and its autograd Jacobian (the
    reference's AUTO_DIFF linearisation, mpc_explicit.py:562-566)."""
    g = golden(f"complex_{prec}")
    dt = np.float64 if prec == "f64" else np.float32
    x, u = g["x"].astype(dt), g["u"].astype(dt)
    PC = models.PendulumComplex
    assert rel(PC.forward(x, u), g["fwd"]) < tol
    assert rel(PC.get_linear_dyn(x, u), g["jac"]) < 10 * tol


@pytest.mark.parametrize("name", ["fixed", "il"])
def test_pendulum_complex_mpc_f64(golden, name):
    """mpc_explicit.MPC(GradMethods.AUTO_DIFF) on the 5-parameter pendulum,
    bounds +-2, decay 0.2, max_ls 5 (the reference's fp64 run)."""
    g = golden("complex_f64")
    T, B = g[f"{name}_u"].shape[:2]
    it, eps, nil = {"fixed": (10, 0.0, 10 ** 9), "il": (40, 1e-3, 5)}[name]
    q, p = models.PendulumComplex.true_obj()
    C, c = mpc.expand_cost(np.diag(q), p, T, B)
    x, u, costs, _ = mpc.mpc_forward(models.PendulumComplex, g[f"{name}_x0"], C, c, T, u_lower=-2.0, u_upper=2.0,
                                     lqr_iter=it, eps=eps, not_improved_lim=nil, linesearch_decay=0.2,
                                     max_linesearch_iter=5)
    assert rel(u, g[f"{name}_u"]) < 1e-8 and rel(x, g[f"{name}_x"]) < 1e-8
    assert rel(costs, g[f"{name}_costs"]) < 1e-8


# ---------------------------------------------------------------- classic adjoint
@pytest.mark.parametrize("tag,bounds", [("m1", None), ("m3", None), ("m1box", (-0.5, 0.5)),
                                        ("m3box", (-0.5, 0.5))])
def test_classic_adjoint(golden, tag, bounds):
    g = golden("adjoint_f64")
    C, c, F, f, x0 = (g[f"{tag}_{k}"] for k in ("C", "c", "F", "f", "x0"))
    T, B, d = c.shape
    n = x0.shape[1]
    m = d - n
    lo, hi = bounds if bounds else (None, None)
    x, u, costs, _ = mpc.mpc_forward(("lin", F, f), x0, C, c, T, u_lower=lo, u_upper=hi, lqr_iter=1)
    assert rel(x, g[f"{tag}_x"]) < 1e-10 and rel(u, g[f"{tag}_u"]) < 1e-10
    dx0, dC, dc, dF, df = adjoint.classic_backward(g[f"{tag}_wx"], g[f"{tag}_wu"], x0, C, c, F, f,
                                                   x, u, lo, hi)
    for key, val in (("dx0", dx0), ("dC", dC), ("dc", dc), ("dF", dF), ("df", df)):
        assert rel(val, g[f"{tag}_{key}"]) < 1e-9, key


# ---------------------------------------------------------------- DiLQR implicit backward
IMPLICIT = {"cart_unc": ("cartpole", None), "cart_box": ("cartpole", (-5.0, 5.0)),
            "pend_box": ("pendulum", (-2.0, 2.0)), "rock_unc": ("rocket", None),
            "rock_box": ("rocket", (-10.0, 10.0)),
            # config 4's horizon: cartpole T=25, B=8 (gen_golden.py IMPLICIT25_CASES)
            "cart25_unc": ("cartpole", None), "cart25_box10": ("cartpole", (-10.0, 10.0)),
            "cart25_box100": ("cartpole", (-100.0, 100.0))}


def implicit_file(tag, prec="f64"):
    return f"implicit25_{prec}" if tag.startswith("cart25") else f"implicit_{prec}"


@pytest.mark.parametrize("tag", list(IMPLICIT))
def test_implicit_backward_f64(golden, tag):
    g = golden(implicit_file(tag))
    mname, bounds = IMPLICIT[tag]
    M = MODELS[mname]
    x, u, Q, P, F = (g[f"{tag}_{k}"] for k in ("x", "u", "Q", "P", "F"))
    T, B, n = x.shape
    m = u.shape[2]
    Fo, fo = mpc.linearize(M, x, u)
    assert rel(Fo, F) < 1e-12
    lo, hi = bounds if bounds else (None, None)
    K, _, _ = lqr.lqr_backward(Q, lqr.c_back(Q, P, x, u), Fo, n, m, u=u, u_lower=lo, u_upper=hi)
    dC, dc, dth = adjoint.implicit_backward(M, g[f"{tag}_wx"], g[f"{tag}_wu"], Q, P, Fo, fo, x, u,
                                            K[::-1], lo, hi)
    assert rel(dth, g[f"{tag}_dtheta_b"]) < 1e-6
    assert rel(dth.sum(0), g[f"{tag}_dtheta"]) < 1e-6
    assert rel(dC, g[f"{tag}_dQ"]) < 1e-6
    assert rel(dc, g[f"{tag}_dP"]) < 1e-6


# ---------------------------------------------------------------- the reference's own datasets
def test_dataset_cartpole_known_answer(golden):
    """data/cartpole.pkl: expert trajectories made by the reference solver
    (il_env.py:81-94) at fp32, T=35, lqr_iter=100, bounds +-100, eps 1e-4,
    decay 0.5, max_ls 2, start th = pi/1.05.  Re-solve from their x_init."""
    g = golden("datasets")
    tau = np.concatenate([g["cartpole_train_data"], g["cartpole_val_data"], g["cartpole_test_data"]])
    tau = tau.astype(np.float32)
    M = MODELS["cartpole"]
    T = int(g["cartpole_mpc_T"])
    x0 = tau[:, 0, :5]
    B = x0.shape[0]
    q, p = M.true_obj()
    C, c = mpc.expand_cost(np.diag(q).astype(np.float32), p.astype(np.float32), T, B)
    x, u, costs, _ = mpc.mpc_forward(M, x0, C, c, T, u_lower=float(g["cartpole_lower"]),
                                     u_upper=float(g["cartpole_upper"]), lqr_iter=int(g["cartpole_lqr_iter"]),
                                     eps=float(g["cartpole_mpc_eps"]), linesearch_decay=float(g["cartpole_linesearch_decay"]),
                                     max_linesearch_iter=int(g["cartpole_max_linesearch_iter"]))
    got = np.concatenate([x, u], 2).transpose(1, 0, 2)
    assert np.max(np.abs(got - tau)) < 5e-3


@pytest.mark.parametrize("tag", list(IMPLICIT))
def test_implicit_backward_fast_f64(golden, tag):
    """The O(T d^3) algebra (the one the HIP kernels use, and the checker the
    full-size GPU tests call) against the reference's (T d)^3 KKT solve."""
    g = golden(implicit_file(tag))
    mname, bounds = IMPLICIT[tag]
    M = MODELS[mname]
    x, u, Q, P = (g[f"{tag}_{k}"] for k in ("x", "u", "Q", "P"))
    T, B, n = x.shape
    m = u.shape[2]
    Fo, fo = mpc.linearize(M, x, u)
    lo, hi = bounds if bounds else (None, None)
    K, _, _ = lqr.lqr_backward(Q, lqr.c_back(Q, P, x, u), Fo, n, m, u=u, u_lower=lo, u_upper=hi)
    dC, dc, dth = adjoint.implicit_backward_fast(M, g[f"{tag}_wx"], g[f"{tag}_wu"], Q, P, Fo, fo, x, u,
                                                 K[::-1], lo, hi)
    # rocket: the reference's dense 160x160 KKT solve (lqr_step_explicit.py:570)
    # is ill-conditioned enough to move its fp64 dtheta by ~6.5e-6 relative to
    # the recursion's; every other case agrees to < 1e-6
    tol = 2e-5 if mname == "rocket" else 1e-6
    assert rel(dth, g[f"{tag}_dtheta_b"]) < tol
    assert rel(dC, g[f"{tag}_dQ"]) < tol
    assert rel(dc, g[f"{tag}_dP"]) < tol


# ---------------------------------------------------------------- dense / time-varying / asymmetric costs
import cost_cases as CC  # noqa: E402  (tests/cost_cases.py, shared with gen_golden.py case_costs)


def oracle_true_obj(mname):
    return MODELS[mname].true_obj()


@pytest.mark.parametrize("name,mode", [(n_, mo) for n_ in CC.SWEEP_SHAPES for mo in CC.SWEEP_MODES[n_]])
def test_riccati_cost_classes(golden, name, mode):
    """lqr_backward on the eight cost classes of tests/cost_cases.py (two
    problems of each in a batch of 16, T = 9) against the reference's sweep as
    LQRStepFn.forward runs it, c_back formed from x, u inside.  This pins the
    oracle's reading of an asymmetric C: c_back = C tau + c, not the symmetrised
    form (lqr_step_explicit.py:635); Q_ux the lower-left block (:80); the
    asymmetric Q_uu itself into the gain solve (:87-96, pnqp :137; the Cholesky
    engine reads its lower triangle, lqr_step_backup.py:203).  The reference is
    finite in every mode on an asymmetric C_uu, so every mode keeps all eight
    classes (the box keeps C_uu symmetric for m > 1, as the cases define it)."""
    g = golden("costs_f64")
    pr = CC.sweep_problem(name, oracle_true_obj, int(g[f"{name}_seed"]))
    CC.check(g[f"{name}_sum"], pr["C"], pr["c"], pr["C_box"], pr["c_box"], pr["F"], pr["x"], pr["u"])
    n, m = pr["n"], pr["m"]
    C, c = (pr["C_box"], pr["c_box"]) if mode == "box" else (pr["C"], pr["c"])
    kw = {}
    if mode == "box":
        kw = dict(u=pr["u"], u_lower=-CC.SWEEP_BOX, u_upper=CC.SWEEP_BOX)
    elif mode == "chol":
        kw = dict(m_solver="chol")
    K, k, _ = lqr.lqr_backward(C, lqr.c_back(C, c, pr["x"], pr["u"]), pr["F"], n, m, **kw)
    assert rel(K, g[f"{name}_{mode}_K"]) < 1e-9
    assert rel(k, g[f"{name}_{mode}_k"]) < 1e-9


@pytest.mark.parametrize("name", list(CC.MPC_CASES))
def test_mpc_cost_classes_f64(golden, name):
    """mpc_forward on the mixed-class MPC fixtures (and rocket at config 3's
    own 10 iterations) against the reference's fp64 solves."""
    g = golden("costs_f64")
    mname, T, Bf, it, bounds, decay, mls, _mixed = CC.MPC_CASES[name]
    C, c = CC.mpc_costs(name, oracle_true_obj, int(g[f"{name}_seed"]))
    CC.check(g[f"{name}_sum"], C, c)
    lo, hi = bounds if bounds else (None, None)
    x, u, costs, _ = mpc.mpc_forward(MODELS[mname], g[f"{name}_x0"], C, c, T, u_lower=lo, u_upper=hi, lqr_iter=it,
                                     eps=0.0, not_improved_lim=10 ** 9, linesearch_decay=decay,
                                     max_linesearch_iter=mls)
    assert rel(x, g[f"{name}_x"]) < 1e-8
    assert rel(u, g[f"{name}_u"]) < 1e-8
    assert rel(costs, g[f"{name}_costs"]) < 1e-8


# ---------------------------------------------------------------- the implicit backward on the cost classes
def implicit_costs_oracle(pr, fn, sel=None):
    """fn (implicit_backward or implicit_backward_fast) on the problems sel of a fixture."""
    M = MODELS[pr["mname"]]
    s = np.arange(len(pr["classes"])) if sel is None else np.asarray(sel)
    x, u, C, c, wx, wu = (pr[k][:, s] for k in ("x", "u", "C", "c", "wx", "wu"))
    Fo, fo = mpc.linearize(M, x, u)
    K, _, _ = lqr.lqr_backward(C, lqr.c_back(C, c, x, u), Fo, pr["n"], pr["m"], u=u, u_lower=pr["lo"], u_upper=pr["hi"])
    return fn(M, wx, wu, C, c, Fo, fo, x, u, K[::-1], pr["lo"], pr["hi"])


def implicit_costs_errors(got, exp):
    return np.stack([CC.per_problem(got[0], exp[0], 1), CC.per_problem(got[1], exp[1], 1),
                     CC.per_problem(got[2], exp[2], 0)], 1)


@pytest.mark.parametrize("tag", list(CC.IMPLICIT_COSTS))
def test_implicit_backward_fast_cost_classes(golden, tag):
    """implicit_backward_fast on the fifteen cost classes (T = 10, one problem of
    each) against the reference's LQRStep(no_op_forward=True) backward, per
    problem, at test_implicit_backward_fast_f64's bars.  The reference agrees on
    every class (asymmetric ones included) to 1e-13, and on rocket
    unconstrained to 2.5e-6 (dC, dc) and 1.4e-5 (dtheta),
    except where C_uu itself is asymmetric with m > 1 (rocket unconstrained, the
    four asym classes): its nested adjoint solve factors Q_uu by Cholesky, which
    reads one triangle, and its dC, dc, dtheta then leave the LU elimination's
    by up to 7e-2, 7e-2, 1.4e-1.  Those four problems are pinned to this
    function's own fp64 value (g["rock_unc_pinned"]); here they are held to the
    reference's answer being off by what the generator recorded, so that a
    change of either is seen."""
    g = golden("implicit_costs_f64")
    pr = CC.implicit_costs_problem(g, tag, oracle_true_obj)
    got = implicit_costs_oracle(pr, adjoint.implicit_backward_fast)
    err = implicit_costs_errors(got, (pr["dQ"], pr["dP"], pr["dtheta"]))
    pin = pr["pinned"]
    tol = 2e-5 if pr["mname"] == "rocket" else 1e-6
    assert err[~pin].max() < tol, dict(zip(pr["classes"], err.max(1)))
    assert err[pin].max(initial=0.0) < 1e-12
    assert [pr["classes"][j] for j in np.flatnonzero(pin)] == (list(CC.ASYM) if tag == "rock_unc" else [])
    if pin.any():
        sel = np.flatnonzero(pin)
        off = implicit_costs_errors([got[0][:, sel], got[1][:, sel], got[2][sel]],
                                    (g[f"{tag}_ref_dQ"], g[f"{tag}_ref_dP"], g[f"{tag}_ref_dtheta"]))
        assert np.allclose(off, g[f"{tag}_oracle_err"][sel], rtol=1e-6, atol=1e-12)
        assert off.max() > 1e-3


@pytest.mark.parametrize("tag", list(CC.IMPLICIT_COSTS))
def test_implicit_backward_cost_classes(golden, tag):
    """The literal restatement (unit right-hand sides, the dense (T d)^2 solve)
    on the same goldens at test_implicit_backward_f64's bar, per problem.  On
    rocket it runs a second per problem, so there it runs fewer: of the
    unconstrained fixture the four asym classes, the problems pinned to the fast
    algebra, where the literal restatement (the reference's Cholesky engine for
    m > 1) must meet the reference's own stored answer instead; of the boxed
    fixture asym and pair_mid against the golden."""
    g = golden("implicit_costs_f64")
    pr = CC.implicit_costs_problem(g, tag, oracle_true_obj)
    if pr["pinned"].any():
        assert pr["mname"] == "rocket"
        sel = np.flatnonzero(pr["pinned"])
        exp = (g[f"{tag}_ref_dQ"], g[f"{tag}_ref_dP"], g[f"{tag}_ref_dtheta"])
    elif pr["mname"] == "rocket":
        sel = np.array([pr["classes"].index("asym"), pr["classes"].index("pair_mid")])
        exp = (pr["dQ"][:, sel], pr["dP"][:, sel], pr["dtheta"][sel])
    else:
        sel = np.arange(len(pr["classes"]))
        assert not pr["pinned"].any()
        exp = (pr["dQ"], pr["dP"], pr["dtheta"])
    got = implicit_costs_oracle(pr, adjoint.implicit_backward, sel)
    err = implicit_costs_errors(got, exp)
    assert err.max() < 1e-6, dict(zip(np.asarray(pr["classes"])[sel], err.max(1)))


@pytest.mark.parametrize("n,m,T", [(3, 1, 10), (5, 1, 10), (13, 3, 10), (5, 1, 2), (13, 3, 3)])
def test_backward_cost_classes_path_bits(n, m, T):
    """Each class of BACKWARD_CLASSES is what cost_cases' table says: which of
    c_offd, c_dif, cv_dif a bitwise scan of the float32 arrays sets (the kernels'
    first pass, restated in numpy), per problem and, as the rocket kernel
    decides, per row; where the one changed step is; and the first eight
    classes are make_costs' own arrays."""
    mname = {3: "pendulum", 5: "cartpole", 13: "rocket"}[n]
    q, p = oracle_true_obj(mname)
    cls = list(CC.BACKWARD_CLASSES)
    C, c = CC.make_backward_costs(q, p, n, T, cls, 3, sym_uu=m > 1)
    # (make_costs' draws depend on the batch size, so the comparison keeps it)
    C8, c8 = CC.make_costs(q, p, n, T, list(CC.CLASSES) + ["tinv_diag"] * (len(cls) - 8), 3, sym_uu=m > 1)
    assert np.array_equal(C[:, :8], C8[:, :8]) and np.array_equal(c[:, :8], c8[:, :8])
    assert np.array_equal(C, CC.f32(C)) and np.array_equal(c, CC.f32(c))
    bits = CC.path_bits(C, c)
    D = np.diag(CC.f32(q))
    i = CC.PAIR_STATE[n]
    for b, k in enumerate(cls):
        assert tuple(int(v) for v in bits[b].any(0)) == CC.PATH_BITS[k], k
        if k in CC.CLASSES:
            continue
        ts = T // 2 if k.endswith("_mid") else 0
        rest = [t for t in range(T) if t != ts]
        assert np.array_equal(C[rest, b], np.broadcast_to(D, (T - 1, n + m, n + m))), k      # diag(q) off the step
        assert not np.signbit(C[:, b]).any(), k                                        # no -0.0 word
        if k.startswith("diag_t") or k == "diag_mid":
            assert np.array_equal(C[ts, b], CC.f32(1.1 * D)) and (c[:, b] == c[0, b]).all()
        elif k.startswith("c_"):
            assert np.array_equal(C[ts, b], D) and (c[rest, b] == c[rest[0], b]).all()
            assert (c[ts, b] != c[rest[0], b]).any()
        elif k.startswith("pair_"):
            E = C[ts, b] - D
            assert E[i, n] == E[n, i] != 0 and np.count_nonzero(E) == 2 and (c[:, b] == c[0, b]).all()
            # the rocket kernel: only rows i and n leave the register path
            assert np.flatnonzero(bits[b, :, 0] | bits[b, :, 1]).tolist() == [i, n]
            # the stage cost stays convex where the state is free
            assert ts == 0 or np.linalg.eigvalsh(C[ts, b]).min() >= 0
        else:
            assert k == "diag_cvar" and np.array_equal(C[ts, b], D) and (np.diff(c[:, b], axis=0) != 0).any(1).all()
    # pair_t0 is the issue's 0.1
    assert C[0, cls.index("pair_t0"), i, n] == CC.f32(0.1)
