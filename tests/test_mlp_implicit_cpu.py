"""CPU checks for the DiLQR implicit backward on a one-hidden-layer network
(csrc/tu_mlp_implicit.hip, ops.mlp_implicit_backward): the fp64 yardstick the
GPU tests use (tests/mlp_oracle.py) is sound, and the library and the binding
carry the new entry points.

The yardstick: oracle.adjoint.implicit_backward_fast on MlpOracle (explicit
partials only) equals the literal (T d)^2 restatement to 1e-12, and is the
derivative of a converged solve (central differences of oracle.mpc.mpc_forward
along weight directions, 2e-3: the solver's convergence noise over a 2e-6
difference, not a precision claim)."""
import os
import re

import numpy as np
import pytest

from mlp_oracle import MlpOracle, implicit_oracle
from oracle import adjoint, lqr
from oracle import mpc as ompc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")
N_, M_, H_, T_, B_ = 2, 1, 4, 6, 3
SOLVE = dict(lqr_iter=200, eps=1e-13, best_cost_eps=0.0)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def problem(act, seed=0):
    rng = np.random.RandomState(seed)
    d = N_ + M_
    model = MlpOracle(0.5 * rng.randn(H_, d), 0.5 * rng.randn(H_), 0.5 * rng.randn(N_, H_), 0.5 * rng.randn(N_),
                      act, True)
    L = rng.randn(T_, B_, d, d)
    C = L @ np.swapaxes(L, 2, 3) + np.eye(d)
    c = 0.3 * rng.randn(T_, B_, d)
    x0 = 0.3 * rng.randn(B_, N_)
    wx, wu = rng.randn(T_, B_, N_), rng.randn(T_, B_, M_)
    return model, x0, C, c, wx, wu


def solve(model, x0, C, c, lo, hi, polish=60):
    """mpc_forward, then the same iLQR iteration judged by its own residual.
    The line search accepts a step only while the cost still falls, which fp64
    resolves down to steps of about 1e-8, and the box QP stops at steps of 1e-4
    (pnqp.py:56); central differences over 2e-6 need the fixed point closer
    than that.  So, with the active set the solve ended on held fixed (the
    masked Riccati solve, exact), the iteration goes on with, per problem, the
    largest step in {1, 1/2, ..} after which the next full step is shorter than
    this one (the fixed-point residual falls), until nothing is left."""
    x, u, _, info = ompc.mpc_forward(model, x0, C, c, T_, u_lower=lo, u_upper=hi, **SOLVE)
    I = adjoint._active_set(u, lo, hi)

    def stepper(x, u):
        F, _ = ompc.linearize(model, x, u)
        K, k, _ = lqr.lqr_backward(C, lqr.c_back(C, c, x, u), F, N_, M_, u_zero_I=I)

        def roll(al):
            xs, us, dx = [x0], [], np.zeros_like(x0)
            for t in range(T_):
                ut = u[t] + al[:, None] * k[t] + lqr.bmv(K[t], dx)
                us.append(ut if I is None else np.where(I[t], u[t], ut))
                if t < T_ - 1:
                    xs.append(model.forward(xs[t], us[t]))
                    dx = xs[t + 1] - x[t + 1]
            return np.stack(xs), np.stack(us)
        return roll

    def residual(x, u):
        return np.abs(stepper(x, u)(np.ones(B_))[1] - u).max((0, 2))

    res = residual(x, u)
    for _ in range(polish):
        roll = stepper(x, u)
        done = np.zeros(B_, bool)
        for al in (1.0, 0.5, 0.25, 0.125):
            xn, un = roll(np.full(B_, al))
            rn = residual(xn, un)
            take = ~done & (rn < res)
            x[:, take], u[:, take], res[take] = xn[:, take], un[:, take], rn[take]
            done |= take
        if not done.any():
            break
    return x, u


def box_of(model, x0, C, c):
    """A box that binds about half of the controls: the median magnitude of the free solve's."""
    _, u = solve(model, x0, C, c, None, None)
    b = float(np.round(np.median(np.abs(u)), 2))
    return -b, b


@pytest.fixture(scope="module", params=[False, True], ids=["free", "box"])
def solved(request):
    """A converged fp64 solve on the sigmoid network, and the fast backward at it."""
    model, x0, C, c, wx, wu = problem("sigmoid")
    lo, hi = box_of(model, x0, C, c) if request.param else (None, None)
    x, u = solve(model, x0, C, c, lo, hi)
    F, f = ompc.linearize(model, x, u)
    fast = adjoint.implicit_backward_fast(model, wx, wu, C, c, F, f, x, u, None, lo, hi)
    return dict(model=model, x0=x0, C=C, c=c, wx=wx, wu=wu, lo=lo, hi=hi, x=x, u=u, F=F, f=f, fast=fast)


def test_box_leaves_some_controls_active(solved):
    if solved["lo"] is None:
        return
    act = adjoint._active_set(solved["u"], solved["lo"], solved["hi"])
    assert 0 < act.sum() < act.size, act.sum()


def test_fast_equals_literal(solved):
    s = solved
    lit = adjoint.implicit_backward(s["model"], s["wx"], s["wu"], s["C"], s["c"], s["F"], s["f"], s["x"], s["u"],
                                    None, s["lo"], s["hi"])
    errs = [rel(a, b) for a, b in zip(s["fast"], lit)]
    print("\n[mlp implicit fast vs literal] dC %.1e dc %.1e dtheta %.1e" % tuple(errs))
    assert max(errs) < 1e-12, errs


def test_oracle_with_every_output_equals_fast(solved):
    """implicit_oracle (dx_init, dF and df besides) is the same computation, and
    param_vjp of its (dF, df) is the fast backward's dtheta."""
    s = solved
    dx0, dC, dc, dF, df = implicit_oracle(s["model"], s["wx"], s["wu"], s["C"], s["c"], s["x"], s["u"], s["lo"],
                                          s["hi"])
    assert rel(dC, s["fast"][0]) < 1e-12 and rel(dc, s["fast"][1]) < 1e-12
    dth = np.concatenate([g.ravel() for g in s["model"].param_vjp(s["x"], s["u"], dF, df)])
    assert rel(dth, s["fast"][2].sum(0)) < 1e-12
    assert dx0.shape == (B_, N_) and dF.shape == (T_ - 1, B_, N_, N_ + M_) and df.shape == (T_ - 1, B_, N_)


def test_is_the_derivative_of_the_fixed_point(solved):
    s = solved
    model, th = s["model"], s["model"].theta()
    dth = s["fast"][2].sum(0)
    rng = np.random.RandomState(5)
    h = 1e-6
    for k in range(3):
        v = rng.randn(th.size)
        L = []
        for sgn in (1, -1):
            x, u = solve(model.with_theta(th + sgn * h * v), s["x0"], s["C"], s["c"], s["lo"], s["hi"])
            L.append((x * s["wx"]).sum() + (u * s["wu"]).sum())
        fd, an = (L[0] - L[1]) / (2 * h), float(dth @ v)
        print(f"\n[mlp implicit vs central differences, direction {k}] {an:.6f} vs {fd:.6f} "
              f"rel {abs(an - fd) / abs(fd):.1e}")
        assert abs(an - fd) <= 2e-3 * abs(fd), (an, fd)


@pytest.mark.parametrize("box", [False, True], ids=["free", "box"])
def test_relu_is_the_classic_adjoint(box):
    """act'' = 0: M = 0, and the implicit derivative is the classic one."""
    model, x0, C, c, wx, wu = problem("relu", seed=1)
    lo, hi = box_of(model, x0, C, c) if box else (None, None)
    x, u = solve(model, x0, C, c, lo, hi)
    if box:
        act = adjoint._active_set(u, lo, hi)
        assert 0 < act.sum() < act.size, act.sum()
    F, f = ompc.linearize(model, x, u)
    dC, dc, dth = adjoint.implicit_backward_fast(model, wx, wu, C, c, F, f, x, u, None, lo, hi)
    _, cC, cc, cF, cf = adjoint.classic_backward(wx, wu, x0, C, c, F, f, x, u, lo, hi)
    assert rel(dC, cC) < 1e-12 and rel(dc, cc) < 1e-12
    gD, gd = model.grad_input(x, u)[:2]
    cth = np.einsum("tbnm,tbnmk->k", cF, gD) + np.einsum("tbn,tbnk->k", cf, gd)
    assert rel(dth.sum(0), cth) < 1e-12
    assert rel(np.concatenate([g.ravel() for g in model.param_vjp(x, u, cF, cf)]), cth) < 1e-12


def test_library_and_binding_carry_the_entry_points():
    import torch
    from dilqr import _native as N
    from dilqr import ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = N.lib()
    for name in ("dilqr_mlp_implicit_backward_f32", "dilqr_mlp_implicit_ws_floats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src) and hasattr(lib, name) and name in N.SIGNATURES
    assert lib.dilqr_version() == 11 and N.ABI_VERSION == 11
    for n, m in N.LANE_SHAPES:
        assert lib.dilqr_mlp_implicit_ws_floats(n, m) == (m * n + m) + (n + m) + 4
    assert lib.dilqr_mlp_implicit_ws_floats(7, 1) == -1
    # the descriptor's and the pointers' checks, before any launch
    n, m, H, T, B = 5, 1, 8, 4, 3
    p16 = 16
    good = dict(n=n, m=m, T=T, B=B, H=H, act=N.MLP_SIGMOID, W1=p16, C=p16, dF=p16, df=p16, dx_init=p16, ws=p16,
                mode=N.BOUNDS_NONE)

    def call(**kw):
        a = dict(good, **kw)
        mlp = N.Mlp(a["H"], a["act"], 1, a["W1"], p16, p16, p16)
        return lib.dilqr_mlp_implicit_backward_f32(a["n"], a["m"], a["T"], a["B"], mlp, a["C"], p16, p16, p16, p16,
                                                   p16, N.Bounds(a["mode"], 0.0, 0.0, None, None), a["ws"],
                                                   a["dx_init"], p16, p16, a["dF"], a["df"], None)

    assert call(B=0) == 0 and call(B=0, dF=None, df=None) == 0
    for kw, rc in (({"C": None}, 2), ({"C": 4}, 2), ({"ws": None}, 2), ({"dx_init": None}, 2), ({"dF": None}, 2),
                   ({"df": 8}, 2), ({"T": 0}, 2), ({"B": -1}, 2), ({"mode": 7}, 2), ({"W1": None}, 2),
                   ({"n": 7}, 1), ({"H": 0}, 1), ({"H": N.MLP_MAX_HIDDEN + 1}, 1), ({"act": 2}, 3)):
        assert call(**kw) == rc, (kw, rc)
    # ops: mis-shaped arguments raise on the host (CPU tensors: nothing is launched)
    md = ops.MlpModel(n, m, N.MLP_SIGMOID, True, torch.zeros(H, n + m), torch.zeros(H), torch.zeros(n, H),
                      torch.zeros(n))
    ok = dict(dl_dx=torch.zeros(T, B, n), dl_du=torch.zeros(T, B, m), C=torch.zeros(T, B, n + m, n + m),
              c=torch.zeros(T, B, n + m), x=torch.zeros(T, B, n), u=torch.zeros(T, B, m), u_lower=None, u_upper=None)
    for k, bad in (("dl_dx", torch.zeros(T, B, n + 1)), ("dl_du", torch.zeros(T - 1, B, m)),
                   ("C", torch.zeros(T, B, n + m, n)), ("c", torch.zeros(T, B + 1, n + m)),
                   ("x", torch.zeros(T * B, n)), ("x", torch.zeros(T, B, n + 1)), ("u", torch.zeros(T, B, m + 1)),
                   ("u_lower", -1.0), ("u_upper", torch.zeros(T, B))):
        with pytest.raises(ValueError):
            ops.mlp_implicit_backward(md, **dict(ok, **{k: bad}))
    with pytest.raises(TypeError):
        ops.mlp_implicit_backward(object(), **ok)
    with pytest.raises(TypeError):
        ops.mlp_implicit_backward(md, **dict(ok, C=ok["C"].double()))


def test_routing_switch_and_envelope(monkeypatch):
    """generic.implicit_mlp_ok: the device model for a one-hidden-layer module
    on GPU fp32 tensors inside the envelope, None otherwise (`is_cuda` faked:
    the routing reads nothing else of the tensor)."""
    import torch
    import dilqr
    from dilqr import generic, ops
    from dilqr.dynamics import NNDynamics

    class Like:
        is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    assert generic.DEVICE_MLP_IMPLICIT is True
    cost = dilqr.QuadCost(torch.zeros(4, 2, 6, 6), torch.zeros(4, 2, 6))
    dx = NNDynamics(5, 1, [8], activation="sigmoid")
    assert isinstance(generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4), cost, dx, Like()), ops.MlpModel)
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4), cost, NNDynamics(5, 1, [8, 8]), Like()) is None
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4), cost, NNDynamics(5, 1, [8], activation="elu"), Like()) is None
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4, slew_rate_penalty=0.1), cost, dx, Like()) is None
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4, u_lower=-1.0, u_upper=1.0, delta_u=0.1), cost, dx, Like()) is None
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4, u_zero_I=torch.zeros(4, 2, 1, dtype=torch.bool)), cost, dx,
                                   Like()) is None
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4, grad_method=dilqr.GradMethods.AUTO_DIFF), cost, dx,
                                   Like()) is None
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4), torch.nn.Identity(), dx, Like()) is None
    assert generic.implicit_mlp_ok(dilqr.MPC(4, 2, 4), cost, dx, Like()) is None
    monkeypatch.setattr(generic, "DEVICE_MLP_IMPLICIT", False)
    assert generic.implicit_mlp_ok(dilqr.MPC(5, 1, 4), cost, dx, Like()) is None
