"""CPU checks for the DiLQR implicit backward on a two-hidden-layer network
(csrc/tu_mlp2_implicit.hip, ops.mlp_implicit_backward on an Mlp2Model): the
fp64 yardstick the GPU tests use (tests/mlp2_oracle.py with
tests/mlp_oracle.py's implicit_oracle) is sound, the library and the binding
carry the entry point, and generic.implicit_mlp_ok routes to it behind its
switch.

The yardstick: Mlp2Oracle's Jacobian and Lagrangian Hessian
  M = P^T diag(s o c2) P + W1^T diag(v o c1) W1
against central differences (1e-7; measured at most 2.4e-9 and 5.8e-9), and
implicit_oracle with that M against central differences of polished fp64 solves
along c, x_init and all six weights (1e-5; measured at most 3.1e-10 free and
with 9 of 18 controls on a box bound; a wrong or missing term of M is >= 1e-3)."""
import os
import re

import numpy as np
import pytest

from mlp2_oracle import Mlp2Oracle
from mlp_oracle import implicit_oracle
from oracle import adjoint
from oracle import mpc as ompc
from test_mlp_implicit_cpu import box_of, solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")
N_, M_, H1_, H2_, T_, B_ = 2, 1, 4, 3, 6, 3           # (n, m, T, B) are those test_mlp_implicit_cpu.solve is written for


def draw_model(rng, n, m, H1, H2, act, pt):
    d = n + m
    ws = [0.5 * rng.randn(H1, d), 0.5 * rng.randn(H1), 0.5 * rng.randn(H2, H1), 0.5 * rng.randn(H2),
          0.5 * rng.randn(n, H2), 0.5 * rng.randn(n)]
    return Mlp2Oracle(*ws, act, pt)


# ------------------------------------------------------------------ 1. the formulas
@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
def test_lag_hess_and_jacobian_against_central_differences(pt):
    n, m, H1, H2, R, h = 5, 1, 9, 6, 4, 1e-6
    d = n + m
    rng = np.random.RandomState(3)
    model = draw_model(rng, n, m, H1, H2, "sigmoid", pt)
    tau, lam = rng.randn(R, d), rng.randn(R, n)
    J = model.get_linear_dyn(tau[:, :n], tau[:, n:])
    M = model.lag_hess(tau[:, :n], tau[:, n:], lam)
    Jfd, Mfd = np.zeros_like(J), np.zeros_like(M)
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        tp, tm = tau + e, tau - e
        Jfd[:, :, k] = (model.forward(tp[:, :n], tp[:, n:]) - model.forward(tm[:, :n], tm[:, n:])) / (2 * h)
        Jp, Jm = model.get_linear_dyn(tp[:, :n], tp[:, n:]), model.get_linear_dyn(tm[:, :n], tm[:, n:])
        Mfd[:, :, k] = np.einsum("ri,rij->rj", lam, Jp - Jm) / (2 * h)
    eJ = float(np.abs(J - Jfd).max() / np.abs(Jfd).max())
    eM = float(np.abs(M - Mfd).max() / np.abs(Mfd).max())
    print(f"\n[mlp2 oracle vs central differences, pt={pt}] get_linear_dyn {eJ:.1e}, lag_hess {eM:.1e}")
    assert eJ <= 1e-7 and eM <= 1e-7, (eJ, eM)
    assert np.abs(M - np.swapaxes(M, 1, 2)).max() <= 1e-14 * np.abs(M).max()
    # either term alone is not M
    for kw in ({"first": False}, {"second": False}):
        part = model.lag_hess(tau[:, :n], tau[:, n:], lam, **kw)
        assert np.abs(part - Mfd).max() > 1e-3 * np.abs(Mfd).max()


def test_relu_lag_hess_is_zero():
    rng = np.random.RandomState(4)
    model = draw_model(rng, 5, 1, 9, 6, "relu", True)
    tau, lam = rng.randn(4, 6), rng.randn(4, 5)
    M = model.lag_hess(tau[:, :5], tau[:, 5:], lam)
    assert M.shape == (4, 6, 6) and not M.any()
    assert model.astype(np.float32).forward(tau[:, :5].astype(np.float32), tau[:, 5:].astype(np.float32)).dtype \
        == np.float32


# ------------------------------------------------------------------ 2. the derivative of the fixed point
def problem():
    rng = np.random.RandomState(0)
    d = N_ + M_
    model = draw_model(rng, N_, M_, H1_, H2_, "sigmoid", True)
    L = rng.randn(T_, B_, d, d)
    C = L @ np.swapaxes(L, 2, 3) + np.eye(d)
    c = 0.3 * rng.randn(T_, B_, d)
    x0 = 0.3 * rng.randn(B_, N_)
    wx, wu = rng.randn(T_, B_, N_), rng.randn(T_, B_, M_)
    return model, x0, C, c, wx, wu


@pytest.mark.parametrize("box", [False, True], ids=["free", "box"])
def test_oracle_is_the_derivative_of_the_fixed_point(box):
    model, x0, C, c, wx, wu = problem()
    lo, hi = box_of(model, x0, C, c) if box else (None, None)
    x, u = solve(model, x0, C, c, lo, hi)
    if box:
        act = adjoint._active_set(u, lo, hi)
        print(f"\n[mlp2 implicit] {int(act.sum())} of {act.size} controls on a bound")
        assert 0 < act.sum() < act.size, act.sum()
    dx0, dC, dc, dF, df = implicit_oracle(model, wx, wu, C, c, x, u, lo, hi)
    h = 1e-6
    rng = np.random.RandomState(5)

    def loss(md, x0_, c_):
        xs, us = solve(md, x0_, C, c_, lo, hi)
        return (xs * wx).sum() + (us * wu).sum()

    def report(tag, an, fd):
        err = abs(an - fd) / abs(fd)
        print(f"\n[mlp2 implicit vs central differences, {tag}, {'box' if box else 'free'}] {an:.9f} vs {fd:.9f} "
              f"rel {err:.1e}")
        assert err <= 1e-5, (tag, an, fd)

    for k in range(2):
        v = rng.randn(*c.shape)
        fd = (loss(model, x0, c + h * v) - loss(model, x0, c - h * v)) / (2 * h)
        report(f"c direction {k}", float((dc * v).sum()), fd)
    v = rng.randn(*x0.shape)
    fd = (loss(model, x0 + h * v, c) - loss(model, x0 - h * v, c)) / (2 * h)
    report("x_init", float((dx0 * v).sum()), fd)
    # one joint direction in all six weights: (dF, df) contracted with the
    # differences of the linearisation at the fixed (x, u)
    vs = [rng.randn(*w.shape) for w in model.weights()]
    mp = model.with_weights([w + h * v for w, v in zip(model.weights(), vs)])
    mm = model.with_weights([w - h * v for w, v in zip(model.weights(), vs)])
    (Fp, fp), (Fm, fm) = ompc.linearize(mp, x, u), ompc.linearize(mm, x, u)
    an = float((dF * (Fp - Fm)).sum() + (df * (fp - fm)).sum()) / (2 * h)
    fd = (loss(mp, x0, c) - loss(mm, x0, c)) / (2 * h)
    report("six weights", an, fd)


# ------------------------------------------------------------------ 3. library and binding
def test_library_and_binding_carry_the_entry_point():
    import torch
    from dilqr import _native as N
    from dilqr import ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = N.lib()
    name = "dilqr_mlp2_implicit_backward_f32"
    assert re.search(r"\bint\s+" + name + r"\s*\(", src) and hasattr(lib, name) and name in N.SIGNATURES
    assert len(N.SIGNATURES[name][0]) == len(N.SIGNATURES["dilqr_mlp_implicit_backward_f32"][0])
    assert lib.dilqr_version() == 11 and N.ABI_VERSION == 11
    cap = N.MLP2_IMPLICIT_MAX_HIDDEN1
    assert re.search(r"#define\s+DILQR_MLP2_IMPLICIT_MAX_HIDDEN1\s+%d\b" % cap, src)
    assert cap >= 64                                            # [64, 64], the reference's network
    # a1 with v, or with the staging area of the largest (n, m), within the 64 KiB of a launch
    assert 256 * cap + max(256 * cap, 256 * max(n + m for n, m in N.LANE_SHAPES) ** 2) <= 65536
    # the descriptor's and the pointers' checks, before any launch
    n, m, H1, H2, T, B = 5, 1, 8, 6, 4, 3
    p16 = 16
    good = dict(n=n, m=m, T=T, B=B, H1=H1, H2=H2, act=N.MLP_SIGMOID, W1=p16, W3=p16, C=p16, dF=p16, df=p16,
                dx_init=p16, ws=p16, mode=N.BOUNDS_NONE)

    def call(**kw):
        a = dict(good, **kw)
        mlp = N.Mlp2(a["H1"], a["H2"], a["act"], 1, a["W1"], p16, p16, p16, a["W3"], p16)
        return lib.dilqr_mlp2_implicit_backward_f32(a["n"], a["m"], a["T"], a["B"], mlp, a["C"], p16, p16, p16, p16,
                                                    p16, N.Bounds(a["mode"], 0.0, 0.0, None, None), a["ws"],
                                                    a["dx_init"], p16, p16, a["dF"], a["df"], None)

    assert call(B=0) == 0 and call(B=0, dF=None, df=None) == 0 and call(B=0, H1=cap) == 0
    for kw, rc in (({"C": None}, 2), ({"C": 4}, 2), ({"ws": None}, 2), ({"dx_init": None}, 2), ({"dF": None}, 2),
                   ({"df": 8}, 2), ({"T": 0}, 2), ({"B": -1}, 2), ({"mode": 7}, 2), ({"W1": None}, 2),
                   ({"W3": 4}, 2), ({"n": 7}, 1), ({"H1": 0}, 1), ({"H2": 0}, 1), ({"H2": N.MLP_MAX_HIDDEN + 1}, 1),
                   ({"H1": cap + 1}, 1), ({"H1": cap + 1, "B": 0}, 1), ({"act": 2}, 3)):
        assert call(**kw) == rc, (kw, rc)
    # ops: mis-shaped arguments raise on the host (CPU tensors: nothing is launched)

    def model(h1):
        return ops.Mlp2Model(n, m, N.MLP_SIGMOID, True, torch.zeros(h1, n + m), torch.zeros(h1), torch.zeros(H2, h1),
                             torch.zeros(H2), torch.zeros(n, H2), torch.zeros(n))

    md = model(H1)
    assert md.implicit_ok and model(cap).implicit_ok and not model(cap + 1).implicit_ok
    ok = dict(dl_dx=torch.zeros(T, B, n), dl_du=torch.zeros(T, B, m), C=torch.zeros(T, B, n + m, n + m),
              c=torch.zeros(T, B, n + m), x=torch.zeros(T, B, n), u=torch.zeros(T, B, m), u_lower=None, u_upper=None)
    for k, bad in (("dl_dx", torch.zeros(T, B, n + 1)), ("dl_du", torch.zeros(T - 1, B, m)),
                   ("C", torch.zeros(T, B, n + m, n)), ("c", torch.zeros(T, B + 1, n + m)),
                   ("x", torch.zeros(T * B, n)), ("x", torch.zeros(T, B, n + 1)), ("u", torch.zeros(T, B, m + 1)),
                   ("u_lower", -1.0), ("u_upper", torch.zeros(T, B))):
        with pytest.raises(ValueError):
            ops.mlp_implicit_backward(md, **dict(ok, **{k: bad}))
    with pytest.raises(ValueError, match="H1 <= %d" % cap):
        ops.mlp_implicit_backward(model(cap + 1), **ok)
    with pytest.raises(TypeError):
        ops.mlp_implicit_backward(object(), **ok)
    with pytest.raises(TypeError):
        ops.mlp_implicit_backward(md, **dict(ok, C=ok["C"].double()))


# ------------------------------------------------------------------ 4. routing
SWITCHES = ("DEVICE_MLP", "DEVICE_MLP_DEEP", "DEVICE_MLP_IMPLICIT", "DEVICE_MLP_DEEP_IMPLICIT")


def test_routing_switches_and_envelope(monkeypatch):
    """generic.implicit_mlp_ok: the Mlp2Model for a two-hidden-layer module on
    GPU fp32 tensors inside the envelope with all four switches on, None
    otherwise (`is_cuda` faked: the routing reads nothing else of the tensor)."""
    import torch
    import dilqr
    from dilqr import _native as N
    from dilqr import generic, ops
    from dilqr.dynamics import NNDynamics

    class Like:
        is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

    cap = N.MLP2_IMPLICIT_MAX_HIDDEN1
    cost = dilqr.QuadCost(torch.zeros(4, 2, 6, 6), torch.zeros(4, 2, 6))
    dx = NNDynamics(5, 1, [8, 8], activation="sigmoid")
    ok = lambda mpc, cost_=cost, dx_=dx: generic.implicit_mlp_ok(mpc, cost_, dx_, Like())   # noqa: E731
    # default flags: the new switch ships off, and nothing is routed
    assert generic.DEVICE_MLP_DEEP_IMPLICIT is False and generic.DEVICE_MLP_DEEP is False
    assert ok(dilqr.MPC(5, 1, 4)) is None
    for name in SWITCHES:
        monkeypatch.setattr(generic, name, True)
    md = ok(dilqr.MPC(5, 1, 4))
    assert isinstance(md, ops.Mlp2Model) and (md.n, md.m, md.H1, md.H2) == (5, 1, 8, 8)
    assert isinstance(ok(dilqr.MPC(5, 1, 4), dx_=NNDynamics(5, 1, [cap, 8], activation="relu")), ops.Mlp2Model)
    # one hidden layer goes on as before
    assert isinstance(ok(dilqr.MPC(5, 1, 4), dx_=NNDynamics(5, 1, [8])), ops.MlpModel)
    assert ok(dilqr.MPC(5, 1, 4), dx_=NNDynamics(5, 1, [cap + 1, 8])) is None
    assert ok(dilqr.MPC(5, 1, 4), dx_=NNDynamics(5, 1, [8, 8, 8])) is None
    assert ok(dilqr.MPC(5, 1, 4), dx_=NNDynamics(5, 1, [8, 8], activation="elu")) is None
    assert ok(dilqr.MPC(5, 1, 4, slew_rate_penalty=0.1)) is None
    assert ok(dilqr.MPC(5, 1, 4, u_lower=-1.0, u_upper=1.0, delta_u=0.1)) is None
    assert ok(dilqr.MPC(5, 1, 4, u_zero_I=torch.zeros(4, 2, 1, dtype=torch.bool))) is None
    assert ok(dilqr.MPC(5, 1, 4, grad_method=dilqr.GradMethods.AUTO_DIFF)) is None
    assert ok(dilqr.MPC(5, 1, 4), cost_=torch.nn.Identity()) is None
    assert ok(dilqr.MPC(4, 2, 4)) is None
    for name in SWITCHES:
        with monkeypatch.context() as mp:
            mp.setattr(generic, name, False)
            assert ok(dilqr.MPC(5, 1, 4)) is None, name
