"""CPU checks of the device route of NNDynamics solves with a slew-rate penalty
or with delta_u (generic.DEVICE_MLP_SLEW, generic.DEVICE_MLP_DELTA_U, both
shipped off): the routing rules of dilqr.generic with the switches off and on,
ops.slew_problem against generic.slew_augment, the dilqr_mlp_slew_* /
dilqr_mlp2_slew_* entry points' argument validation (errors return before any
launch, so no GPU is needed), the binding against the header and
ops.mpc_solve_unfused's refusal of delta_u without bounds."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")
CALLS = ("rollout", "linearize", "lqr_forward")
NAMES = [f"dilqr_{kind}_slew_{call}_f32" for kind in ("mlp", "mlp2") for call in CALLS]


class _Taken(Exception):
    pass


class FakeCuda(torch.Tensor):
    is_cuda = True


# ------------------------------------------------------------------ binding
def test_binding_matches_header():
    from dilqr import _native as N
    raw = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = N.lib()
    assert lib.dilqr_version() == N.ABI_VERSION
    for name in NAMES:
        assert hasattr(lib, name), name
        decl = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", src, re.S)
        assert decl, name
        plain = re.search(rf"\bint\s+{name.replace('_slew', '')}\s*\((.*?)\)\s*;", src, re.S)
        # the argument list of the plain counterpart, in the header and in the binding
        assert re.sub(r"\s+", " ", decl.group(1)) == re.sub(r"\s+", " ", plain.group(1)), name
        assert N.SIGNATURES[name] == N.SIGNATURES[name.replace("_slew", "")], name
        assert len(N.SIGNATURES[name][0]) == decl.group(1).count(",") + 1, name
    # the comments of the new family cite the reference
    block = raw[raw.index("learned dynamics under the slew-rate augmentation"):]
    assert block.count("dynamics.py:133-156") >= 2 and block.count("mpc_explicit.py:383-466") >= 2
    # the shape list did not change
    assert N.LANE_SHAPES == ((3, 1), (5, 1), (4, 3), (4, 1), (2, 1), (4, 2), (6, 2), (6, 1))


# ------------------------------------------------------------------ argument checks
def _calls(N, kind, n=5, m=1, H=32, H2=16, act=0, W=16, x=16, T=4, B=65, max_ls=10, bounds=None, which=None):
    """The three slew entry points of a kind with fake (never dereferenced)
    pointers; W: the value of the weight pointer `which` (all others 16)."""
    lib = N.lib()
    P = ctypes.c_void_p
    nw = 4 if kind == "mlp" else 6
    ws = [16] * nw
    if which is not None:
        ws[which] = W
    d = N.Mlp(H, act, 1, *ws) if kind == "mlp" else N.Mlp2(H, H2, act, 1, *ws)
    nb = bounds or N.Bounds(N.BOUNDS_NONE, 0.0, 0.0, None, None)
    p = P(16)
    f = {call: getattr(lib, f"dilqr_{kind}_slew_{call}_f32") for call in CALLS}
    return {
        "rollout": f["rollout"](n, m, T, B, d, P(x), p, p, None),
        "linearize": f["linearize"](n, m, T, B, d, P(x), p, p, p, None),
        "lqr_forward": f["lqr_forward"](n, m, T, B, d, P(x), p, p, p, p, p, p, nb, None, 0.2, max_ls, p, p, p, p, p,
                                        None, None),
    }


@pytest.mark.parametrize("kind", ["mlp", "mlp2"])
def test_slew_entry_points_reject_bad_arguments_without_launch(kind):
    """Null / misaligned pointers -> 2, a base (n, m) without an augmented shape
    or a width outside [1, 256] -> 1, unknown activation -> 3, an empty batch ->
    0, each before any kernel launch (this runs without a GPU)."""
    from dilqr import _native as N
    E_SHAPE, E_ARG, E_MODE = 1, 2, 3
    for which in range(4 if kind == "mlp" else 6):
        for bad in (None, 4, 8, 20):
            assert set(_calls(N, kind, which=which, W=bad).values()) == {E_ARG}, (which, bad)
    for kw in ({"x": None}, {"x": 4}):
        assert set(_calls(N, kind, **kw).values()) == {E_ARG}, kw
    # base shapes whose (n + m, m) the one-lane kernels are not compiled for
    for n, m in ((4, 3), (6, 1), (6, 2), (13, 3), (7, 3), (0, 1), (5, 0), (-1, -1), (2 ** 31 - 1, 1)):
        assert set(_calls(N, kind, n=n, m=m).values()) == {E_SHAPE}, (n, m)
    widths = ({"H": 0}, {"H": N.MLP_MAX_HIDDEN + 1}) + (({"H2": 0}, {"H2": N.MLP_MAX_HIDDEN + 1}) if kind == "mlp2"
                                                        else ())
    for kw in widths:
        assert set(_calls(N, kind, **kw).values()) == {E_SHAPE}, kw
    for kw in ({"act": 2}, {"act": -1}):
        assert set(_calls(N, kind, **kw).values()) == {E_MODE}, kw
    # a pointer error is reported before a shape error, as for the plain entry points
    assert set(_calls(N, kind, n=6, m=2, x=4).values()) == {E_ARG}
    # sizes and options, as dilqr_mlp_entry.h checks them
    assert _calls(N, kind, max_ls=0)["lqr_forward"] == E_ARG
    assert _calls(N, kind, bounds=N.Bounds(N.BOUNDS_TENSOR, 0.0, 0.0, None, None))["lqr_forward"] == E_ARG
    assert set(_calls(N, kind, T=0).values()) == {E_ARG}
    assert set(_calls(N, kind, B=-1).values()) == {E_ARG}
    # an empty batch, or T = 1 for the linearisation, is valid and launches nothing: every served base shape
    for n, m in ((2, 1), (3, 1), (4, 1), (5, 1), (4, 2)):
        assert set(_calls(N, kind, n=n, m=m, B=0).values()) == {0}, (n, m)
        assert _calls(N, kind, n=n, m=m, T=1)["linearize"] == 0


# ------------------------------------------------------------------ the handle
@pytest.mark.parametrize("hidden", [[8], [8, 4]], ids=["one", "two"])
def test_slew_dynamics_handle(hidden):
    from dilqr import ops
    from dilqr.dynamics import NNDynamics
    like = torch.zeros(1)
    for n, m in ((2, 1), (3, 1), (4, 1), (5, 1), (4, 2)):
        md = NNDynamics(n, m, hidden_sizes=hidden).device_model(like, deep=True)
        dyn = ops.slew_dynamics(md)
        assert isinstance(dyn, ops.Dynamics) and (dyn.n, dyn.m) == (n + m, m) and dyn.mlp is md and dyn.slew
        assert dyn._entry == md.entry + "slew_"
        assert dyn._head(7, 9)[:4] == (n, m, 7, 9)                 # the entry points take the network's (n, m)
        assert ops.mlp_solve_route(dyn, 65, 4, None, 0) == "unfused"
        # it stands where a handle does, at the augmented width only
        assert ops.Dynamics.of(dyn, None, n + m, m) is dyn
        with pytest.raises(ValueError):
            ops.Dynamics.of(dyn, None, n, m)
        with pytest.raises(ValueError, match="slew-rate"):
            dyn.check(torch.zeros(3, n), torch.zeros(3, m))
        dyn.check(torch.zeros(3, n + m), torch.zeros(3, m))
    for n, m in ((4, 3), (6, 1), (6, 2)):
        assert ops.slew_dynamics(NNDynamics(n, m, hidden_sizes=hidden).device_model(like, deep=True)) is None
    # the plain handle of the same model is not a slew handle
    md = NNDynamics(5, 1, hidden_sizes=hidden).device_model(like, deep=True)
    assert ops.Dynamics(md, 5, 1).slew is False
    with pytest.raises(TypeError):
        ops.slew_dynamics(None)


# ------------------------------------------------------------------ slew_problem
@pytest.mark.parametrize("prev", ["none", "m", "Bm", "1Bm"])
@pytest.mark.parametrize("nm", [(5, 1), (4, 2)], ids=["5x1", "4x2"])
def test_slew_problem_is_slew_augment(nm, prev):
    from dilqr import generic, ops
    from dilqr.definitions import QuadCost
    from dilqr.dynamics import NNDynamics
    n, m = nm
    T, B, d = 4, 3, n + m
    gen = torch.Generator().manual_seed(7)
    x_init, C, c = torch.randn(B, n, generator=gen), torch.randn(T, B, d, d, generator=gen), torch.randn(T, B, d, generator=gen)
    F, f = torch.randn(T - 1, B, n, d, generator=gen), torch.randn(T - 1, B, n, generator=gen)
    x, u = torch.randn(T, B, n, generator=gen), torch.randn(T, B, m, generator=gen)
    prev_ctrl = {"none": None, "m": torch.randn(m, generator=gen), "Bm": torch.randn(B, m, generator=gen),
                 "1Bm": torch.randn(1, B, m, generator=gen)}[prev]
    mpc = types.SimpleNamespace(T=T, n_state=n, n_ctrl=m, slew_rate_penalty=0.37, prev_ctrl=prev_ctrl)
    _x_init, _C, _c, _F, _f, _dyn, _cost, _x = generic.slew_augment(mpc, x_init, C, c, F, f, QuadCost(C, c),
                                                                   NNDynamics(n, m, hidden_sizes=[4]), x, u)
    x0, Ca, ca = ops.slew_problem(x_init, C, c, 0.37, prev_ctrl, m)
    assert torch.equal(x0, _x_init) and torch.equal(Ca, _C) and torch.equal(ca, _c)
    assert x0.shape == (B, n + m) and Ca.shape == (T, B, d + m, d + m) and ca.shape == (T, B, d + m)
    # the augmentation as the issue states it, independently of slew_augment
    want = torch.zeros(T, B, d + m, d + m)
    want[:, :, m:, m:] = C
    eye = 0.37 * torch.eye(m)
    want[:, :, :m, :m] += eye
    want[:, :, -m:, -m:] += eye
    want[:, :, :m, -m:] -= eye
    want[:, :, -m:, :m] -= eye
    assert torch.allclose(Ca, want, rtol=0, atol=1e-6)
    assert torch.equal(ca[:, :, :m], torch.zeros(T, B, m)) and torch.equal(ca[:, :, m:], c)
    p = torch.zeros(B, m) if prev_ctrl is None else prev_ctrl.reshape(-1, m).expand(B, m)
    assert torch.equal(x0[:, :m], p) and torch.equal(x0[:, m:], x_init)


# ------------------------------------------------------------------ routing of the solve
@pytest.fixture
def routed(monkeypatch):
    """generic.solve with ops.mpc_solve_unfused replaced by a stub that tells
    what it was handed and ends the call, and the torch loop's first step (the
    rollout) by another (tests/test_mlp_cpu.py's technique: FakeCuda tensors
    stand in for GPU ones)."""
    from dilqr import generic, ops

    def stub(model_id, theta, x_init, C, c, T, delta_u=None, **k):
        if isinstance(model_id, ops.MLP_MODELS):
            raise _Taken("device")
        assert isinstance(model_id, ops.Dynamics) and model_id.mlp is not None and theta is None
        n, m = model_id.mlp.n, model_id.mlp.m
        if model_id.slew:
            assert delta_u is None
            assert tuple(x_init.shape) == (3, n + m) and tuple(C.shape) == (T, 3, n + 2 * m, n + 2 * m)
            assert tuple(c.shape) == (T, 3, n + 2 * m)
            raise _Taken("device:slew")
        assert delta_u is not None and tuple(x_init.shape) == (3, n) and tuple(C.shape) == (T, 3, n + m, n + m)
        raise _Taken(f"device:delta_u={delta_u}")

    def torch_loop(*a, **k):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "mpc_solve_unfused", stub)
    monkeypatch.setattr(generic, "rollout", torch_loop)

    def route(dx, cost, n=5, m=1, **mpc_kw):
        from dilqr.mpc_explicit import GradMethods
        kw = dict(T=4, n_state=n, n_ctrl=m, u_init=None, u_lower=-1.0, u_upper=1.0, lqr_iter=3, eps=1e-7,
                  grad_method=GradMethods.ANALYTIC, slew_rate_penalty=None, delta_u=None, prev_ctrl=None, verbose=0,
                  linesearch_decay=0.2, max_linesearch_iter=10, not_improved_lim=5, best_cost_eps=1e-4)
        kw.update(mpc_kw)
        x0 = torch.zeros(3, n).as_subclass(FakeCuda)
        with pytest.raises(_Taken) as e:
            generic.solve(types.SimpleNamespace(**kw), x0, cost, dx, 3)
        return str(e.value)

    return route


def test_solve_routing_with_the_switches(routed, monkeypatch):
    from dilqr import generic
    from dilqr.definitions import QuadCost
    from dilqr.dynamics import NNDynamics
    from dilqr.mpc_explicit import GradMethods
    quad = QuadCost(torch.zeros(4, 3, 6, 6), torch.zeros(4, 3, 6))
    one, two = NNDynamics(5, 1, hidden_sizes=[32]), NNDynamics(5, 1, hidden_sizes=[16, 8])
    slew, trust = dict(slew_rate_penalty=0.1), dict(delta_u=0.25)
    assert generic.DEVICE_MLP_SLEW is False and generic.DEVICE_MLP_DELTA_U is False
    # off: today's routing
    for dx in (one, two):
        assert routed(dx, quad, **slew) == "torch" and routed(dx, quad, **trust) == "torch"
    assert routed(one, quad) == "device" and routed(two, quad) == "torch"
    # each switch sends exactly its own case to the device
    monkeypatch.setattr(generic, "DEVICE_MLP_SLEW", True)
    assert routed(one, quad, **slew) == "device:slew"
    assert routed(one, quad, prev_ctrl=torch.zeros(3, 1), **slew) == "device:slew"
    assert routed(one, quad, u_lower=None, u_upper=None, **slew) == "device:slew"
    assert routed(one, quad, **trust) == "torch"
    assert routed(one, quad) == "device"
    assert routed(two, quad, **slew) == "torch"                     # two hidden layers: DEVICE_MLP_DEEP as well
    monkeypatch.setattr(generic, "DEVICE_MLP_SLEW", False)
    monkeypatch.setattr(generic, "DEVICE_MLP_DELTA_U", True)
    assert routed(one, quad, **trust) == "device:delta_u=0.25"
    assert routed(one, quad, **slew) == "torch"
    assert routed(one, quad) == "device"
    assert routed(two, quad, **trust) == "torch"
    # both on
    monkeypatch.setattr(generic, "DEVICE_MLP_SLEW", True)
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    for dx in (one, two, NNDynamics(5, 1, hidden_sizes=[100], activation="relu", passthrough=False)):
        assert routed(dx, quad, **slew) == "device:slew"
        assert routed(dx, quad, **trust) == "device:delta_u=0.25"
        assert routed(dx, quad, verbose=-1, **slew) == "device:slew"
        # the two options together, and every option outside the envelope, keep the torch loop
        assert routed(dx, quad, **slew, **trust) == "torch"
        for opt in (slew, trust):
            assert routed(dx, quad, verbose=1, **opt) == "torch"
            assert routed(dx, quad, grad_method=GradMethods.AUTO_DIFF, **opt) == "torch"
            assert routed(dx, quad, grad_method=GradMethods.FINITE_DIFF, **opt) == "torch"
            assert routed(dx, lambda tau: (tau ** 2).sum(-1), **opt) == "torch"
    for opt in (slew, trust):
        assert routed(NNDynamics(5, 1, hidden_sizes=[32], activation="elu"), quad, **opt) == "torch"
        assert routed(NNDynamics(5, 1, hidden_sizes=[8, 8, 8]), quad, **opt) == "torch"
        assert routed(NNDynamics(5, 1, hidden_sizes=[32]).double(), quad, **opt) == "torch"
    # a (4,3) network: (7,3) is not a compiled shape, so the slew-rate solve stays in torch; delta_u does not
    quad43 = QuadCost(torch.zeros(4, 3, 7, 7), torch.zeros(4, 3, 7))
    dx43 = NNDynamics(4, 3, hidden_sizes=[8])
    assert routed(dx43, quad43, n=4, m=3, **slew) == "torch"
    assert routed(dx43, quad43, n=4, m=3, **trust) == "device:delta_u=0.25"
    assert routed(dx43, quad43, n=4, m=3) == "device"
    # a (4,2) network under slew is served: (6,2)
    quad42 = QuadCost(torch.zeros(4, 3, 6, 6), torch.zeros(4, 3, 6))
    assert routed(NNDynamics(4, 2, hidden_sizes=[8]), quad42, n=4, m=2, **slew) == "device:slew"
    # and DEVICE_MLP off switches all of it off
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    assert routed(one, quad, **slew) == "torch" and routed(one, quad, **trust) == "torch"


# ------------------------------------------------------------------ routing of one LQR step
T_, B_, N_, M_ = 4, 3, 5, 1


@pytest.fixture
def step_routed(monkeypatch):
    """tests/test_mlp_cpu.py's step_routed: one regular LQR step forward through
    each of its three drivers with the sweep, the device line search and the
    torch line search's first step replaced by stubs."""
    from dilqr import generic, lqr_step, lqr_step_explicit, ops

    def fake(*shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).as_subclass(FakeCuda)

    def sweep(C, c, F, n, m, **kw):
        T, B = C.shape[:2]
        return torch.zeros(T, B, m, n), torch.zeros(T, B, m), 0

    seen = {}

    def device(model_id, theta, x_init, C, c, x, u, K, k, F=None, f=None, u_lower=None, u_upper=None, **kw):
        seen["bounds"] = (u_lower, u_upper)
        raise _Taken("device")

    def torch_loop(*a, **k):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "lqr_backward", sweep)
    monkeypatch.setattr(ops, "lqr_forward", device)
    monkeypatch.setattr(generic, "traj_cost", torch_loop)

    def route(driver, dx, cost, delta_u=None, lo=-1.0, hi=1.0):
        d = N_ + M_
        x_init, x, u = fake(B_, N_), fake(T_, B_, N_), fake(T_, B_, M_)
        C, c, F = fake(T_, B_, d, d), fake(T_, B_, d), fake(T_ - 1, B_, N_, d)
        seen.clear()
        with pytest.raises(_Taken) as e:
            if driver == "generic":
                generic.lqr_step_forward(T_, N_, M_, x_init, C, c, F, x, u, cost, dx, lo, hi, delta_u, 0.2, 10)
            else:
                mod = {"classic": lqr_step, "explicit": lqr_step_explicit}[driver]
                step = mod.LQRStep(N_, M_, T_, u_lower=lo, u_upper=hi, delta_u=delta_u, true_cost=cost,
                                   true_dynamics=dx, current_x=x, current_u=u)
                step(x_init, C, c, F)
        return str(e.value), seen.get("bounds"), u

    route.fake = fake
    return route


@pytest.mark.parametrize("driver", ["classic", "explicit", "generic"])
def test_lqr_step_routing_with_delta_u(step_routed, driver, monkeypatch):
    """With DEVICE_MLP_DELTA_U one LQR step with delta_u on a network takes the
    device line search, clamped to ops.delta_u_rollout_bounds, through all three
    drivers; off, it keeps the torch line search."""
    from dilqr import generic, ops
    from dilqr.definitions import QuadCost
    from dilqr.dynamics import NNDynamics
    d = N_ + M_
    fake = step_routed.fake
    quad = QuadCost(fake(T_, B_, d, d), fake(T_, B_, d))
    nn, nn2 = NNDynamics(N_, M_, hidden_sizes=[8]), NNDynamics(N_, M_, hidden_sizes=[8, 8])
    assert step_routed(driver, nn, quad, delta_u=0.25)[0] == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP_DELTA_U", True)
    took, bounds, u = step_routed(driver, nn, quad, delta_u=0.25)
    assert took == "device"
    lo, hi = ops.delta_u_rollout_bounds(-1.0, 1.0, u, 0.25)
    assert torch.equal(bounds[0], lo) and torch.equal(bounds[1], hi)
    # without delta_u nothing changed
    assert step_routed(driver, nn, quad)[:2] == ("device", (-1.0, 1.0))
    # the other rules stand: two layers need DEVICE_MLP_DEEP, a callable cost and a partial QuadCost stay in torch
    assert step_routed(driver, nn2, quad, delta_u=0.25)[0] == "torch"
    assert step_routed(driver, nn, lambda tau: (tau ** 2).sum(-1), delta_u=0.25)[0] == "torch"
    assert step_routed(driver, nn, QuadCost(fake(d, d), fake(d)), delta_u=0.25)[0] == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    assert step_routed(driver, nn2, quad, delta_u=0.25)[0] == "device"
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    assert step_routed(driver, nn, quad, delta_u=0.25)[0] == "torch"


# ------------------------------------------------------------------ delta_u without bounds
def test_mpc_solve_unfused_delta_u_needs_bounds():
    """The reference's refusal (lqr_step_explicit.py:197), before anything is allocated or launched."""
    from dilqr import _native as N
    from dilqr import ops
    T, B, n, m = 4, 3, 5, 1
    x0, C, c = torch.zeros(B, n), torch.zeros(T, B, n + m, n + m), torch.zeros(T, B, n + m)
    with pytest.raises(NotImplementedError, match="delta_u without u_lower"):
        ops.mpc_solve_unfused(N.MODEL_CARTPOLE, torch.zeros(4), x0, C, c, T, delta_u=1.0)
