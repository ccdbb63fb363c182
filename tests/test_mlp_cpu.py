"""CPU checks of the device MLP dynamics (csrc/tu_mlp.hip) around the kernels:
what NNDynamics.device_model hands the C-ABI, the dilqr_mlp_* entry points'
argument validation (errors return before any launch, so no GPU is needed) and
the routing rules of dilqr.generic.solve."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")


def header_int(name):
    return int(re.search(rf"#define {name}\s+(\d+)", open(HEADER).read()).group(1))


def test_binding_constants_match_header():
    from dilqr import _native as N
    assert N.MODEL_MLP == header_int("DILQR_MODEL_MLP")
    assert N.MLP_SIGMOID == header_int("DILQR_MLP_SIGMOID") and N.MLP_RELU == header_int("DILQR_MLP_RELU")
    assert N.MLP_MAX_HIDDEN == header_int("DILQR_MLP_MAX_HIDDEN")
    assert N.MLP_MAX_HIDDEN >= 256
    # the binding's struct has the header's fields, in order
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct dilqr_mlp \{(.*?)\} dilqr_mlp;", src, re.S).group(1)
    assert [f for f, _ in N.Mlp._fields_] == re.findall(r"(\w+)\s*;", body)
    # the shape list is the one the kernels are compiled for
    common = open(os.path.join(ROOT, "differentiable-ilqr_amd", "csrc", "dilqr_common.h")).read()
    line = re.search(r"#define DILQR_FOR_EACH_SHAPE\(X\)(.*)", common).group(1)
    assert tuple((int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", line)) == N.LANE_SHAPES


def test_device_model_contents():
    from dilqr import _native as N
    from dilqr.dynamics import NNDynamics
    like = torch.zeros(1)
    dx = NNDynamics(5, 1, hidden_sizes=[32], activation="sigmoid")
    md = dx.device_model(like)
    assert (md.n, md.m, md.H) == (5, 1, 32)
    assert (md.desc.n_hidden, md.desc.activation, md.desc.passthrough) == (32, N.MLP_SIGMOID, 1)
    # the module's own parameter storage, not a copy
    assert md.desc.W1 == dx.fcs[0].weight.data_ptr() and md.desc.b1 == dx.fcs[0].bias.data_ptr()
    assert md.desc.W2 == dx.fcs[1].weight.data_ptr() and md.desc.b2 == dx.fcs[1].bias.data_ptr()
    md = NNDynamics(4, 2, hidden_sizes=[N.MLP_MAX_HIDDEN], activation="relu", passthrough=False).device_model(like)
    assert (md.n, md.m, md.desc.n_hidden, md.desc.activation, md.desc.passthrough) == (
        4, 2, N.MLP_MAX_HIDDEN, N.MLP_RELU, 0)


def test_device_model_outside_envelope_is_none():
    from dilqr import _native as N
    from dilqr.dynamics import NNDynamics
    like = torch.zeros(1)
    assert NNDynamics(5, 1, hidden_sizes=[16, 8]).device_model(like) is None
    assert NNDynamics(5, 1, hidden_sizes=[32], activation="elu").device_model(like) is None
    assert NNDynamics(5, 1, hidden_sizes=[N.MLP_MAX_HIDDEN + 1]).device_model(like) is None
    assert NNDynamics(7, 3, hidden_sizes=[32]).device_model(like) is None
    assert NNDynamics(5, 1, hidden_sizes=[32]).double().device_model(like) is None
    # parameters on another device than the inputs
    assert NNDynamics(5, 1, hidden_sizes=[32]).device_model(torch.zeros(1, device="meta")) is None
    # non-contiguous parameters
    dx = NNDynamics(5, 1, hidden_sizes=[32])
    dx.fcs[0].weight = torch.nn.Parameter(torch.zeros(6, 32).t())
    assert dx.device_model(like) is None


def _calls(N, n=5, m=1, H=32, act=0, W1=16, b1=16, W2=16, b2=16, x=16):
    """Every dilqr_mlp_* entry point with fake (never dereferenced) pointers."""
    lib = N.lib()
    P = ctypes.c_void_p
    d = N.Mlp(H, act, 1, W1, b1, W2, b2)
    nb = N.Bounds(N.BOUNDS_NONE, 0.0, 0.0, None, None)
    p = P(16)
    return {
        "dynamics": lib.dilqr_mlp_dynamics_f32(n, m, 65, d, P(x), p, p, None),
        "linear_dyn": lib.dilqr_mlp_linear_dyn_f32(n, m, 65, d, P(x), p, p, None),
        "rollout": lib.dilqr_mlp_rollout_f32(n, m, 4, 65, d, P(x), p, p, None),
        "linearize": lib.dilqr_mlp_linearize_f32(n, m, 4, 65, d, P(x), p, p, p, None),
        "lqr_forward": lib.dilqr_mlp_lqr_forward_f32(n, m, 4, 65, d, P(x), p, p, p, p, p, p, nb, None, 0.2, 10, p, p,
                                                     p, p, p, None, None),
    }


def test_mlp_entry_points_reject_bad_arguments_without_launch():
    """Null / misaligned pointers -> 2, unsupported (n, m) or H -> 1, unknown
    activation -> 3, each before any kernel launch (this runs without a GPU)."""
    from dilqr import _native as N
    E_SHAPE, E_ARG, E_MODE = 1, 2, 3
    for kw in ({"W1": None}, {"b1": None}, {"W2": None}, {"b2": None}, {"W1": 4}, {"b1": 8}, {"W2": 20},
               {"b2": 12}, {"x": None}, {"x": 4}):
        assert set(_calls(N, **kw).values()) == {E_ARG}, kw
    for kw in ({"n": 7, "m": 3}, {"n": 13, "m": 3}, {"H": 0}, {"H": N.MLP_MAX_HIDDEN + 1}):
        assert set(_calls(N, **kw).values()) == {E_SHAPE}, kw
    for kw in ({"act": 2}, {"act": -1}):
        assert set(_calls(N, **kw).values()) == {E_MODE}, kw
    lib = N.lib()
    p = ctypes.c_void_p(16)
    nb = N.Bounds(N.BOUNDS_NONE, 0.0, 0.0, None, None)
    d = N.Mlp(32, 0, 1, 16, 16, 16, 16)
    # sizes and options of the line search, as dilqr_lqr_forward_f32 checks them
    assert lib.dilqr_mlp_lqr_forward_f32(5, 1, 4, 65, d, p, p, p, p, p, p, p, nb, None, 0.2, 0, p, p, p, p, p, None,
                                         None) == E_ARG
    assert lib.dilqr_mlp_lqr_forward_f32(5, 1, 4, 65, d, p, p, p, p, p, p, p,
                                         N.Bounds(N.BOUNDS_TENSOR, 0.0, 0.0, None, None), None, 0.2, 10, p, p, p, p,
                                         p, None, None) == E_ARG
    assert lib.dilqr_mlp_rollout_f32(5, 1, 0, 65, d, p, p, p, None) == E_ARG
    # an empty batch is valid and launches nothing
    assert lib.dilqr_mlp_dynamics_f32(5, 1, 0, d, p, p, p, None) == 0
    assert lib.dilqr_mlp_linearize_f32(5, 1, 1, 65, d, p, p, p, p, None) == 0


def test_ops_refuse_mismatched_shapes_before_launch():
    """Rows whose widths are not the model's (n, m) would be indexed out of
    bounds on the device: refused on the host."""
    from dilqr import ops
    from dilqr.dynamics import NNDynamics
    md = NNDynamics(5, 1, hidden_sizes=[8]).device_model(torch.zeros(1))
    with pytest.raises(ValueError, match="MLP model"):
        ops.mlp_dynamics(md, torch.zeros(3, 4), torch.zeros(3, 1))
    with pytest.raises(ValueError, match="MLP model"):
        ops.mlp_linearize(md, torch.zeros(4, 3, 5), torch.zeros(4, 3, 2))
    with pytest.raises(ValueError, match="MLP model"):
        ops.mlp_rollout(md, torch.zeros(3, 5), torch.zeros(4, 2, 1))
    with pytest.raises(TypeError):
        ops.mlp_dynamics(md, torch.zeros(3, 5, dtype=torch.float64), torch.zeros(3, 1))


class _Taken(Exception):
    pass


@pytest.fixture
def routed(monkeypatch):
    """generic.solve with ops.mpc_solve_unfused replaced by a stub that records
    the call and ends it, and the torch loop's first step (the rollout)
    replaced by another: route(...) tells which one the solve reached.  The
    routing only looks at the inputs' device and dtype, so `meta` tensors stand
    in for GPU ones (is_cuda is read through the fake below)."""
    from dilqr import generic, ops

    def stub(model_id, theta, *a, **k):
        assert isinstance(model_id, ops.MlpModel) and theta is None
        raise _Taken("device")

    def torch_loop(*a, **k):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "mpc_solve_unfused", stub)
    monkeypatch.setattr(generic, "rollout", torch_loop)

    class FakeCuda(torch.Tensor):
        is_cuda = True

    def route(dx, cost, **mpc_kw):
        from dilqr.mpc_explicit import GradMethods
        kw = dict(T=4, n_state=5, n_ctrl=1, u_init=None, u_lower=-1.0, u_upper=1.0, lqr_iter=3, eps=1e-7,
                  grad_method=GradMethods.ANALYTIC, slew_rate_penalty=None, delta_u=None, verbose=0,
                  linesearch_decay=0.2, max_linesearch_iter=10, not_improved_lim=5, best_cost_eps=1e-4)
        kw.update(mpc_kw)
        x0 = torch.zeros(3, 5).as_subclass(FakeCuda)
        with pytest.raises(_Taken) as e:
            generic.solve(types.SimpleNamespace(**kw), x0, cost, dx, 3)
        return str(e.value)

    return route


def test_solve_routing(routed, monkeypatch):
    from dilqr import generic
    from dilqr.definitions import QuadCost
    from dilqr.dynamics import NNDynamics
    from dilqr.mpc_explicit import GradMethods
    quad = QuadCost(torch.zeros(4, 3, 6, 6), torch.zeros(4, 3, 6))
    dx = NNDynamics(5, 1, hidden_sizes=[32])
    assert generic.DEVICE_MLP is True
    assert routed(dx, quad) == "device"
    assert routed(NNDynamics(5, 1, hidden_sizes=[100], activation="relu", passthrough=False), quad) == "device"
    assert routed(dx, quad, verbose=-1) == "device"
    # every excluded option keeps the torch loop
    assert routed(dx, quad, grad_method=GradMethods.AUTO_DIFF) == "torch"
    assert routed(dx, quad, grad_method=GradMethods.FINITE_DIFF) == "torch"
    assert routed(dx, quad, slew_rate_penalty=0.1) == "torch"
    assert routed(dx, quad, delta_u=0.5) == "torch"
    assert routed(dx, quad, verbose=1) == "torch"
    assert routed(dx, lambda tau: (tau ** 2).sum(-1)) == "torch"
    assert routed(NNDynamics(5, 1, hidden_sizes=[16, 8]), quad) == "torch"
    assert routed(NNDynamics(5, 1, hidden_sizes=[32], activation="elu"), quad) == "torch"
    assert routed(NNDynamics(5, 1, hidden_sizes=[32]).double(), quad) == "torch"
    # and so does the switch
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    assert routed(dx, quad) == "torch"


T_, B_, N_, M_ = 4, 3, 5, 1


@pytest.fixture
def step_routed(monkeypatch):
    """One regular (non no-op) LQR step forward through each of its three
    drivers, with the sweep (ops.lqr_backward) replaced by zero gains, the
    device line search (ops.lqr_forward) by a stub that records the bounds it
    was handed and ends the call, and the torch line search's first step
    (generic.traj_cost) by another: route(...) tells which one the step
    reached, and with which (u_lower, u_upper).  Every tensor is a FakeCuda."""
    from dilqr import generic, lqr_step, lqr_step_explicit, ops

    class FakeCuda(torch.Tensor):
        is_cuda = True

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
def test_lqr_step_routing(step_routed, driver, monkeypatch):
    """Which line search one LQR step takes, and with which rollout bounds.

    Through both LQRStep factories an env_dx model or a LinDx with a QuadCost
    takes the device line search, with or without delta_u.  generic.
    lqr_step_forward called directly (the generic MPC loop's use of it) has
    always run those dynamics in torch and sends only a device MLP to the
    kernels; that difference between the drivers is part of today's routing
    and is pinned here too.  A one-hidden-layer NNDynamics with a full QuadCost
    and no delta_u takes the device line search through all three."""
    from dilqr import generic, ops
    from dilqr.definitions import LinDx, QuadCost
    from dilqr.dynamics import NNDynamics
    from dilqr.env_dx.cartpole import CartpoleDx
    d = N_ + M_
    fake = step_routed.fake
    quad = QuadCost(fake(T_, B_, d, d), fake(T_, B_, d))
    lin = LinDx(fake(T_ - 1, B_, N_, d), fake(T_ - 1, B_, N_))
    nn = NNDynamics(N_, M_, hidden_sizes=[8])

    def callable_cost(tau):
        return (tau ** 2).sum(-1)

    env_route = "device" if driver != "generic" else "torch"
    for dx, delta_u, want in ((CartpoleDx(), None, env_route), (CartpoleDx(), 0.25, env_route),
                              (lin, None, env_route), (lin, 0.25, env_route), (nn, None, "device")):
        took, bounds, u = step_routed(driver, dx, quad, delta_u=delta_u)
        assert took == want, (type(dx).__name__, delta_u)
        if took == "device" and delta_u is None:
            assert bounds == (-1.0, 1.0)
        elif took == "device":
            lo, hi = ops.delta_u_rollout_bounds(-1.0, 1.0, u, delta_u)
            assert torch.equal(bounds[0], lo) and torch.equal(bounds[1], hi)
    # unbounded: no bounds reach the line search
    took, bounds, _ = step_routed(driver, CartpoleDx(), quad, lo=None, hi=None)
    assert (took, bounds) == (env_route, (None, None) if env_route == "device" else None)
    took, bounds, _ = step_routed(driver, nn, quad, lo=None, hi=None)
    assert (took, bounds) == ("device", (None, None))
    # everything else keeps the torch line search
    assert step_routed(driver, nn, quad, delta_u=0.25)[0] == "torch"
    assert step_routed(driver, nn, callable_cost)[0] == "torch"
    assert step_routed(driver, NNDynamics(N_, M_, hidden_sizes=[8, 8]), quad)[0] == "torch"
    assert step_routed(driver, CartpoleDx(), callable_cost)[0] == "torch"
    # a QuadCost that is not the full [T,B,d,d] / [T,B,d] keeps the MLP in torch
    assert step_routed(driver, nn, QuadCost(fake(d, d), fake(d)))[0] == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    assert step_routed(driver, nn, quad)[0] == "torch"
