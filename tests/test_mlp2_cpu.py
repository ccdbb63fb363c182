"""CPU checks of the two-hidden-layer device MLP dynamics (csrc/tu_mlp2.hip)
around the kernels: the binding against the header, what NNDynamics.
device_model(like, deep=True) hands the C-ABI, the dilqr_mlp2_* entry points'
argument validation (errors return before any launch, so no GPU is needed) and
the routing rules of dilqr.generic under DEVICE_MLP_DEEP, which ships off."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")
NAMES = ["dilqr_mlp2_dynamics_f32", "dilqr_mlp2_linear_dyn_f32", "dilqr_mlp2_rollout_f32", "dilqr_mlp2_linearize_f32",
         "dilqr_mlp2_lqr_forward_f32"]


def header_src():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_binding_matches_header():
    from dilqr import _native as N
    src = header_src()
    body = re.search(r"typedef struct dilqr_mlp2 \{(.*?)\} dilqr_mlp2;", src, re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == ["n_hidden1", "n_hidden2", "activation", "passthrough", "W1", "b1", "W2", "b2", "W3", "b3"]
    assert [f for f, _ in N.Mlp2._fields_] == fields
    lib = N.lib()
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
        assert hasattr(lib, name), name
        assert name in N.SIGNATURES, name
        # the argument list of the one-layer counterpart, with the descriptor exchanged
        args, res = N.SIGNATURES[name]
        args1, res1 = N.SIGNATURES[name.replace("mlp2", "mlp")]
        assert res is res1 and [N.Mlp if a is N.Mlp2 else a for a in args] == args1 and N.Mlp2 in args
    # additive symbols: the version is the one the binding expects
    assert lib.dilqr_version() == N.ABI_VERSION
    # the one-layer descriptor is as it was
    body1 = re.search(r"typedef struct dilqr_mlp \{(.*?)\} dilqr_mlp;", src, re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body1) == ["n_hidden", "activation", "passthrough", "W1", "b1", "W2", "b2"]


def _calls(N, n=5, m=1, H1=32, H2=16, act=0, W1=16, b1=16, W2=16, b2=16, W3=16, b3=16, x=16):
    """Every dilqr_mlp2_* entry point with fake (never dereferenced) pointers."""
    lib = N.lib()
    P = ctypes.c_void_p
    d = N.Mlp2(H1, H2, act, 1, W1, b1, W2, b2, W3, b3)
    nb = N.Bounds(N.BOUNDS_NONE, 0.0, 0.0, None, None)
    p = P(16)
    return {
        "dynamics": lib.dilqr_mlp2_dynamics_f32(n, m, 65, d, P(x), p, p, None),
        "linear_dyn": lib.dilqr_mlp2_linear_dyn_f32(n, m, 65, d, P(x), p, p, None),
        "rollout": lib.dilqr_mlp2_rollout_f32(n, m, 4, 65, d, P(x), p, p, None),
        "linearize": lib.dilqr_mlp2_linearize_f32(n, m, 4, 65, d, P(x), p, p, p, None),
        "lqr_forward": lib.dilqr_mlp2_lqr_forward_f32(n, m, 4, 65, d, P(x), p, p, p, p, p, p, nb, None, 0.2, 10, p, p,
                                                      p, p, p, None, None),
    }


def test_mlp2_entry_points_reject_bad_arguments_without_launch():
    """Null / misaligned pointers -> 2, unsupported (n, m) or width -> 1, unknown
    activation -> 3, each before any kernel launch (this runs without a GPU)."""
    from dilqr import _native as N
    E_SHAPE, E_ARG, E_MODE = 1, 2, 3
    for w in ("W1", "b1", "W2", "b2", "W3", "b3"):
        for bad in (None, 4, 8, 20):
            assert set(_calls(N, **{w: bad}).values()) == {E_ARG}, (w, bad)
    for kw in ({"x": None}, {"x": 4}):
        assert set(_calls(N, **kw).values()) == {E_ARG}, kw
    for kw in ({"n": 7, "m": 3}, {"n": 13, "m": 3}, {"H1": 0}, {"H1": N.MLP_MAX_HIDDEN + 1}, {"H2": 0},
               {"H2": N.MLP_MAX_HIDDEN + 1}):
        assert set(_calls(N, **kw).values()) == {E_SHAPE}, kw
    for kw in ({"act": 2}, {"act": -1}):
        assert set(_calls(N, **kw).values()) == {E_MODE}, kw
    # both widths at the limit are inside the envelope: only the pointers' alignment is left to refuse
    assert set(_calls(N, H1=N.MLP_MAX_HIDDEN, H2=N.MLP_MAX_HIDDEN, x=4).values()) == {E_ARG}
    lib = N.lib()
    p = ctypes.c_void_p(16)
    nb = N.Bounds(N.BOUNDS_NONE, 0.0, 0.0, None, None)
    d = N.Mlp2(32, 16, 0, 1, 16, 16, 16, 16, 16, 16)
    # sizes and options of the line search, as dilqr_lqr_forward_f32 checks them
    assert lib.dilqr_mlp2_lqr_forward_f32(5, 1, 4, 65, d, p, p, p, p, p, p, p, nb, None, 0.2, 0, p, p, p, p, p, None,
                                          None) == E_ARG
    assert lib.dilqr_mlp2_lqr_forward_f32(5, 1, 4, 65, d, p, p, p, p, p, p, p,
                                          N.Bounds(N.BOUNDS_TENSOR, 0.0, 0.0, None, None), None, 0.2, 10, p, p, p, p,
                                          p, None, None) == E_ARG
    assert lib.dilqr_mlp2_rollout_f32(5, 1, 0, 65, d, p, p, p, None) == E_ARG
    # an empty batch, or T = 1 for the linearisation, is valid and launches nothing
    assert lib.dilqr_mlp2_dynamics_f32(5, 1, 0, d, p, p, p, None) == 0
    assert lib.dilqr_mlp2_linear_dyn_f32(5, 1, 0, d, p, p, p, None) == 0
    assert lib.dilqr_mlp2_rollout_f32(5, 1, 4, 0, d, p, p, p, None) == 0
    assert lib.dilqr_mlp2_linearize_f32(5, 1, 1, 65, d, p, p, p, p, None) == 0
    assert lib.dilqr_mlp2_linearize_f32(5, 1, 4, 0, d, p, p, p, p, None) == 0
    assert lib.dilqr_mlp2_lqr_forward_f32(5, 1, 4, 0, d, p, p, p, p, p, p, p, nb, None, 0.2, 10, p, p, p, p, p, None,
                                          None) == 0


def test_device_model_deep_contents():
    from dilqr import _native as N
    from dilqr import ops
    from dilqr.dynamics import NNDynamics
    like = torch.zeros(1)
    dx = NNDynamics(5, 1, hidden_sizes=[32, 16], activation="sigmoid")
    md = dx.device_model(like, deep=True)
    assert isinstance(md, ops.Mlp2Model) and not isinstance(md, ops.MlpModel)
    assert (md.n, md.m, md.H1, md.H2, md.device) == (5, 1, 32, 16, like.device)
    assert (md.desc.n_hidden1, md.desc.n_hidden2, md.desc.activation, md.desc.passthrough) == (32, 16, N.MLP_SIGMOID, 1)
    # the module's own parameter storage, not a copy
    for i, fc in enumerate(dx.fcs):
        assert getattr(md.desc, f"W{i + 1}") == fc.weight.data_ptr() and getattr(md.desc, f"b{i + 1}") == fc.bias.data_ptr()
        assert md.tensors[2 * i].data_ptr() == fc.weight.data_ptr() and md.tensors[2 * i + 1].data_ptr() == fc.bias.data_ptr()
    md = NNDynamics(4, 2, hidden_sizes=[N.MLP_MAX_HIDDEN, 1], activation="relu", passthrough=False).device_model(
        like, deep=True)
    assert (md.n, md.m, md.desc.n_hidden1, md.desc.n_hidden2, md.desc.activation, md.desc.passthrough) == (
        4, 2, N.MLP_MAX_HIDDEN, 1, N.MLP_RELU, 0)
    # deep=True leaves a one-hidden-layer module with its one-layer model
    one = NNDynamics(5, 1, hidden_sizes=[32]).device_model(like, deep=True)
    assert isinstance(one, ops.MlpModel) and one.H == 32
    # and the model refuses rows of other widths, like the one-layer model
    md = dx.device_model(like, deep=True)
    with pytest.raises(ValueError, match="MLP model"):
        ops.mlp_dynamics(md, torch.zeros(3, 4), torch.zeros(3, 1))
    with pytest.raises(ValueError, match="MLP model"):
        ops.mlp_rollout(md, torch.zeros(3, 5), torch.zeros(4, 2, 1))
    with pytest.raises(TypeError):
        ops.mlp_linearize_vjp(md, torch.zeros(4, 3, 5), torch.zeros(4, 3, 1), None, None)


def test_device_model_deep_outside_envelope_is_none():
    from dilqr import _native as N
    from dilqr.dynamics import NNDynamics
    like = torch.zeros(1)
    assert NNDynamics(5, 1, hidden_sizes=[16, 8, 8]).device_model(like, deep=True) is None
    assert NNDynamics(5, 1, hidden_sizes=[16, 8], activation="elu").device_model(like, deep=True) is None
    assert NNDynamics(5, 1, hidden_sizes=[N.MLP_MAX_HIDDEN + 1, 8]).device_model(like, deep=True) is None
    assert NNDynamics(5, 1, hidden_sizes=[8, N.MLP_MAX_HIDDEN + 1]).device_model(like, deep=True) is None
    assert NNDynamics(7, 3, hidden_sizes=[16, 8]).device_model(like, deep=True) is None
    assert NNDynamics(5, 1, hidden_sizes=[16, 8]).double().device_model(like, deep=True) is None
    assert NNDynamics(5, 1, hidden_sizes=[16, 8]).device_model(torch.zeros(1, device="meta"), deep=True) is None
    dx = NNDynamics(5, 1, hidden_sizes=[16, 8])
    dx.fcs[1].weight = torch.nn.Parameter(torch.zeros(16, 8).t())
    assert dx.device_model(like, deep=True) is None
    # without deep, two layers have no device model, as before
    assert NNDynamics(5, 1, hidden_sizes=[16, 8]).device_model(like) is None
    assert NNDynamics(5, 1, hidden_sizes=[16, 8]).device_model(like, deep=False) is None


class _Taken(Exception):
    pass


class FakeCuda(torch.Tensor):
    is_cuda = True


def test_solve_routing(monkeypatch):
    """generic.solve with ops.mpc_solve_unfused replaced by a stub that records
    the model it was handed and ends the call, and the torch loop's first step
    (the rollout) by another.  `is_cuda` is faked: the routing reads nothing
    else of the device."""
    from dilqr import generic, ops
    from dilqr.definitions import QuadCost
    from dilqr.dynamics import NNDynamics
    from dilqr.mpc_explicit import GradMethods
    seen = {}

    def stub(model_id, theta, *a, **k):
        seen["model"] = model_id
        assert theta is None
        raise _Taken("device")

    def torch_loop(*a, **k):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "mpc_solve_unfused", stub)
    monkeypatch.setattr(generic, "rollout", torch_loop)

    def routed(dx, cost, **mpc_kw):
        kw = dict(T=4, n_state=5, n_ctrl=1, u_init=None, u_lower=-1.0, u_upper=1.0, lqr_iter=3, eps=1e-7,
                  grad_method=GradMethods.ANALYTIC, slew_rate_penalty=None, delta_u=None, verbose=0,
                  linesearch_decay=0.2, max_linesearch_iter=10, not_improved_lim=5, best_cost_eps=1e-4)
        kw.update(mpc_kw)
        x0 = torch.zeros(3, 5).as_subclass(FakeCuda)
        seen.clear()
        with pytest.raises(_Taken) as e:
            generic.solve(types.SimpleNamespace(**kw), x0, cost, dx, 3)
        return str(e.value)

    quad = QuadCost(torch.zeros(4, 3, 6, 6), torch.zeros(4, 3, 6))
    dx = NNDynamics(5, 1, hidden_sizes=[16, 8])
    # the switch ships off: torch
    assert generic.DEVICE_MLP_DEEP is False
    assert routed(dx, quad) == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    assert routed(dx, quad) == "device" and isinstance(seen["model"], ops.Mlp2Model)
    assert routed(NNDynamics(5, 1, hidden_sizes=[64, 64], activation="relu", passthrough=False), quad) == "device"
    assert routed(dx, quad, verbose=-1) == "device"
    # a one-layer module keeps its own model
    assert routed(NNDynamics(5, 1, hidden_sizes=[32]), quad) == "device" and isinstance(seen["model"], ops.MlpModel)
    # every excluded option keeps the torch loop
    assert routed(dx, quad, grad_method=GradMethods.AUTO_DIFF) == "torch"
    assert routed(dx, quad, grad_method=GradMethods.FINITE_DIFF) == "torch"
    assert routed(dx, quad, slew_rate_penalty=0.1) == "torch"
    assert routed(dx, quad, delta_u=0.5) == "torch"
    assert routed(dx, quad, verbose=1) == "torch"
    assert routed(dx, lambda tau: (tau ** 2).sum(-1)) == "torch"
    assert routed(NNDynamics(5, 1, hidden_sizes=[16, 8, 8]), quad) == "torch"
    assert routed(NNDynamics(5, 1, hidden_sizes=[16, 8], activation="elu"), quad) == "torch"
    assert routed(NNDynamics(5, 1, hidden_sizes=[16, 8]).double(), quad) == "torch"
    # DEVICE_MLP off switches every network off, deep or not
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    assert routed(dx, quad) == "torch"


T_, B_, N_, M_ = 4, 3, 5, 1


@pytest.mark.parametrize("driver", ["classic", "explicit", "generic"])
def test_lqr_step_routing(driver, monkeypatch):
    """Which line search one regular LQR step takes for a two-hidden-layer
    module, through each of the step's three drivers: the sweep is replaced by
    zero gains, the device line search (ops.lqr_forward) and the torch line
    search's first step (generic.traj_cost) by stubs that end the call."""
    from dilqr import generic, lqr_step, lqr_step_explicit, ops
    from dilqr.definitions import QuadCost
    from dilqr.dynamics import NNDynamics

    def fake(*shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).as_subclass(FakeCuda)

    def sweep(C, c, F, n, m, **kw):
        T, B = C.shape[:2]
        return torch.zeros(T, B, m, n), torch.zeros(T, B, m), 0

    seen = {}

    def device(model_id, theta, x_init, C, c, x, u, K, k, F=None, f=None, u_lower=None, u_upper=None, **kw):
        seen["model"], seen["bounds"] = model_id, (u_lower, u_upper)
        raise _Taken("device")

    def torch_loop(*a, **k):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "lqr_backward", sweep)
    monkeypatch.setattr(ops, "lqr_forward", device)
    monkeypatch.setattr(generic, "traj_cost", torch_loop)
    d = N_ + M_

    def route(dx, cost, delta_u=None, lo=-1.0, hi=1.0):
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
        return str(e.value)

    quad = QuadCost(fake(T_, B_, d, d), fake(T_, B_, d))
    nn = NNDynamics(N_, M_, hidden_sizes=[8, 8])
    assert generic.DEVICE_MLP_DEEP is False
    assert route(nn, quad) == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    assert route(nn, quad) == "device"
    model = seen["model"].mlp if isinstance(seen["model"], ops.Dynamics) else seen["model"]
    assert isinstance(model, ops.Mlp2Model) and seen["bounds"] == (-1.0, 1.0)
    assert route(nn, quad, lo=None, hi=None) == "device" and seen["bounds"] == (None, None)
    # everything else keeps the torch line search
    assert route(nn, quad, delta_u=0.25) == "torch"
    assert route(nn, lambda tau: (tau ** 2).sum(-1)) == "torch"
    assert route(nn, QuadCost(fake(d, d), fake(d))) == "torch"
    assert route(NNDynamics(N_, M_, hidden_sizes=[8, 8, 8]), quad) == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    assert route(nn, quad) == "torch"


def test_linearize_routing(monkeypatch):
    """generic.linearize: without gradient a two-layer module reaches the
    kernel only with the switch on; with gradient it reaches the torch graph
    whatever the switch says, and a one-layer module still reaches
    ops.mlp_linearize_diff."""
    from dilqr import generic, ops
    from dilqr.dynamics import NNDynamics
    from dilqr.mpc_explicit import GradMethods

    def diff_kernel(mlp, params, x, u):
        assert isinstance(mlp, ops.MlpModel) and len(params) == 4
        raise _Taken("device diff")

    def kernel(mlp, x, u):
        raise _Taken("device " + type(mlp).__name__)

    def torch_graph(self, x, u):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "mlp_linearize_diff", diff_kernel)
    monkeypatch.setattr(ops, "mlp_linearize", kernel)
    monkeypatch.setattr(NNDynamics, "grad_input", torch_graph)
    monkeypatch.setattr(NNDynamics, "forward", torch_graph)

    def route(dx, diff, gm=GradMethods.ANALYTIC):
        x = torch.zeros(4, 3, 5).as_subclass(FakeCuda)
        u = torch.zeros(4, 3, 1).as_subclass(FakeCuda)
        with pytest.raises(_Taken) as e:
            generic.linearize(types.SimpleNamespace(grad_method=gm), x, u, dx, diff)
        return str(e.value)

    two, one = NNDynamics(5, 1, hidden_sizes=[8, 8]), NNDynamics(5, 1, hidden_sizes=[32])
    assert generic.DEVICE_MLP_DEEP is False and generic.DEVICE_MLP_VJP is True
    assert route(two, False) == "torch" and route(two, True) == "torch"
    assert route(one, False) == "device MlpModel" and route(one, True) == "device diff"
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    assert route(two, False) == "device Mlp2Model"
    assert route(two, True) == "torch"
    assert route(two, False, GradMethods.AUTO_DIFF) == "torch"
    assert route(two, False, GradMethods.FINITE_DIFF) == "torch"
    assert route(one, False) == "device MlpModel" and route(one, True) == "device diff"
