"""GPU checks of NNDynamics MPC solves with a slew-rate penalty or with delta_u
on device (generic.DEVICE_MLP_SLEW, generic.DEVICE_MLP_DELTA_U; both ship off
and are turned on here): the control-passthrough model's kernels
(csrc/dilqr_ctrl_through.h, dilqr_mlp_slew_* / dilqr_mlp2_slew_*), the line
search on it, and whole solves and their gradients through dilqr.mpc.MPC.

Oracles.  Kernels: the plain MLP kernels, bit for bit (the adaptor adds only
copies, literal zeros and ones).  Solves: the reference's mpc.MPC on the CPU
(tests/golden/nn_options_f32.npz, gen_golden_nn_options.py) and the torch loop
on the same module (the switches off).  Tolerances are the project's for the
NN problem (tests/test_mlp_gpu.py): 1e-4 for costs, 5e-3 for trajectories and
gradients, a trajectory being held to 3x the reference's own fp32-vs-fp64
spread where that is larger (the stored spreads are all below 1e-3, so 5e-3
stands everywhere); relerr has the max(1, .) normaliser.  B = 65 (one full
wave and a one-lane tail), problem b being fixture problem b % 8.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B65 = 65
T = 10

# tag -> (n, m, hidden, activation, passthrough), the networks of gen_golden_nn_options.py
NETS = {
    "s32": (5, 1, [32], "sigmoid", True),
    "s16x8": (5, 1, [16, 8], "sigmoid", True),
    "r16x8": (5, 1, [16, 8], "relu", True),
    "r16np": (4, 2, [16], "relu", False),
}
# case -> (slew_rate_penalty, bound, uses prev_ctrl, delta_u)
CASES = {
    "slew": (0.5, None, False, None),
    "slew_box": (0.5, 0.2, False, None),
    "slew_prev": (0.5, 1.0, True, None),
    "delta_u": (None, 1.0, False, 0.05),
    "delta_u_big": (None, 1.0, False, 0.3),
}
BASE_SHAPES = [(2, 1), (3, 1), (4, 1), (5, 1), (4, 2)]


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


@pytest.fixture
def switches(monkeypatch):
    """Both new switches (and DEVICE_MLP_DEEP, which the two-hidden-layer
    networks need for any device route) on; switches(False) turns the two new
    ones off again: the torch loop on the same module."""
    from dilqr import generic
    assert generic.DEVICE_MLP_SLEW is False and generic.DEVICE_MLP_DELTA_U is False
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)

    def turn(on):
        monkeypatch.setattr(generic, "DEVICE_MLP_SLEW", on)
        monkeypatch.setattr(generic, "DEVICE_MLP_DELTA_U", on)

    turn(True)
    return turn


def random_net(n, m, hidden, act, pt, seed):
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(seed)
    return NNDynamics(n, m, hidden_sizes=list(hidden), activation=act, passthrough=pt).to(DEV)


def golden_net(g, tag):
    from dilqr.dynamics import NNDynamics
    n, m, hidden, act, pt = NETS[tag]
    dx = NNDynamics(n, m, hidden_sizes=list(hidden), activation=act, passthrough=pt).to(DEV)
    with torch.no_grad():
        for i, fc in enumerate(dx.fcs):
            fc.weight.copy_(gpu(g[f"{tag}_W{i}"]))
            fc.bias.copy_(gpu(g[f"{tag}_b{i}"]))
    return dx


def model_of(dx):
    md = dx.device_model(torch.zeros(1, device=DEV), deep=True)
    assert md is not None
    return md


def solver(n, m, case, B, prev=None, lqr_iter=4):
    import dilqr.mpc as cmpc
    gamma, bound, use_prev, delta_u = CASES[case]
    return cmpc.MPC(n, m, T, lqr_iter=lqr_iter, grad_method=cmpc.GradMethods.ANALYTIC,
                    u_lower=None if bound is None else -bound, u_upper=bound, n_batch=B, exit_unconverged=False,
                    detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=10, slew_rate_penalty=gamma,
                    delta_u=delta_u, prev_ctrl=prev if use_prev else None)


def solve65(g, tag, case, dx):
    from dilqr import QuadCost
    n, m = NETS[tag][:2]
    idx = np.arange(B65) % 8
    mpc = solver(n, m, case, B65, prev=gpu(g[f"{tag}_prev"][idx]))
    with torch.no_grad():
        return mpc(gpu(g[f"{tag}_x0"][idx]), QuadCost(gpu(g[f"{tag}_C"][:, idx]), gpu(g[f"{tag}_c"][:, idx])), dx)


def boom(self, x, u):
    raise AssertionError("NNDynamics.forward called")


# ------------------------------------------------------------------ 1. the adaptor's kernels, exact
@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("hidden", [[8], [8, 4]], ids=["one", "two"])
@pytest.mark.parametrize("nm", BASE_SHAPES, ids=[f"{a}x{b}" for a, b in BASE_SHAPES])
def test_adaptor_kernels_are_the_plain_kernels(nm, hidden, act, pt):
    """The slew rollout and linearisation: the lower block has the plain MLP
    kernels' bits, the upper block is the shifted control / [0 0 I] / 0."""
    from dilqr import ops
    n, m = nm
    md = model_of(random_net(n, m, hidden, act, pt, seed=1000 * n + 100 * m + len(hidden)))
    dyn = ops.slew_dynamics(md)
    assert dyn is not None and (dyn.n, dyn.m) == (n + m, m)
    gen = torch.Generator().manual_seed(17 * n + m)
    for Tk in (1, 2, 10):
        x0 = (0.5 * torch.randn(B65, n, generator=gen)).to(DEV)
        prev = torch.randn(B65, m, generator=gen).to(DEV)
        u = (0.5 * torch.randn(Tk, B65, m, generator=gen)).to(DEV)
        xs = torch.full((Tk, B65, n + m), float("nan"), device=DEV)
        dyn.rollout(torch.cat((prev, x0), 1).contiguous(), u, xs)
        xb = ops.mlp_rollout(md, x0, u)
        assert torch.isfinite(xb).all()
        assert torch.equal(xs[:, :, m:], xb)
        assert torch.equal(xs[:, :, :m], torch.cat((prev.unsqueeze(0), u[:-1]), 0))
        Fs, fs = dyn.linearize(xs, u)
        Fb, fb = ops.mlp_linearize(md, xb, u)
        assert Fs.shape == (Tk - 1, B65, n + m, n + 2 * m) and fs.shape == (Tk - 1, B65, n + m)
        assert torch.equal(Fs[:, :, m:, m:], Fb) and torch.equal(fs[:, :, m:], fb)
        assert torch.equal(Fs[:, :, m:, :m], torch.zeros(Tk - 1, B65, n, m, device=DEV))
        top = torch.cat((torch.zeros(m, n + m), torch.eye(m)), 1).to(DEV).expand(Tk - 1, B65, m, n + 2 * m)
        assert torch.equal(Fs[:, :, :m], top)
        assert torch.equal(fs[:, :, :m], torch.zeros(Tk - 1, B65, m, device=DEV))


# ------------------------------------------------------------------ 2. the line search on the adaptor
@pytest.mark.parametrize("bounds", ["none", "scalar", "tensor"])
def test_line_search_on_the_slew_handle(golden, bounds):
    """ops.lqr_forward on the slew handle against generic.lqr_step_forward with
    the torch line search on CtrlPassthroughDynamics (the switches off): the
    same HIP sweep, then the device line search vs torch's."""
    from dilqr import QuadCost, generic, ops
    g = golden("nn_options_f32")
    tag = "s32"
    n, m = NETS[tag][:2]
    idx = np.arange(B65) % 8
    dx = golden_net(g, tag)
    dyn = ops.slew_dynamics(model_of(dx))
    x0, C, c = ops.slew_problem(gpu(g[f"{tag}_x0"][idx]), gpu(g[f"{tag}_C"][:, idx]), gpu(g[f"{tag}_c"][:, idx]), 0.5,
                                gpu(g[f"{tag}_prev"][idx]), m)
    gen = torch.Generator().manual_seed(5)
    u = (0.1 * torch.randn(T, 8, m, generator=gen))[:, idx].to(DEV).contiguous()
    x = torch.empty(T, B65, n + m, device=DEV)
    dyn.rollout(x0, u, x)
    F, _ = dyn.linearize(x, u)
    if bounds == "none":
        lo = hi = None
    elif bounds == "scalar":
        lo, hi = -0.2, 0.2
    else:
        lo = (-0.2 - 0.1 * torch.rand(T, 8, m, generator=gen))[:, idx].to(DEV).contiguous()
        hi = (0.2 + 0.1 * torch.rand(T, 8, m, generator=gen))[:, idx].to(DEV).contiguous()
    K, k, _ = ops.delta_sweep(C, c, F, n + m, m, x, u, lo, hi)
    nx, nu, cost, du_sq, alpha = ops.lqr_forward(dyn, None, x0, C, c, x, u, K, k, u_lower=lo, u_upper=hi,
                                                 linesearch_decay=0.2, max_linesearch_iter=10)
    fdn = ops.quirk_norm(du_sq)
    assert generic.DEVICE_MLP_SLEW is False
    tx, tu, tcost, tfdn, talpha, _ = generic.lqr_step_forward(
        T, n + m, m, x0, C, c, F, x, u, QuadCost(C, c), generic.CtrlPassthroughDynamics(dx), lo, hi, None, 0.2, 10,
        extras=True)
    errs = {"x": relerr(cpu(nx), cpu(tx)), "u": relerr(cpu(nu), cpu(tu)), "costs": relerr(cpu(cost), cpu(tcost)),
            "full_du_norm": relerr(cpu(fdn), cpu(tfdn)), "mean_alpha": abs(float(alpha.mean()) - float(talpha.mean()))}
    print(f"\n[slew line search, bounds {bounds}] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert max(errs.values()) < 1e-4, errs


# ------------------------------------------------------------------ 3. solves against the reference
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("tag", list(NETS))
def test_solves_against_reference(golden, switches, tag, case):
    g = golden("nn_options_f32")
    dx = golden_net(g, tag)
    idx = np.arange(B65) % 8
    x, u, costs = solve65(g, tag, case, dx)
    key = f"{tag}_{case}"
    errs = {"costs": relerr(cpu(costs), g[f"{key}_costs"][idx]), "x": relerr(cpu(x), g[f"{key}_x"][:, idx]),
            "u": relerr(cpu(u), g[f"{key}_u"][:, idx])}
    spread = {k: float(g[f"{key}_spread_{k}"]) for k in ("x", "u", "costs")}
    print(f"\n[{key} B=65 device vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items())
          + "; the reference's fp32 spread " + ", ".join(f"{a} {b:.2e}" for a, b in spread.items()))
    assert spread["costs"] < 1e-5
    assert errs["costs"] < 1e-4, errs
    assert errs["x"] < max(5e-3, 3 * spread["x"]) and errs["u"] < max(5e-3, 3 * spread["u"]), errs
    # lanes are independent: every copy of a fixture problem is the same bits
    first = torch.as_tensor(idx, device=DEV)
    assert torch.equal(x, x[:, first]) and torch.equal(u, u[:, first]) and torch.equal(costs, costs[first])
    # the torch loop on the same inputs
    switches(False)
    xt, ut, costs_t = solve65(g, tag, case, dx)
    err = relerr(cpu(costs), cpu(costs_t))
    print(f"[{key} B=65 device vs torch loop] costs {err:.2e}, x {relerr(cpu(x), cpu(xt)):.2e}, "
          f"u {relerr(cpu(u), cpu(ut)):.2e}")
    assert err < 1e-4


def test_delta_u_solve_on_cartpole(golden):
    """ops.mpc_solve_unfused(delta_u=...) works for any handle: cartpole against
    the reference's delta_u case (tests/test_generic.py::test_delta_u_trust_region's
    settings and tolerance)."""
    from dilqr import _native as N
    from dilqr import ops
    from dilqr.env_dx.cartpole import CartpoleDx
    g = golden("generic_f32")
    Tc, B = g["delta_u_x"].shape[:2]
    dx = CartpoleDx()
    q, p = dx.get_true_obj()
    C, c = torch.diag(q).repeat(Tc, B, 1, 1).to(DEV), p.repeat(Tc, B, 1).to(DEV)
    x0 = gpu(g["cart_auto_x0"])
    ws = ops.mpc_solve_unfused(N.MODEL_CARTPOLE, ops.theta_of(dx, x0), x0, C, c, Tc, u_lower=-10.0, u_upper=10.0,
                               lqr_iter=5, eps=0.0, linesearch_decay=0.5, max_linesearch_iter=2,
                               not_improved_lim=10 ** 9, delta_u=1.0)
    errs = {"costs": relerr(cpu(ws.best_cost), g["delta_u_costs"]), "u": relerr(cpu(ws.best_u), g["delta_u_u"]),
            "x": relerr(cpu(ws.best_x), g["delta_u_x"])}
    print("\n[cartpole delta_u, mpc_solve_unfused vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert errs["costs"] < 1e-3 and errs["u"] < 1e-3, errs


# ------------------------------------------------------------------ 4. the device path really ran
@pytest.mark.parametrize("case", ["slew_box", "delta_u"])
@pytest.mark.parametrize("tag", ["s32", "s16x8"])
def test_device_path_really_ran(golden, switches, monkeypatch, tag, case):
    """The device solve never evaluates the Module; the torch loop must."""
    from dilqr.dynamics import NNDynamics
    g = golden("nn_options_f32")
    dx = golden_net(g, tag)
    monkeypatch.setattr(NNDynamics, "forward", boom)
    x, u, costs = solve65(g, tag, case, dx)
    assert relerr(cpu(costs), g[f"{tag}_{case}_costs"][np.arange(B65) % 8]) < 1e-4
    switches(False)
    with pytest.raises(AssertionError, match="forward called"):
        solve65(g, tag, case, dx)


# ------------------------------------------------------------------ 5. the other shapes
@pytest.mark.parametrize("hidden", [[8], [8, 4]], ids=["one", "two"])
@pytest.mark.parametrize("nm", [s for s in BASE_SHAPES if s != (5, 1)], ids=["2x1", "3x1", "4x1", "4x2"])
def test_other_shapes_against_torch_loop(switches, nm, hidden):
    """A small random network per remaining base shape, 3 iterations at +-0.5:
    the device route against the torch loop, with a slew-rate penalty and with
    delta_u."""
    import dilqr.mpc as cmpc
    from dilqr import QuadCost
    n, m = nm
    d = n + m
    dx = random_net(n, m, hidden, "sigmoid", True, seed=31 * n + m)
    rng = np.random.RandomState(100 * n + m)
    L = rng.normal(size=(T, B65, d, d)) * 0.3
    C, c = gpu(L @ np.swapaxes(L, -1, -2) + np.eye(d)), gpu(0.1 * rng.normal(size=(T, B65, d)))
    x0 = gpu(0.3 * rng.normal(size=(B65, n)))
    for opt in (dict(slew_rate_penalty=0.5), dict(delta_u=0.1)):
        costs = {}
        for on in (True, False):
            switches(on)
            mpc = cmpc.MPC(n, m, T, lqr_iter=3, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-0.5, u_upper=0.5,
                           n_batch=B65, exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2,
                           max_linesearch_iter=10, **opt)
            with torch.no_grad():
                costs[on] = cpu(mpc(x0, QuadCost(C, c), dx)[2])
        err = relerr(costs[True], costs[False])
        print(f"\n[(n, m) = {nm}, hidden {hidden}, {opt}] device vs torch loop: costs {err:.2e}")
        assert err < 1e-4, (opt, err)


# ------------------------------------------------------------------ 6. gradients
@pytest.mark.parametrize("case", ["slew_box", "delta_u"])
@pytest.mark.parametrize("tag", ["s32", "s16x8"])
def test_gradients(golden, switches, tag, case):
    """Forward and backward through dilqr.mpc.MPC on the device route and on the
    torch route: gradients into x_init, C, c and every parameter.  The loss
    weighs the first copy of each fixture problem only (b < 8), so the
    parameter gradients are the reference's sums over its eight problems."""
    from dilqr import QuadCost
    g = golden("nn_options_f32")
    n, m = NETS[tag][:2]
    idx = np.arange(B65) % 8
    only = (np.arange(B65) < 8).astype(np.float64)[None, :, None]
    wx, wu = gpu(g[f"{tag}_wx"][:, idx] * only), gpu(g[f"{tag}_wu"][:, idx] * only)
    key = f"{tag}_{case}"

    def run():
        dx = golden_net(g, tag)
        X0, C, c = gpu(g[f"{tag}_x0"][idx], True), gpu(g[f"{tag}_C"][:, idx], True), gpu(g[f"{tag}_c"][:, idx], True)
        x, u, costs = solver(n, m, case, B65, prev=gpu(g[f"{tag}_prev"][idx]))(X0, QuadCost(C, c), dx)
        ((x * wx).sum() + (u * wu).sum()).backward()
        out = {"dx0": X0.grad[:8], "dC": C.grad[:, :8], "dc": c.grad[:, :8]}
        rest = max(float(X0.grad[8:].abs().max()), float(C.grad[:, 8:].abs().max()), float(c.grad[:, 8:].abs().max()))
        assert rest == 0.0                                       # problems are independent
        for i, fc in enumerate(dx.fcs):
            out[f"dW{i}"], out[f"db{i}"] = fc.weight.grad, fc.bias.grad
        assert all(v is not None for v in out.values())
        return {k: cpu(v) for k, v in out.items()}

    dev = run()
    switches(False)
    ref = run()
    vs_torch = {k: relerr(dev[k], ref[k]) for k in ref}
    dev_ref = {k: relerr(dev[k], g[f"{key}_{k}"]) for k in ref}
    torch_ref = {k: relerr(ref[k], g[f"{key}_{k}"]) for k in ref}
    print(f"\n[{key} backward] device vs torch route: " + ", ".join(f"{a} {b:.2e}" for a, b in vs_torch.items()))
    print(f"[{key} backward] device vs reference:   " + ", ".join(f"{a} {b:.2e}" for a, b in dev_ref.items()))
    print(f"[{key} backward] torch  vs reference:   " + ", ".join(f"{a} {b:.2e}" for a, b in torch_ref.items()))
    assert len(ref) == 3 + 2 * (len(NETS[tag][2]) + 1)
    assert max(vs_torch.values()) < 5e-3, vs_torch
    missed = {k: v for k, v in dev_ref.items() if torch_ref[k] < 5e-3 and not v < 5e-3}
    assert not missed, missed


# ------------------------------------------------------------------ 7. the LQRStep route
@pytest.mark.parametrize("variant", ["explicit", "classic"])
def test_lqrstep_delta_u_route(golden, switches, monkeypatch, variant):
    """dilqr.LQRStep(..., delta_u=0.25, true_dynamics=nn): with the switch on the
    line search runs on the device model (the Module is never called) and
    equals the torch route."""
    import dilqr
    import dilqr.lqr_step as classic
    from dilqr import ops
    from dilqr.dynamics import NNDynamics
    g = golden("nn_options_f32")
    tag = "s32"
    n, m = NETS[tag][:2]
    idx = np.arange(B65) % 8
    dx = golden_net(g, tag)
    md = model_of(dx)
    x0, C, c = gpu(g[f"{tag}_x0"][idx]), gpu(g[f"{tag}_C"][:, idx]), gpu(g[f"{tag}_c"][:, idx])
    gen = torch.Generator().manual_seed(9)
    u = (0.1 * torch.randn(T, 8, m, generator=gen))[:, idx].to(DEV).contiguous()
    x = ops.mlp_rollout(md, x0, u)
    F, _ = ops.mlp_linearize(md, x, u)
    mod = dilqr if variant == "explicit" else classic

    def step():
        s = mod.LQRStep(n, m, T, u_lower=-1.0, u_upper=1.0, delta_u=0.25, true_cost=dilqr.QuadCost(C, c),
                        true_dynamics=dx, current_x=x, current_u=u)
        with torch.no_grad():
            return s(x0, C, c, F)[:2]

    switches(False)
    tx, tu = step()
    with monkeypatch.context() as mp:
        mp.setattr(NNDynamics, "forward", boom)
        with pytest.raises(AssertionError, match="forward called"):
            step()
        switches(True)
        nx, nu = step()
    errs = {"x": relerr(cpu(nx), cpu(tx)), "u": relerr(cpu(nu), cpu(tu))}
    print(f"\n[LQRStep {variant} delta_u, device vs torch line search] x {errs['x']:.2e}, u {errs['u']:.2e}")
    assert max(errs.values()) < 1e-4, errs
    # the trust region held
    assert float((nu - u).abs().max()) <= 0.25 + 1e-6 and float(nu.abs().max()) <= 1.0
