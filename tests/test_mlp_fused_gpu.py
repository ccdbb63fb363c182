"""GPU checks of the fused MPC path on the one-hidden-layer network
(csrc/dilqr_mlp_fused.h: dilqr_mlp_ilqr_iterate_f32, dilqr_mlp_mpc_solve_small_f32)
and of the route ops.mpc_solve_unfused takes through it.

The contract is equality of bits with the four-launch route (linearise, Riccati
sweep, line search, best-iterate/stop rule), which the fused kernels share their
arithmetic with; the reference's goldens (generic_f32 case J) are checked at the
project's tolerances for that fixture (tests/test_mlp_gpu.py).  Everything is
seeded on the CPU.
"""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def gpu(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV, requires_grad=grad)


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ problems
# A batch is built to hold every line-search outcome.  The weights are scaled
# up so the network bends within one iLQR step, and three per-problem knobs are
# spread over decades across the batch: the size of x0 and of the starting
# controls (large ones start the hidden units deep in the activation's flat
# tails, where a Gauss-Newton step overshoots by 1 / act'), the control cost
# (a dear control takes small steps and accepts the full one), and, for the
# last N_ASYM problems, an antisymmetric part added to C: the sweep takes C as
# it is while the cost only sees its symmetric part, so the step is no longer
# the cost's Newton step and the search backtracks, for relu and H = 1 as well.
W1_SCALE, W2_SCALE = 24.0, 4.0
R_LO, R_HI = 1e-7, 10.0
S_LO, S_HI = 0.1, 10.0
A_LO, A_HI = 1e-2, 10.0
N_ASYM = 48


def log_spread(lo, hi, k):
    return torch.exp(torch.linspace(math.log(lo), math.log(hi), k))[torch.randperm(k)]


def make_problem(n, m, H, act, pt, T, B, seed, w=None):
    """(network on the GPU, x0 [B,n], u [T,B,m], C [T,B,d,d], c [T,B,d]).  C is
    bitwise symmetric except for the last min(N_ASYM, B) problems."""
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(seed)
    dx = NNDynamics(n, m, hidden_sizes=[H], activation=act, passthrough=pt)
    w1, w2 = w or (W1_SCALE, W2_SCALE)
    with torch.no_grad():
        dx.fcs[0].weight.mul_(w1)
        dx.fcs[1].weight.mul_(w2)
    d = n + m
    s = log_spread(S_LO, S_HI, B)
    x0 = s[:, None] * torch.randn(B, n)
    u = 0.5 * s[None, :, None] * torch.randn(T, B, m)
    L = torch.randn(T, B, d, d) * (0.3 / d ** 0.5)
    C = L @ L.transpose(-1, -2)
    C = 0.5 * (C + C.transpose(-1, -2))
    diag = torch.cat((torch.ones(B, n), log_spread(R_LO, R_HI, B)[:, None].expand(B, m)), 1)
    C = C + torch.diag_embed(diag)[None]
    k = min(N_ASYM, B)
    A = torch.randn(T, k, d, d)
    C[:, B - k:] += log_spread(A_LO, A_HI, k)[None, :, None, None] * (A - A.transpose(-1, -2))
    c = 0.3 * torch.randn(T, B, d)
    return copy.deepcopy(dx).to(DEV), x0.to(DEV), u.to(DEV), C.to(DEV).contiguous(), c.to(DEV).contiguous()


def make_bounds(kind, T, B, m, seed):
    if kind == "none":
        return None, None
    if kind == "scalar":
        return -0.3, 0.3
    g = torch.Generator().manual_seed(seed)
    lo = -(0.1 + 0.4 * torch.rand(T, B, m, generator=g))
    hi = 0.1 + 0.4 * torch.rand(T, B, m, generator=g)
    return lo.to(DEV), hi.to(DEV)


def passes(alpha, decay):
    """The line-search pass each problem accepted, from its final alpha = decay ** p."""
    a = alpha.detach().cpu().double()
    return torch.round(torch.log(a) / math.log(decay)).long()


def unfused_iteration(dyn, x0, C, c, xa, ua, lo, hi, decay, max_ls, old_cost):
    """linearise -> sweep -> line search: the three launches of one iteration."""
    from dilqr import _native as N
    from dilqr import ops
    T, B, n = xa.shape
    m = ua.shape[2]
    bounds, keep = N.make_bounds(lo, hi)
    F, _ = dyn.linearize(xa, ua)
    K, k, _ = ops.lqr_backward(C, c, F, n, m, x=xa, u=ua, u_lower=lo, u_upper=hi)
    out = (torch.full_like(xa, 7.0), torch.full_like(ua, 7.0), torch.full((B,), 7.0, device=DEV),
           torch.full((T, m, B), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV))
    dyn.line_search(x0, C, c, xa, ua, K, k, bounds, None, decay, max_ls, *out, old_cost=old_cost)
    del keep
    return out


def fused_iteration(dyn, x0, C, c, xa, ua, lo, hi, decay, max_ls, old_cost, ctrl=None):
    from dilqr import _native as N
    from dilqr import ops
    T, B, n = xa.shape
    m = ua.shape[2]
    bounds, keep = N.make_bounds(lo, hi)
    ws = torch.full((T * B * ops.ilqr_ws_floats(n, m),), 7.0, device=DEV)
    out = (torch.full_like(xa, 7.0), torch.full_like(ua, 7.0), torch.full((B,), 7.0, device=DEV),
           torch.full((T, m, B), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV))
    dyn.fused_iterate(x0, C, c, xa, ua, bounds, decay, max_ls, ws, *out, old_cost=old_cost, ctrl=ctrl)
    del keep
    return out


NAMES = ("x_out", "u_out", "cost", "du_sq", "alpha")
LS = ((1, 0.2), (2, 0.5), (5, 0.2))


def check_iteration(n, m, H, act, pt, bkind, T, B, seed, ls=LS, coverage=True):
    from dilqr import ops
    dx, x0, u, C, c = make_problem(n, m, H, act, pt, T, B, seed)
    md = dx.device_model(x0)
    assert md is not None and (md.n, md.m, md.H) == (n, m, H)
    dyn = ops.Dynamics(md, n, m)
    xa = ops.mlp_rollout(md, x0, u)
    lo, hi = make_bounds(bkind, T, B, m, seed + 1)
    oc = ops.quad_traj_cost(xa, u, C, c).contiguous()
    hist = {}
    for max_ls, decay in ls:
        for old in (None, oc):
            ref = unfused_iteration(dyn, x0, C, c, xa, u, lo, hi, decay, max_ls, old)
            got = fused_iteration(dyn, x0, C, c, xa, u, lo, hi, decay, max_ls, old)
            p = passes(ref[4], decay)
            cnt = torch.bincount(p, minlength=max_ls).tolist()
            hist[(max_ls, decay, old is not None)] = cnt
            tag = f"n={n} m={m} H={H} {act} pt={pt} {bkind} T={T} max_ls={max_ls} decay={decay} old={old is not None}"
            print(f"[fused iteration {tag}] accepted passes {cnt}")
            assert bool(torch.isfinite(ref[2]).all()), tag
            if coverage:
                # the batch must hold every kind of line-search outcome max_ls allows
                assert cnt[0] > 0, (tag, cnt)
                if max_ls >= 2:
                    assert sum(cnt[1::2]) > 0, (tag, cnt)
                if max_ls >= 3:
                    assert sum(cnt[2::2]) > 0, (tag, cnt)
            for name, a, b in zip(NAMES, got, ref):
                assert same_bits(a, b), (tag, name, relerr(cpu(a), cpu(b)))
    return hist


SHAPES = [(5, 1), (2, 1), (4, 2), (6, 2), (4, 3)]
# chosen against the four-launch route on an MI355X: with it every combination below holds all the
# line-search outcomes its max_ls allows (check_iteration asserts that on the unfused result)
SEED = 59


# ------------------------------------------------------------------ 1. one iteration
@pytest.mark.parametrize("bkind", ["none", "scalar", "tensor"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("nm", SHAPES, ids=[f"{n}x{m}" for n, m in SHAPES])
def test_fused_iteration_equals_three_launches(nm, act, bkind):
    """x_out, u_out, cost, du_sq, alpha of the fused iteration are the bits of
    linearise + sweep + line search, with the old cost summed by the sweep and
    with it given, at T = 6, B = 70 (a full wave and a tail), H in {1, 33},
    passthrough on and off, three line-search settings; the unfused result
    shows the batch accepts pass 0, an odd pass and an even pass >= 2."""
    n, m = nm
    for H in (1, 33):
        for pt in (True, False):
            check_iteration(n, m, H, act, pt, bkind, 6, 70, SEED + 100 * n + 10 * m + H)


@pytest.mark.parametrize("T", [1, 2])
def test_fused_iteration_short_horizons(T):
    """T = 1 (the sweep's peeled step alone, no dynamics step) and T = 2."""
    for bkind in ("none", "scalar"):
        check_iteration(5, 1, 33, "sigmoid", True, bkind, T, 70, SEED + T, coverage=False)


def test_fused_iteration_is_a_noop_once_stopped():
    from dilqr import _native as N
    from dilqr import ops
    n, m, T, B = 5, 1, 6, 70
    dx, x0, u, C, c = make_problem(n, m, 33, "sigmoid", True, T, B, SEED)
    md = dx.device_model(x0)
    dyn = ops.Dynamics(md, n, m)
    xa = ops.mlp_rollout(md, x0, u)
    ctrl = torch.zeros(N.CTRL_INTS, dtype=torch.int32, device=DEV)
    ctrl[1] = 1
    oc = ops.quad_traj_cost(xa, u, C, c).contiguous()
    for old in (None, oc):
        got = fused_iteration(dyn, x0, C, c, xa, u, -0.3, 0.3, 0.5, 2, old, ctrl=ctrl)
        for name, a in zip(NAMES, got):
            assert bool((a == 7.0).all()), name
    ctrl[1] = 0                                              # and with the flag down it runs
    got = fused_iteration(dyn, x0, C, c, xa, u, -0.3, 0.3, 0.5, 2, None, ctrl=ctrl)
    assert not bool((got[0] == 7.0).any())
    assert ctrl.tolist() == [0] * N.CTRL_INTS                # the iteration itself leaves the word alone


# ------------------------------------------------------------------ 2. the whole solve
FIELDS = ("best_x", "best_u", "best_cost", "best_du", "fdn")


def solve(md, x0, C, c, T, fused, monkeypatch, small=False, **kw):
    """fused: ops.MLP_FUSED; small: the one-launch solve switched on (it ships off)."""
    from dilqr import ops
    monkeypatch.setattr(ops, "MLP_FUSED", fused)
    monkeypatch.setattr(ops, "MLP_SMALL_MAX_BATCH", ops.SMALL_BATCH_MAX if small else 0)
    ws = ops.mpc_solve_unfused(md, None, x0, C, c, T, u_lower=-1.0, u_upper=1.0, lqr_iter=6, linesearch_decay=0.5,
                               max_linesearch_iter=3, **kw)
    torch.cuda.synchronize()
    return ws


@pytest.mark.parametrize("B", [1, 65, 256, 257])
@pytest.mark.parametrize("nmH", [(5, 1, 32), (4, 2, 8), (6, 2, 8)], ids=["5x1_H32", "4x2_H8", "6x2_H8"])
def test_solve_route_equals_four_launch_route(nmH, B, monkeypatch):
    """MLP_FUSED on against off: the same bits in best_x, best_u, best_cost,
    best_du, fdn and the same (iter, stopped, n_not_improved), at B = 1, 65 (two
    waves in the one-launch kernel: the quirk rows read another wave's du_sq),
    256 and 257 (the per-iteration route, with a tail), with the stop rule
    unable to fire, firing on eps, and firing on "not improved"; u_init None
    and given."""
    from dilqr import ops
    n, m, H = nmH
    T = 5
    dx, x0, u, C, c = make_problem(n, m, H, "sigmoid", True, T, B, SEED + B, w=(4.0, 2.0))
    md = dx.device_model(x0)
    # the routes to hold against the four launches: the fused iteration per launch (what ships), and
    # up to one workgroup's batch the one-launch solve too ((6, 2) has none)
    assert ops.mlp_solve_route(md, B, 6, None, 0) == "fused"
    monkeypatch.setattr(ops, "MLP_SMALL_MAX_BATCH", ops.SMALL_BATCH_MAX)
    has_small = B <= 256 and (n, m) != (6, 2)
    assert ops.mlp_solve_route(md, B, 6, None, 0) == ("small" if has_small else "fused")
    monkeypatch.setattr(ops, "MLP_SMALL_MAX_BATCH", 0)
    for u_init in (None, u):
        # the max row norm after each iteration, from the logged four-launch loop
        log = ops.mpc_solve_unfused(md, None, x0, C, c, T, u_lower=-1.0, u_upper=1.0, lqr_iter=6,
                                    linesearch_decay=0.5, max_linesearch_iter=3, eps=0.0, not_improved_lim=10 ** 9,
                                    u_init=u_init, verbose=1).log
        # eps just above the latest running minimum among iterations 0..4: the rule (max < eps) first
        # holds there, so the solve stops after that iteration, before the sixth
        mx = log["stats"][:5, 1].cpu().numpy()
        j = max(i for i in range(5) if mx[i] <= mx[:i + 1].min())
        eps = float(np.nextafter(np.float32(mx[j]), np.float32(np.inf)))
        settings = [
            ("never", dict(eps=0.0, not_improved_lim=10 ** 9), False),
            ("eps", dict(eps=eps), True),
            ("not improved", dict(eps=0.0, not_improved_lim=0, best_cost_eps=-1.0), True),
            ("not improved, lim 2", dict(eps=0.0, not_improved_lim=2, best_cost_eps=-1.0), None),   # may or may not stop
        ]
        settings.append(("eps, polled", dict(eps=eps, check_every=2), True))   # the host's poll breaks the loop
        for name, kw, stops in settings:
            off = solve(md, x0, C, c, T, False, monkeypatch, u_init=u_init, **kw)
            ctl_off = off.ctrl[:3].tolist()
            tag = f"n={n} m={m} B={B} u_init={'given' if u_init is not None else None} {name}"
            print(f"[solve route {tag}] (iter, stopped, n_not_improved) = {ctl_off}")
            if stops:
                assert ctl_off[1] == 1 and ctl_off[0] < 6, (tag, ctl_off)
            elif stops is False:
                assert ctl_off[:2] == [6, 0], (tag, ctl_off)
            assert bool(torch.isfinite(off.best_cost).all()), tag
            for small in ((False, True) if has_small else (False,)):
                on = solve(md, x0, C, c, T, True, monkeypatch, small=small, u_init=u_init, **kw)
                ctl_on = on.ctrl[:3].tolist()
                assert ctl_on == ctl_off, (tag, small, ctl_on, ctl_off)
                for f in FIELDS:
                    assert same_bits(getattr(on, f), getattr(off, f)), (tag, small, f)


# ------------------------------------------------------------------ 3, 4. the reference's goldens
def golden_model(g):
    from dilqr.dynamics import NNDynamics
    dx = NNDynamics(5, 1, hidden_sizes=[32], activation="sigmoid").to(DEV)
    with torch.no_grad():
        for i, fc in enumerate(dx.fcs):
            fc.weight.copy_(gpu(g[f"nn_W{i}"]))
            fc.bias.copy_(gpu(g[f"nn_b{i}"]))
    return dx


def record_calls(monkeypatch):
    from dilqr import _native as N
    names = []
    real = N.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(N, "call", call)
    return names


def expect_route(names, route, final_step=False):
    """The entry points that ran: the new route's, never the unfused per-iteration
    MLP launches (final_step: the backward's one linearisation at the solution)."""
    assert names.count("dilqr_mlp_linearize_f32") == int(final_step), names
    assert "dilqr_mlp_lqr_forward_f32" not in names, names
    if route == "small":
        assert names.count("dilqr_mlp_mpc_solve_small_f32") == 1 and "dilqr_mlp_ilqr_iterate_f32" not in names, names
    else:
        assert names.count("dilqr_mlp_ilqr_iterate_f32") >= 1 and "dilqr_mlp_mpc_solve_small_f32" not in names, names


@pytest.mark.parametrize("route", ["small", "fused"])
@pytest.mark.parametrize("B", [8, 65])
def test_mpc_against_reference_takes_the_new_route(golden, monkeypatch, B, route):
    """generic_f32 case J (the NN problem), its 8 problems and those tiled to
    65: mpc.MPC.forward under no_grad against the reference, through one
    dilqr_mlp_mpc_solve_small_f32 (switched on) or, as shipped, the fused
    iteration per launch, and none of the unfused per-iteration MLP launches."""
    import dilqr.mpc as cmpc
    from dilqr import QuadCost, ops
    monkeypatch.setattr(ops, "MLP_SMALL_MAX_BATCH", ops.SMALL_BATCH_MAX if route == "small" else 0)
    g = golden("generic_f32")
    dx = golden_model(g)
    idx = np.arange(B) % 8
    T = g["nn_C"].shape[0]
    names = record_calls(monkeypatch)
    m = cmpc.MPC(5, 1, T, lqr_iter=4, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0, u_upper=1.0, n_batch=B,
                 exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=10)
    with torch.no_grad():
        x, u, costs = m(gpu(g["nn_x0"][idx]), QuadCost(gpu(g["nn_C"][:, idx]), gpu(g["nn_c"][:, idx])), dx)
    errs = {"costs": relerr(cpu(costs), g["nn_analytic_costs"][idx]), "x": relerr(cpu(x), g["nn_analytic_x"][:, idx]),
            "u": relerr(cpu(u), g["nn_analytic_u"][:, idx])}
    print(f"\n[mlp MPC B={B} route {route} vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert errs["costs"] < 1e-4, errs
    assert max(errs["x"], errs["u"]) < 5e-3, errs
    expect_route(names, route)
    # lanes are independent: every copy of a golden problem is the same bits
    first = torch.as_tensor(idx, device=DEV)
    assert torch.equal(x, x[:, first]) and torch.equal(u, u[:, first]) and torch.equal(costs, costs[first])


@pytest.mark.parametrize("route", ["small", "fused"])
def test_backward_reaches_the_weights_through_the_new_route(golden, monkeypatch, route):
    """tests/test_mlp_gpu.py test_backward_reaches_the_weights with the solve
    taking the new route (the one-launch solve switched on, or the fused
    iteration as shipped), then the torch final_step; gradients into the
    network, the cost and x_init against the reference."""
    import dilqr.mpc as cmpc
    from dilqr import QuadCost, generic, ops
    monkeypatch.setattr(ops, "MLP_SMALL_MAX_BATCH", ops.SMALL_BATCH_MAX if route == "small" else 0)
    g = golden("generic_f32")
    dx = golden_model(g)
    T, B = g["nn_C"].shape[:2]
    assert B == 8 and generic.DEVICE_MLP is True
    names = record_calls(monkeypatch)
    X0, C, c = gpu(g["nn_x0"], True), gpu(g["nn_C"], True), gpu(g["nn_c"], True)
    m = cmpc.MPC(5, 1, T, lqr_iter=4, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0, u_upper=1.0, n_batch=B,
                 exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=10)
    x, u, costs = m(X0, QuadCost(C, c), dx)
    expect_route(names, route, final_step=True)
    assert relerr(cpu(costs), g["nn_analytic_costs"]) < 1e-4
    assert relerr(cpu(u), g["nn_analytic_u"]) < 5e-3
    assert relerr(cpu(x), g["nn_analytic_x"]) < 5e-3
    ((x * gpu(g["nn_wx"])).sum() + (u * gpu(g["nn_wu"])).sum()).backward()
    errs = {"dx0": relerr(cpu(X0.grad), g["nn_analytic_dx0"]), "dC": relerr(cpu(C.grad), g["nn_analytic_dC"]),
            "dc": relerr(cpu(c.grad), g["nn_analytic_dc"])}
    for i, fc in enumerate(dx.fcs):
        errs[f"dW{i}"] = relerr(cpu(fc.weight.grad), g[f"nn_analytic_dW{i}"])
        errs[f"db{i}"] = relerr(cpu(fc.bias.grad), g[f"nn_analytic_db{i}"])
    print(f"\n[mlp MPC backward, route {route}, vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert max(errs.values()) < 5e-3, errs
