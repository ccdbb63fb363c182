"""GPU checks of closed-loop MPC episodes (dilqr.closed_loop.mpc_episode,
csrc/tu_advance.hip, IL_Env.populate_data2):

  * an episode equals, bit for bit, the composition of calls a user could
    already write (a fresh ops.mpc_solve per step, ops.rollout over the plan's
    first control, the shift in torch), for every env_dx model, warm-start
    mode and solve route;
  * the reference's own closed-loop episodes (tests/golden/closed_loop_*.npz)
    are reproduced in fp32 within max(1e-4, 3 x the reference's fp32-vs-fp64
    spread of that case);
  * the stage-cost log, the model-mismatch plant, a network planner, the
    absence of host synchronisation, and populate_data2's dataset.
"""
import numpy as np
import pytest
import torch

import closed_loop_oracle as clo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMPLEX_PARAMS = (10., 1., 1., 1.0, 0.1)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def gpu(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def make_model(name, params=None, device=None):
    """A dilqr env_dx model by the golden generator's names; params on `device`
    when given (a model whose parameters live on the GPU is uploaded once)."""
    from dilqr.env_dx.cartpole import CartpoleDx
    from dilqr.env_dx.pendulum import PendulumDx
    from dilqr.env_dx.rocket import RocketDx
    if params is None and name == "pendulum-complex":
        params = COMPLEX_PARAMS
    p = None if params is None else torch.tensor(tuple(float(v) for v in params), device=device)
    if name == "pendulum":
        return PendulumDx(p)
    if name == "pendulum-complex":
        return PendulumDx(p, simple=False)
    return (CartpoleDx if name == "cartpole" else RocketDx)(p)


def xinit(name, B, rng):
    if name.startswith("pendulum"):
        th = rng.uniform(-np.pi / 2, np.pi / 2, B)
        return np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, B)], 1)
    if name == "cartpole":
        th = rng.uniform(-0.3, 0.3, B)
        return np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                         rng.uniform(-1, 1, B)], 1)
    r = rng.uniform([0, -4, -2.5], [10, 4, 2.5], (B, 3))
    q = np.array([1., 0, 0, 0]) + 0.05 * rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([r, rng.normal(0, 0.1, (B, 3)), q, rng.normal(0, 0.02, (B, 3))], 1)


def true_cost(dx, T, B):
    q, p = dx.get_true_obj()
    return torch.diag(q).repeat(T, B, 1, 1).to(DEV), p.repeat(T, B, 1).to(DEV)


def shift(u, warm):
    """The three warm-start rules in torch (il_env.py:139-140 for "reference")."""
    if warm == "cold":
        return torch.zeros_like(u)
    w = torch.cat((u[1:], torch.zeros_like(u[:1])), dim=0)
    if warm == "reference":
        w[-2] = w[-3]
    return w


def composition(solve, plant, x0, steps, warm):
    """The loop a caller can write from existing calls: solve(x, u_init) ->
    (plan, best_cost, best_du) from a fresh solve, the plant step as the second
    row of ops.rollout over the plan's first two controls, the shift in torch."""
    from dilqr import ops
    theta = ops.theta_of(plant, x0)
    x, u_init = x0.clone(), None
    xs, us, costs, dus = [x], [], [], []
    for _ in range(steps):
        plan, best_cost, best_du = solve(x, u_init)
        x = ops.rollout(plant.model_id, theta, x, plan[:2].contiguous())[1].clone()
        xs.append(x)
        us.append(plan[0].clone())
        costs.append(best_cost.clone())
        dus.append(best_du.clone())
        u_init = shift(plan, warm)
    return torch.stack(xs), torch.stack(us), torch.stack(costs), torch.stack(dus)


def assert_same_bits(ep, ref, label):
    for name, a, b in zip(("x", "u", "solve_cost", "solve_du"), (ep.x, ep.u, ep.solve_cost, ep.solve_du), ref):
        assert a.shape == b.shape and torch.equal(a, b), (label, name, float((a - b).abs().max()))


# ---------------------------------------------------------------- 1. bit equality with the composition
# (T, steps, B): both horizons, every step count, a lone problem, a partial wave,
# a partial wave after a full one, and a batch past ops.SMALL_BATCH_MAX (the
# polled stop-rule route)
SHAPES = ((3, 1, 1), (3, 2, 3), (5, 5, 65), (5, 2, 300), (3, 5, 300), (5, 1, 3), (5, 2, 1))
ROCKET_SHAPES = ((4, 2, 2), (4, 3, 65))


def solver_settings(route, dx, bounded):
    kw = dict(lqr_iter=4, linesearch_decay=dx.linesearch_decay, max_linesearch_iter=dx.max_linesearch_iter,
              exit_unconverged=False, detach_unconverged=False)
    if route == "fixed":                      # the stop rule cannot fire: one launch per solve
        kw.update(eps=0.0, not_improved_lim=10 ** 9)
    else:                                     # the stop rule: one launch up to 256 problems, polled above
        kw.update(eps=dx.mpc_eps, lqr_iter=6)
    if bounded:
        lim = 2.0 if dx.n_ctrl == 1 else 20.0
        kw.update(u_lower=-lim, u_upper=lim)
    return kw


@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
@pytest.mark.parametrize("route", ["fixed", "stop"])
@pytest.mark.parametrize("name", ["pendulum", "pendulum-complex", "cartpole", "rocket"])
def test_episode_equals_composition_bit_for_bit(name, route, bounded):
    import dilqr
    from dilqr import ops
    from dilqr.closed_loop import mpc_episode
    dx = make_model(name)
    n, m = dx.n_state, dx.n_ctrl
    kw = solver_settings(route, dx, bounded)
    rng = np.random.RandomState(7)
    for T, steps, B in (ROCKET_SHAPES if name == "rocket" else SHAPES):
        mpc = dilqr.MPC(n, m, T, **kw)
        x0 = gpu(xinit(name, B, rng))
        C, c = true_cost(dx, T, B)
        theta = ops.theta_of(dx, x0)
        args = mpc.solver_args()
        args.pop("u_init")

        def solve(x, u_init):
            _, plan, best_cost, best_du, _ = ops.mpc_solve(dx.model_id, theta, x, C, c, T, u_init=u_init, **args)
            return plan, best_cost, best_du

        for warm in ("reference", "shift", "cold"):
            ep = mpc_episode(mpc, x0, dilqr.QuadCost(C, c), dx, steps, warm_start=warm)
            assert ep.x.shape == (steps + 1, B, n) and ep.u.shape == (steps, B, m)
            assert ep.cost.shape == ep.solve_cost.shape == ep.solve_du.shape == (steps, B)
            assert torch.equal(ep.x[0], x0) and not ep.x.requires_grad
            assert_same_bits(ep, composition(solve, dx, x0, steps, warm), (name, route, bounded, T, steps, B, warm))


def test_episode_seeds_step_zero_with_the_mpcs_u_init():
    import dilqr
    from dilqr import ops
    from dilqr.closed_loop import mpc_episode
    dx = make_model("cartpole")
    T, steps, B = 5, 3, 65
    rng = np.random.RandomState(11)
    u0 = gpu(rng.uniform(-1, 1, (T, B, 1)))
    mpc = dilqr.MPC(5, 1, T, u_init=u0, **solver_settings("stop", dx, True))
    x0 = gpu(xinit("cartpole", B, rng))
    C, c = true_cost(dx, T, B)
    theta = ops.theta_of(dx, x0)
    args = mpc.solver_args()
    args.pop("u_init")

    def solve(x, u_init):
        _, plan, bc, bd, _ = ops.mpc_solve(dx.model_id, theta, x, C, c, T, u_init=u0 if u_init is None else u_init,
                                           **args)
        return plan, bc, bd

    ep = mpc_episode(mpc, x0, dilqr.QuadCost(C, c), dx, steps)
    assert_same_bits(ep, composition(solve, dx, x0, steps, "reference"), "u_init")
    cold = mpc_episode(dilqr.MPC(5, 1, T, **solver_settings("stop", dx, True)), x0, dilqr.QuadCost(C, c), dx, steps)
    assert not torch.equal(ep.u, cold.u)


# ---------------------------------------------------------------- 2./3. the reference's episodes
def golden_episode(g, name, plant=True):
    """A stored case through the public mpc_episode; plant=False: the planner's
    own parameters for the plant too (plant=None)."""
    import dilqr
    from dilqr.closed_loop import mpc_episode
    mname = str(g[f"{name}_model"])
    T, steps, lqr_iter, eps, lo, hi, decay, max_ls = g[f"{name}_settings"]
    T, steps = int(T), int(steps)
    planner = make_model(mname, g[f"{name}_planner_params"])
    true = make_model(mname, g[f"{name}_plant_params"])
    kw = {} if np.isnan(lo) else dict(u_lower=float(lo), u_upper=float(hi))
    gm = dilqr.GradMethods.AUTO_DIFF if mname == "pendulum-complex" else dilqr.GradMethods.ANALYTIC
    mpc = dilqr.MPC(true.n_state, true.n_ctrl, T, lqr_iter=int(lqr_iter), eps=float(eps), linesearch_decay=float(decay),
                    max_linesearch_iter=int(max_ls), exit_unconverged=False, detach_unconverged=False,
                    grad_method=gm, **kw)
    x0 = gpu(g[f"{name}_x0"])
    C, c = true_cost(true, T, x0.shape[0])
    return mpc_episode(mpc, x0, dilqr.QuadCost(C, c), planner, steps, plant=true if plant else None)


def case_tol(golden, name):
    g32 = golden("closed_loop_f32")
    return (max(1e-4, 3 * float(g32[f"{name}_spread_x"])), max(1e-4, 3 * float(g32[f"{name}_spread_u"])))


@pytest.mark.parametrize("name", ["pend", "cart", "pend_b1", "pend_mismatch", "pend_t3", "complex", "rocket"])
def test_reference_parity(golden, name):
    """fp32 device against the reference's fp64 episode, each case held to
    max(1e-4, 3 x the reference's own fp32-vs-fp64 spread of that case)."""
    g = golden("closed_loop_f64")
    ep = golden_episode(g, name)
    ex, eu = relerr(cpu(ep.x), g[f"{name}_x"]), relerr(cpu(ep.u), g[f"{name}_u"])
    ec = relerr(cpu(ep.solve_cost), g[f"{name}_plan_costs"])
    tx, tu = case_tol(golden, name)
    print(f"\n[closed loop {name}] x {ex:.2e} (tol {tx:.1e}), u {eu:.2e} (tol {tu:.1e}), plan costs {ec:.2e}")
    assert ex < tx and eu < tu


def test_reference_parity_through_populate_data2(golden, monkeypatch):
    """The B = 1 case is populate_data2 itself: the dataset it fills is the
    reference's cat(x[:-1], u)."""
    from dilqr.il import IL_Env
    g = golden("closed_loop_f64")
    T, steps, lqr_iter = (int(v) for v in g["pend_b1_settings"][:3])
    assert T == steps
    env = IL_Env("pendulum", lqr_iter=lqr_iter, mpc_T=T, device=DEV)
    monkeypatch.setattr(env, "sample_xinit", lambda n_batch=1: torch.tensor(g["pend_b1_x0"], dtype=torch.float32))
    env.populate_data2(1, 0, 0)
    want = np.concatenate([g["pend_b1_x"][:-1], g["pend_b1_u"]], 2).transpose(1, 0, 2)
    assert tuple(env.train_data.shape) == want.shape == (1, T, 4)
    tx, tu = case_tol(golden, "pend_b1")
    assert relerr(cpu(env.train_data)[..., :3], want[..., :3]) < tx
    assert relerr(cpu(env.train_data)[..., 3:], want[..., 3:]) < tu


def test_model_mismatch_plant(golden):
    """A planner with wrong parameters against the true plant: its episode is
    the golden's, and not the one in which the plant has the planner's
    parameters."""
    g = golden("closed_loop_f64")
    ep = golden_episode(g, "pend_mismatch")
    same = golden_episode(g, "pend_mismatch", plant=False)
    tx, tu = case_tol(golden, "pend_mismatch")
    assert relerr(cpu(ep.x), g["pend_mismatch_x"]) < tx and relerr(cpu(ep.u), g["pend_mismatch_u"]) < tu
    assert relerr(cpu(same.x), g["pend_mismatch_x"]) > 100 * tx
    assert not torch.equal(ep.x[1], same.x[1])


# ---------------------------------------------------------------- 4. the stage-cost log
@pytest.mark.parametrize("name,B", [("cartpole", 65), ("rocket", 3), ("pendulum", 300)])
def test_cost_log(name, B):
    """cost[s] = 0.5 tau^T C_0 tau + c_0^T tau at the logged (x_s, u_s), against
    fp64 numpy within 1e-5 relative (the bound test_lqr_step_explicit holds costs
    to), on a dense SPD C and a random c."""
    import dilqr
    from dilqr.closed_loop import mpc_episode
    dx = make_model(name)
    n, m = dx.n_state, dx.n_ctrl
    d, T, steps = n + m, 4, 3
    rng = np.random.RandomState(5)
    L = 0.3 * rng.normal(size=(T, B, d, d))
    C = L @ np.swapaxes(L, -1, -2) + np.eye(d)
    c = 0.1 * rng.normal(size=(T, B, d))
    mpc = dilqr.MPC(n, m, T, **solver_settings("fixed", dx, True))
    ep = mpc_episode(mpc, gpu(xinit(name, B, rng)), dilqr.QuadCost(gpu(C), gpu(c)), dx, steps, warm_start="shift")
    C0, c0 = cpu(gpu(C[0])), cpu(gpu(c[0]))                    # the fp32 cost the kernel read
    for s in range(steps):
        want = clo.stage_cost(cpu(ep.x[s]), cpu(ep.u[s]), C0, c0)
        err = np.abs(cpu(ep.cost[s]) - want) / np.maximum(1.0, np.abs(want))
        assert err.max() < 1e-5, (s, err.max())


# ---------------------------------------------------------------- 5. a network planner
def test_nn_planner_equals_composition_bit_for_bit():
    """A (3,1) [16] sigmoid NNDynamics planning for the true pendulum: the
    episode is the composition built from ops.mpc_solve_unfused."""
    import dilqr
    from dilqr import ops
    from dilqr.closed_loop import mpc_episode
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(3)
    net = NNDynamics(3, 1, hidden_sizes=(16,), activation="sigmoid").to(DEV)
    plant = make_model("pendulum")
    T, steps, B = 5, 3, 5
    mpc = dilqr.MPC(3, 1, T, **solver_settings("stop", plant, True))
    x0 = gpu(xinit("pendulum", B, np.random.RandomState(9)))
    C, c = true_cost(plant, T, B)
    mlp = net.device_model(x0)
    assert isinstance(mlp, ops.MlpModel)
    args = mpc.solver_args()
    args.pop("u_init")

    def solve(x, u_init):
        ws = ops.mpc_solve_unfused(mlp, None, x, C, c, T, u_init=u_init, **args)
        return ws.best_u, ws.best_cost, ws.best_du

    for warm in ("reference", "cold"):
        ep = mpc_episode(mpc, x0, dilqr.QuadCost(C, c), net, steps, plant=plant, warm_start=warm)
        assert_same_bits(ep, composition(solve, plant, x0, steps, warm), ("nn", warm))
    # the states are the plant's, not the network's prediction
    assert torch.equal(ep.x[1], plant(x0, ep.u[0]))


# ---------------------------------------------------------------- 6. no host synchronisation
@pytest.mark.parametrize("route,B", [("fixed", 65), ("fixed", 300), ("stop", 65)])
def test_episode_does_not_synchronise(route, B):
    """With its inputs on the device, an episode on the fixed-count route or
    the one-launch stop-rule route (B <= ops.SMALL_BATCH_MAX) never waits for
    the GPU: it runs under torch's sync debug mode set to "error", which this
    test first shows to catch a .item()."""
    import dilqr
    from dilqr.closed_loop import mpc_episode
    dx = make_model("cartpole", (9.8, 1.0, 0.1, 0.5), device=DEV)
    T, steps = 5, 3
    mpc = dilqr.MPC(5, 1, T, **solver_settings(route, dx, True))
    x0 = gpu(xinit("cartpole", B, np.random.RandomState(2)))
    C, c = true_cost(dx, T, B)
    cost = dilqr.QuadCost(C, c)
    first = mpc_episode(mpc, x0, cost, dx, steps)              # loads the kernels
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            x0.sum().item()                                     # the mode is honoured
        ep = mpc_episode(mpc, x0, cost, dx, steps)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert torch.equal(ep.x, first.x) and torch.equal(ep.u, first.u)


# ---------------------------------------------------------------- 7. populate_data2
@pytest.mark.parametrize("env_name", ["pendulum", "cartpole", "pendulum-complex"])
def test_populate_data2(env_name):
    from dilqr.il import IL_Env
    T = 5
    env = IL_Env(env_name, lqr_iter=5, mpc_T=T, device=DEV)
    n, m = env.true_dx.n_state, env.true_dx.n_ctrl
    ep = env.populate_data2(3, 2, 2, seed=4)
    for data, rows in ((env.train_data, 3), (env.val_data, 2), (env.test_data, 2)):
        assert tuple(data.shape) == (rows, T, n + m)
    torch.manual_seed(4)
    xinit_ = env.sample_xinit(n_batch=7).to(DEV)
    tau = torch.cat((env.train_data, env.val_data, env.test_data), 0)
    assert torch.equal(tau[:, 0, :n], xinit_)
    assert torch.equal(tau[:, :, :n], ep.x[:-1].transpose(0, 1)) and torch.equal(tau[:, :, n:], ep.u.transpose(0, 1))
    # consecutive states satisfy the plant's forward, bit for bit
    for t in range(T):
        assert torch.equal(ep.x[t + 1], env.true_dx(ep.x[t], ep.u[t])), t
