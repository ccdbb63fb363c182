"""Closed-loop (receding-horizon) MPC episodes on device: solve, apply the
plan's first control to the plant, shift the plan into the next warm start,
solve again — the loop of the reference's IL_Env.populate_data2
(il_env.py:96-151) and of its test_mpc.py gym demo, batched.

Every solve is one of the existing launches, unchanged (ops.mpc_solve for an
env_dx planner, ops.mpc_solve_unfused for a one-hidden-layer NNDynamics); the
step between two solves is one more launch (ops.mpc_advance,
csrc/tu_advance.hip) that writes the next solve's x_init and u_init into
device buffers and the episode's logs.  The driver queues steps x (solve,
advance) on the current stream.  With inputs already on the device, a
fixed-count solve (eps <= 0, not_improved_lim >= lqr_iter) or a stop-rule solve
of at most ops.SMALL_BATCH_MAX problems of a thread-per-problem model never
synchronises with the host; the other routes keep the stop polls their solves
have.  An episode is bit for bit the composition of those calls a caller could
write: a fresh ops.mpc_solve, ops.rollout over the plan's first control, the
shift in torch.

There is no torch fallback: what the launches do not cover is refused with a
NotImplementedError that names the reason.
"""
import collections

import torch

from . import ops
from .definitions import LinDx, QuadCost
from .mpc_explicit import expand_cost

Episode = collections.namedtuple("Episode", "x u cost solve_cost solve_du")
Episode.__doc__ = """x [steps+1,B,n]: the plant's states, x[0] = x_init; u [steps,B,m]: the applied
controls as the solver gave them; cost [steps,B]: the t = 0 stage cost
0.5 tau^T C_0 tau + c_0^T tau at (x[s], u[s]); solve_cost, solve_du [steps,B]:
each solve's best cost and the du norm of its best iterate (above the MPC's eps
where it did not converge)."""


def _refuse(why):
    raise NotImplementedError(f"dilqr: mpc_episode: {why}")


def _route(mpc, x_init, cost, dx, plant, T, warm_start):
    """("env", model_id) or ("nn", MlpModel), after every refusal."""
    if not isinstance(cost, QuadCost):
        _refuse("a non-quadratic cost is not on the device path")
    if mpc.slew_rate_penalty is not None:
        _refuse("slew_rate_penalty is not supported in an episode")
    if mpc.delta_u is not None:
        _refuse("delta_u is not supported in an episode")
    if getattr(mpc, "verbose", 0) > 0:
        _refuse("verbose > 0 is not supported (the solve log needs the host)")
    if isinstance(dx, LinDx) or isinstance(plant, LinDx):
        _refuse("LinDx dynamics have no plant to advance")
    if getattr(plant, "model_id", None) is None:
        _refuse("the plant must be a dilqr.env_dx model (pass plant=... for a learned planner)")
    if warm_start == "reference" and T < 3:
        _refuse('warm_start="reference" needs T >= 3 (the reference indexes u_init[-3], il_env.py:140)')
    if (plant.n_state, plant.n_ctrl) != (mpc.n_state, mpc.n_ctrl):
        raise ValueError(f"mpc_episode: the plant is (n, m) = {(plant.n_state, plant.n_ctrl)}, the MPC "
                         f"{(mpc.n_state, mpc.n_ctrl)}")
    if getattr(dx, "model_id", None) is not None:
        if plant.model_id != dx.model_id:
            raise ValueError("mpc_episode: planner and plant must be the same env_dx model (their params may differ)")
        if not mpc.fused(cost, dx):
            _refuse("this grad_method has no fused solve for the model")
        if mpc.u_zero_I is not None:
            _refuse("u_zero_I is not supported with an env_dx planner")
        return "env", dx.model_id
    if not x_init.is_cuda:
        raise RuntimeError("dilqr: x_init must be on the GPU (no CPU path)")
    from . import generic
    mlp = generic.device_solve_ok(mpc, cost, dx, x_init)
    if not isinstance(mlp, ops.MlpModel) or (mlp.n, mlp.m) != (mpc.n_state, mpc.n_ctrl):
        _refuse("the planner must be an env_dx model or a one-hidden-layer NNDynamics with a device model of the "
                "MPC's (n, m), under the ANALYTIC linearisation")
    return "nn", mlp


def mpc_episode(mpc, x_init, cost, dx, steps, plant=None, warm_start="reference"):
    """`steps` control steps of receding-horizon MPC from x_init [B,n].

    mpc: a dilqr.MPC or dilqr.mpc.MPC; its options are those of every solve
    (MPC.solver_args), its u_init seeds step 0.  cost: a QuadCost, expanded as
    MPC.forward expands it and reused at every step, as the reference does.
    dx: the planner's model, an env_dx model or a one-hidden-layer NNDynamics
    with a device model.  plant: the env_dx model the controls are applied to
    (default dx): for an env_dx planner the same model, its params free to
    differ (the model mismatch of the IL experiments); any env_dx model of the
    planner's (n, m) for a network.  warm_start: "reference" (populate_data2's
    rule with its quirk: u[T-2] used twice, u[T-1] dropped), "shift" (the plain
    shift with a zero tail) or "cold" (zeros).

    Returns an Episode; everything in it is detached (no gradient flows through
    an episode).  solve_cost and solve_du are copied on the stream, so where a
    solve did not converge is visible without a synchronisation (they stand in
    for MPC.forward's unconverged warning, which needs one)."""
    if warm_start not in ops.WARM_MODES:
        raise ValueError(f"mpc_episode: warm_start must be one of {sorted(ops.WARM_MODES)}, got {warm_start!r}")
    steps = int(steps)
    if steps < 1:
        raise ValueError("mpc_episode: steps must be at least 1")
    plant = dx if plant is None else plant
    T, n, m = mpc.T, mpc.n_state, mpc.n_ctrl
    kind, planner = _route(mpc, x_init, cost, dx, plant, T, warm_start)
    if not x_init.is_cuda:
        raise RuntimeError("dilqr: x_init must be on the GPU (no CPU path)")
    if x_init.ndimension() != 2 or x_init.shape[1] != n:
        raise ValueError(f"mpc_episode: x_init must be [B, {n}], got {tuple(x_init.shape)}")
    B = x_init.shape[0]
    if mpc.n_batch is not None and mpc.n_batch != B:
        raise ValueError(f"mpc_episode: x_init has {B} rows, the MPC's n_batch is {mpc.n_batch}")
    C, c = expand_cost(cost.C, cost.c, T, B, n + m)
    if tuple(C.shape) != (T, B, n + m, n + m) or tuple(c.shape) != (T, B, n + m):
        raise ValueError(f"mpc_episode: the cost must expand to C {(T, B, n + m, n + m)}, c {(T, B, n + m)}; got "
                         f"{tuple(C.shape)}, {tuple(c.shape)}")
    dev = x_init.device
    with torch.no_grad():
        C, c = ops._f32(C.to(dev)), ops._f32(c.to(dev))
        x_cur = ops._f32(x_init).clone()
        args = mpc.solver_args()
        u0 = args.pop("u_init")
        theta = dx._theta(x_cur) if kind == "env" else None
        theta_plant = plant._theta(x_cur)
        u_warm = torch.empty(T, B, m, device=dev)
        x = torch.empty(steps + 1, B, n, device=dev)
        u = torch.empty(steps, B, m, device=dev)
        stage, solve_cost, solve_du = (torch.empty(steps, B, device=dev) for _ in range(3))
        x[0].copy_(x_cur)
        for s in range(steps):
            # a fresh solve per step (its state block is not shown to reset everything
            # the next solve reads; the caching allocator does not synchronise)
            if kind == "env":
                _, plan, best_cost, best_du, _ = ops.mpc_solve(planner, theta, x_cur, C, c, T, u_init=u0, **args)
            else:
                ws = ops.mpc_solve_unfused(planner, None, x_cur, C, c, T, u_init=u0, u_zero_I=mpc.u_zero_I, **args)
                plan, best_cost, best_du = ws.best_u, ws.best_cost, ws.best_du
            solve_cost[s].copy_(best_cost)
            solve_du[s].copy_(best_du)
            ops.mpc_advance(plant.model_id, theta_plant, plan, x_cur, u_warm, warm_start, x[s + 1], u[s], C, c,
                            stage[s])
            u0 = u_warm
    return Episode(x, u, stage, solve_cost, solve_du)
