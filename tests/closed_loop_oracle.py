"""A numpy closed-loop (receding-horizon) MPC episode, restating the loop of
IL_Env.populate_data2 (il_env.py:110-140) batched: oracle.mpc.mpc_forward for
each solve, the oracle.models forward for the plant, and the three warm-start
rules of dilqr_mpc_advance_f32 (include/dilqr.h DILQR_WARM_*).

TEST INFRASTRUCTURE ONLY: tests/test_closed_loop_cpu.py pins it to the fp64
golden (tests/golden/closed_loop_f64.npz); the GPU tests read the goldens."""
import numpy as np

from oracle import models as omodels
from oracle import mpc as ompc

WARM_MODES = ("reference", "shift", "cold")
# the generator's model names -> oracle.models.MODELS
MODEL_NAMES = {"pendulum": "pendulum", "pendulum-complex": "pendulum_complex", "cartpole": "cartpole",
               "rocket": "rocket"}


def warm_start(u, mode):
    """The next solve's u_init from this solve's plan u [T,B,m]."""
    T = u.shape[0]
    if mode == "cold":
        return np.zeros_like(u)
    w = np.concatenate([u[1:], np.zeros_like(u[:1])], 0)          # il_env.py:139
    if mode == "reference":
        if T < 3:
            raise IndexError("the reference's u_init[-3] needs T >= 3")
        w[-2] = w[-3]                                              # il_env.py:140
    elif mode != "shift":
        raise ValueError(mode)
    return w


def stage_cost(x, u, C0, c0):
    """0.5 tau^T C_0 tau + c_0^T tau per problem, tau = [x; u]."""
    tau = np.concatenate([x, u], -1)
    return 0.5 * np.einsum("bi,bij,bj->b", tau, C0, tau) + np.einsum("bi,bi->b", tau, c0)


def episode(model, x0, C, c, T, steps, planner_params=None, plant_params=None, warm="reference", u_init=None,
            **solver):
    """x [steps+1,B,n], u [steps,B,m], stage costs [steps,B], plan costs
    [steps,B]; `solver`: mpc_forward's keywords."""
    x = np.array(x0)
    xs, us, stage, plan_costs = [x], [], [], []
    for _ in range(steps):
        _, plan, costs, _ = ompc.mpc_forward(model, x, C, c, T, u_init=u_init, params=planner_params, **solver)
        stage.append(stage_cost(x, plan[0], C[0], c[0]))
        x = model.forward(x, plan[0], plant_params)
        xs.append(x)
        us.append(plan[0])
        plan_costs.append(costs)
        u_init = warm_start(plan, warm)
    return np.stack(xs), np.stack(us), np.stack(stage), np.stack(plan_costs)


def golden_case(g, name, dtype=np.float64):
    """A stored case's inputs as episode() takes them: (model, x0, C, c, T, steps,
    keywords)."""
    model = omodels.MODELS[MODEL_NAMES[str(g[f"{name}_model"])]]
    T, steps, lqr_iter, eps, lo, hi, decay, max_ls = g[f"{name}_settings"]
    T, steps = int(T), int(steps)
    x0 = g[f"{name}_x0"].astype(dtype)
    q, p = model.true_obj()
    C, c = ompc.expand_cost(np.diag(q).astype(dtype), p.astype(dtype), T, x0.shape[0])
    kw = dict(planner_params=tuple(g[f"{name}_planner_params"]), plant_params=tuple(g[f"{name}_plant_params"]),
              lqr_iter=int(lqr_iter), eps=float(eps), linesearch_decay=float(decay),
              max_linesearch_iter=int(max_ls))
    if not np.isnan(lo):
        kw.update(u_lower=float(lo), u_upper=float(hi))
    return model, x0, C, c, T, steps, kw
