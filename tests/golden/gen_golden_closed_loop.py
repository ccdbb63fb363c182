#!/usr/bin/env python3
"""Generate tests/golden/closed_loop_f64.npz and closed_loop_f32.npz from the
reference: closed-loop (receding-horizon) episodes of mpc_explicit.MPC, the
loop of IL_Env.populate_data2 (il_env.py:96-151) written out here so that it
runs batched and with a plant whose parameters differ from the planner's.

TEST INFRASTRUCTURE ONLY, as gen_golden.py: it imports the reference
implementation (read-only; its directory is the first argument or
$DILQR_REFERENCE) with the same recipe (flat imports, no bytecode, an empty
stand-in for casadi) and writes data.  It never runs on a GPU; only the .npz
files travel.

Per step (il_env.py:120-140): solve from x with u_init, apply
nominal_actions[0] to the plant, u_init = cat(nominal_actions[1:], 0) and then
u_init[-2] = u_init[-3].  Every case takes linesearch_decay,
max_linesearch_iter and eps = mpc_eps from the model, the bounds from the model
(rocket: none), exit_unconverged and detach_unconverged False, the true
objective as the cost, repeated over T and the batch.

Cases (CASES below): pendulum and cartpole batched, the literal populate_data2
case at B = 1, a planner with wrong parameters against the true plant, the
smallest horizon the quirk is defined at (T = 3), the 5-parameter pendulum
through GradMethods.AUTO_DIFF (its runnable reference path), the rocket.

Stored per case `k`: k_x0 [B,n], k_x [steps+1,B,n], k_u [steps,B,m],
k_plan_costs [steps,B] (each solve's costs), k_settings (T, steps, lqr_iter,
eps, lower, upper (nan: none), linesearch_decay, max_linesearch_iter),
k_planner_params, k_plant_params; `cases` lists the names and k_model the
model's.  The fp32 file also holds the reference's own fp32-vs-fp64 spread of x
and u (k_spread_x, k_spread_u: max |a32 - a64| / max(1, max |a64|), the tests'
relerr).

Condition, checked here: every stored case has spread_x and spread_u below
1e-4.  A draw that does not gets another seed (the case's seed below); the
bound is not widened.  (The rocket's first seed, 6, gave spread_u 2.1e-4.  The
seeds of pend_b1 and complex were also redrawn, away from episodes whose every
control sits at a bound, which would compare nothing but the clamp.)

Usage:  python tests/golden/gen_golden_closed_loop.py [REFERENCE_DIR]
"""
import contextlib
import io
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DILQR_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
if not REF or not os.path.isdir(REF):
    sys.exit("usage: gen_golden_closed_loop.py REFERENCE_DIR (or set DILQR_REFERENCE)")

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)

if REF not in sys.path:
    sys.path.insert(0, REF)
sys.modules.setdefault("casadi", types.ModuleType("casadi"))
import util  # noqa: E402,F401
import pnqp  # noqa: E402,F401
import mpc as ref_mpc  # noqa: E402,F401  (before lqr_step: the two import each other)
import lqr_step  # noqa: E402,F401
import lqr_step_explicit  # noqa: E402,F401
import mpc_explicit  # noqa: E402
from env_dx import cartpole, pendulum, rocket  # noqa: E402

SPREAD_MAX = 1e-4
MAX_FILE_BYTES = 1 << 20
COMPLEX_PARAMS = (10., 1., 1., 1.0, 0.1)        # il_env.py:41

# name: model, T, steps, lqr_iter, B, seed, planner params (None: the model's own)
CASES = {
    "pend": ("pendulum", 8, 6, 10, 4, 0, None),
    "cart": ("cartpole", 10, 10, 20, 4, 1, None),
    "pend_b1": ("pendulum", 6, 6, 10, 1, 14, None),
    "pend_mismatch": ("pendulum", 8, 6, 10, 4, 3, (15., 3., 0.5)),
    "pend_t3": ("pendulum", 3, 2, 10, 4, 4, None),
    "complex": ("pendulum-complex", 8, 4, 10, 4, 12, None),
    "rocket": ("rocket", 6, 3, 5, 2, 18, None),
}


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


def np_(t):
    return t.detach().cpu().numpy()


def make_model(mname, params, dt):
    p = None if params is None else torch.tensor(params, dtype=dt)
    if mname == "pendulum":
        return pendulum.PendulumDx(p)
    if mname == "pendulum-complex":
        return pendulum.PendulumDx(torch.tensor(COMPLEX_PARAMS, dtype=dt) if p is None else p, simple=False)
    if mname == "cartpole":
        return cartpole.CartpoleDx(p)
    return rocket.RocketDx(p)


def xinit(mname, B, rng):
    if mname.startswith("pendulum"):       # il_env.py:63-66
        th = rng.uniform(-np.pi / 2, np.pi / 2, B)
        return np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, B)], 1)
    if mname == "cartpole":                # near upright: the angle within +-0.3
        th = rng.uniform(-0.3, 0.3, B)
        return np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                         rng.uniform(-1, 1, B)], 1)
    r = rng.uniform([0, -4, -2.5], [10, 4, 2.5], (B, 3))      # rocket near hover
    v = rng.normal(0, 0.1, (B, 3))
    q = np.array([1., 0, 0, 0]) + 0.05 * rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w = rng.normal(0, 0.02, (B, 3))
    return np.concatenate([r, v, q, w], 1)


def episode(name, dt, x0):
    mname, T, steps, lqr_iter, B, _, planner_params = CASES[name]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        planner = make_model(mname, planner_params, dt)
        plant = make_model(mname, None, dt)
        q, p = plant.get_true_obj()
        Q = torch.diag(q).to(dt).unsqueeze(0).unsqueeze(0).repeat(T, B, 1, 1)
        P = p.to(dt).unsqueeze(0).repeat(T, B, 1)
        bounds = {} if mname == "rocket" else dict(u_lower=plant.lower, u_upper=plant.upper)
        gm = mpc_explicit.GradMethods.AUTO_DIFF if mname == "pendulum-complex" else mpc_explicit.GradMethods.ANALYTIC
        x = torch.tensor(x0, dtype=dt)
        u_init = None
        xs, us, costs = [x], [], []
        for _ in range(steps):
            solver = mpc_explicit.MPC(
                plant.n_state, plant.n_ctrl, T, u_init=u_init, lqr_iter=lqr_iter, verbose=-1, n_batch=B,
                exit_unconverged=False, detach_unconverged=False, linesearch_decay=plant.linesearch_decay,
                max_linesearch_iter=plant.max_linesearch_iter, grad_method=gm, eps=plant.mpc_eps, **bounds)
            # AUTO_DIFF differentiates the dynamics with torch.autograd.grad: grad mode stays on
            with contextlib.redirect_stdout(io.StringIO()):
                _, actions, cost = solver(x, mpc_explicit.QuadCost(Q.clone(), P.clone()), planner)
            actions = actions.detach()
            with torch.no_grad():
                x = plant(x, actions[0]).detach()
            us.append(actions[0])
            xs.append(x)
            costs.append(cost.detach())
            u_init = torch.cat((actions[1:], torch.zeros(1, B, plant.n_ctrl)), dim=0)      # il_env.py:139-140
            u_init[-2] = u_init[-3]
        lo, hi = (np.nan, np.nan) if not bounds else (float(plant.lower), float(plant.upper))
        settings = np.array([T, steps, lqr_iter, plant.mpc_eps, lo, hi, plant.linesearch_decay,
                             plant.max_linesearch_iter], np.float64)
        return dict(x=np_(torch.stack(xs)), u=np_(torch.stack(us)), plan_costs=np_(torch.stack(costs)),
                    settings=settings, planner_params=np_(planner.params).astype(np.float64),
                    plant_params=np_(plant.params).astype(np.float64))
    finally:
        torch.set_default_dtype(old)


def main():
    files = {torch.float64: {}, torch.float32: {}}
    for name, (mname, T, steps, lqr_iter, B, seed, _) in CASES.items():
        x0 = xinit(mname, B, np.random.RandomState(seed))
        r64, r32 = episode(name, torch.float64, x0), episode(name, torch.float32, x0)
        spread = {k: relerr(r32[k], r64[k]) for k in ("x", "u", "plan_costs")}
        sat = "" if np.isnan(r64["settings"][4]) else \
            f", {np.mean(np.abs(r64['u']) >= r64['settings'][5] - 1e-9):.0%} of controls at a bound"
        print(f"  {name:14s} spread: " + ", ".join(f"{k} {v:.1e}" for k, v in spread.items()) + sat)
        assert spread["x"] < SPREAD_MAX and spread["u"] < SPREAD_MAX, (
            f"{name}: the reference's own fp32 spread is x {spread['x']:.2e}, u {spread['u']:.2e}; draw another seed")
        for dt, r in ((torch.float64, r64), (torch.float32, r32)):
            npdt = np.float64 if dt == torch.float64 else np.float32
            files[dt][f"{name}_x0"] = x0.astype(npdt)
            files[dt][f"{name}_model"] = np.array(mname)
            files[dt].update({f"{name}_{k}": v for k, v in r.items()})
        files[torch.float32].update({f"{name}_spread_{k}": np.float64(spread[k]) for k in ("x", "u")})
    for dt, out in files.items():
        out["cases"] = np.array(list(CASES))
        path = os.path.join(OUT, f"closed_loop_{'f64' if dt == torch.float64 else 'f32'}.npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(f"  wrote {os.path.basename(path)} ({size / 1024:.1f} KiB)")
        assert size <= MAX_FILE_BYTES, path


if __name__ == "__main__":
    main()
