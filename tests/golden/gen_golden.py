#!/usr/bin/env python3
"""Generate the golden input/output vectors under tests/golden/ from the reference.

TEST INFRASTRUCTURE ONLY.  This script imports the reference implementation
(josef-w/Differentiable-iLQR, mounted read-only at /root/reference) in the BUILD
container and writes small .npz fixtures (inputs + the reference's outputs).
It never runs on the GPU box; only the .npz files travel.  Nothing from the
reference is copied: the fixtures are data.

Recipes follow SURVEY.md §8(c):
  * flat imports with PYTHONDONTWRITEBYTECODE (the tree is read-only);
  * rocket.py does `from casadi import *` only for its animation code
    (rocket.py:6, 959, 1006) -> an empty stand-in module named `casadi`;
  * the Riccati sweep is reached through the LQRStepFn.forward closure;
  * the DiLQR implicit backward is driven through LQRStep(no_op_forward=True)
    (backward through mpc_explicit.MPC itself raises under torch 2.10);
  * data/*.pkl are NOT unpickled: their opcode stream is parsed statically
    with pickletools and only the embedded tensor storages are loaded, with
    torch.load(weights_only=True).

Usage:  python tests/golden/gen_golden.py   (takes ~1-2 minutes on 8 cores)
"""
import contextlib
import glob
import io
import os
import pickletools
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)


def _import_reference():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.modules.setdefault("casadi", types.ModuleType("casadi"))
    import util
    import pnqp
    import mpc            # before lqr_step: mpc.py <-> lqr_step.py import each other
    import lqr_step
    import mpc_backup     # likewise for lqr_step_backup.py
    import lqr_step_backup
    import lqr_step_explicit
    import mpc_explicit
    from env_dx import cartpole, pendulum, rocket
    return types.SimpleNamespace(
        util=util, pnqp=pnqp, lqr_step_explicit=lqr_step_explicit, lqr_step_backup=lqr_step_backup,
        lqr_step=lqr_step, mpc_explicit=mpc_explicit, mpc=mpc,
        cartpole=cartpole, pendulum=pendulum, rocket=rocket)


R = _import_reference()


@contextlib.contextmanager
def default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def np_(t):
    if isinstance(t, (list, tuple)):
        return np.stack([np_(x) for x in t])
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().numpy()
    return np.asarray(t)


MAX_FILE_BYTES = 1 << 20       # no fixture file above 1 MiB


def save(name, **arrs):
    """name.npz; a set that compresses to more than MAX_FILE_BYTES is split, in
    key order, into name.npz, name.part1.npz, ... (the tests' `golden` fixture
    loads every part into one dict)."""
    arrs = {k: np.asarray(v) for k, v in arrs.items()}
    for old in glob.glob(os.path.join(OUT, name + ".part*.npz")):
        os.remove(old)
    parts = [list(arrs)]
    while True:
        paths = [os.path.join(OUT, name + (f".part{i}" if i else "") + ".npz") for i in range(len(parts))]
        for path, keys in zip(paths, parts):
            np.savez_compressed(path, **{k: arrs[k] for k in keys})
        big = [i for i, path in enumerate(paths) if os.path.getsize(path) > MAX_FILE_BYTES and len(parts[i]) > 1]
        if not big:
            break
        i = big[0]                  # halve the first oversized part by raw bytes, keeping the key order
        keys = parts[i]
        run = np.cumsum([arrs[k].nbytes for k in keys])
        cut = min(max(int(np.searchsorted(run, run[-1] / 2)), 1), len(keys) - 1)
        parts[i:i + 1] = [keys[:cut], keys[cut:]]
    for path in paths:
        print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)/1024:.1f} KiB)")


def model(name):
    return {"pendulum": R.pendulum.PendulumDx, "cartpole": R.cartpole.CartpoleDx,
            "rocket": R.rocket.RocketDx}[name]()


def tname(dt):
    return "f64" if dt == torch.float64 else "f32"


# --------------------------------------------------------------------------
# random inputs (numpy RandomState so the oracle tests can regenerate them)
# --------------------------------------------------------------------------
def sample_states(name, N, rng, wide=True):
    if name == "pendulum":
        th = rng.uniform(-np.pi, np.pi, N)
        dth = rng.uniform(-8, 8, N)
        x = np.stack([np.cos(th), np.sin(th), dth], 1)
        u = rng.uniform(-3, 3, (N, 1))       # beyond the +-2 clamp
    elif name == "cartpole":
        th = rng.uniform(-np.pi, np.pi, N)
        x = np.stack([rng.uniform(-1, 1, N), rng.uniform(-2, 2, N), np.cos(th), np.sin(th),
                      rng.uniform(-3, 3, N)], 1)
        u = rng.uniform(-150, 150, (N, 1)) if wide else rng.uniform(-5, 5, (N, 1))
    elif name == "rocket":
        r = rng.uniform([0, -4, -2.5], [10, 4, 2.5], (N, 3))
        v = rng.normal(0, 1.0, (N, 3))
        q = np.array([1., 0, 0, 0]) + 0.3 * rng.normal(size=(N, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w = rng.normal(0, 0.5, (N, 3))
        x = np.concatenate([r, v, q, w], 1)
        u = rng.uniform(-30, 30, (N, 3))
    return x, u


def random_lqr(n, m, T, B, rng):
    """SURVEY.md §8(d) Riccati workload: C=LL^T+0.1I, c~N, F=[I+0.05N | 0.1N]."""
    d = n + m
    L = rng.normal(size=(T, B, d, d)) * 0.5 / np.sqrt(d)
    C = L @ np.swapaxes(L, -1, -2) + 0.1 * np.eye(d)
    c = rng.normal(size=(T, B, d))
    F = np.concatenate([np.eye(n) + 0.05 * rng.normal(size=(T - 1, B, n, n)),
                        0.1 * rng.normal(size=(T - 1, B, n, m))], -1)
    f = 0.1 * rng.normal(size=(T - 1, B, n))
    return C, c, F, f


def riccati_closure(step_mod, n, m, T, **kw):
    fn = step_mod.LQRStep(n, m, T, **kw).__self__.forward
    cells = dict(zip(fn.__code__.co_freevars, [c.cell_contents for c in fn.__closure__]))
    return cells["lqr_backward"]


# --------------------------------------------------------------------------
# A. dynamics models: forward, get_linear_dyn, get_matrices, grad_input
# --------------------------------------------------------------------------
def case_models():
    print("A. models")
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            for name in ("pendulum", "cartpole", "rocket"):
                rng = np.random.RandomState(100)
                N = 64
                x, u = sample_states(name, N, rng)
                dx = model(name)
                X, U = torch.tensor(x, dtype=dt), torch.tensor(u, dtype=dt)
                with torch.no_grad():
                    out[f"{name}_x"] = x
                    out[f"{name}_u"] = u
                    out[f"{name}_fwd"] = np_(dx(X, U))
                    out[f"{name}_D"] = np_(dx.get_linear_dyn(X, U))
                    Ns = 16
                    mats = dx.get_matrices(X[:Ns], U[:Ns])
                    for k, v in zip(("D", "D_params", "D_x", "D_u", "x_theta", "x_xtm1", "x_utm1"), mats):
                        out[f"{name}_gm_{k}"] = np_(v)
                    # grad_input over a short random closed-loop trajectory
                    T, B = 6, 3
                    rng2 = np.random.RandomState(7)
                    xs, us = sample_states(name, T * B, rng2, wide=False)
                    Xs = torch.tensor(xs.reshape(T, B, -1), dtype=dt)
                    Us = torch.tensor(us.reshape(T, B, -1), dtype=dt)
                    K = torch.tensor(rng2.normal(size=(T, B, dx.n_ctrl, dx.n_state)) * 0.3, dtype=dt)
                    gi = dx.grad_input(Xs, Us, K)
                    out[f"{name}_gi_X"], out[f"{name}_gi_U"], out[f"{name}_gi_K"] = np_(Xs), np_(Us), np_(K)
                    for k, v in zip(("grad_D", "grad_d", "D_x", "D_u", "D", "d_x", "d_u"), gi):
                        out[f"{name}_gi_{k}"] = np_(v)
            save(f"models_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# B. Riccati sweep (lqr_backward) unconstrained / bounded / Cholesky variant
# --------------------------------------------------------------------------
def case_riccati():
    print("B. riccati")
    shapes = {"pendulum": (3, 1, 10, 16), "cartpole": (5, 1, 25, 16), "rocket": (13, 3, 30, 8)}
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            for name, (n, m, T, B) in shapes.items():
                rng = np.random.RandomState(0)
                C, c, F, _ = random_lqr(n, m, T, B, rng)
                u = rng.uniform(-0.5, 0.5, (T, B, m))
                Ct, ct, Ft, ut = (torch.tensor(a, dtype=dt) for a in (C, c, F, u))
                out[f"{name}_C"], out[f"{name}_c"], out[f"{name}_F"], out[f"{name}_u"] = C, c, F, u
                ctx = types.SimpleNamespace(current_u=ut)
                with torch.no_grad():
                    lb = riccati_closure(R.lqr_step_explicit, n, m, T)
                    Ks, ks, _ = lb(ctx, Ct, ct, Ft, None)
                    out[f"{name}_K"], out[f"{name}_k"] = np_(Ks[::-1]), np_(ks[::-1])
                    lo, hi = -1.0, 1.0
                    lb = riccati_closure(R.lqr_step_explicit, n, m, T, u_lower=lo, u_upper=hi)
                    Ks, ks, nqp = lb(ctx, Ct, ct, Ft, None)
                    out[f"{name}_box_K"], out[f"{name}_box_k"] = np_(Ks[::-1]), np_(ks[::-1])
                    out[f"{name}_box_nqp"] = np.array(nqp)
                    # adjoint engine (lqr_step_backup: Cholesky + 1e-6 I for m>1)
                    lb = riccati_closure(R.lqr_step_backup, n, m, T)
                    Ks, ks, _ = lb(ctx, Ct, ct, Ft, None)
                    out[f"{name}_chol_K"], out[f"{name}_chol_k"] = np_(Ks[::-1]), np_(ks[::-1])
                    # u_zero_I branch (active-set masked solve used by the adjoints)
                    I = torch.tensor(rng.uniform(size=(T, B, m)) < 0.3)
                    lb = riccati_closure(R.lqr_step_backup, n, m, T, u_zero_I=I)
                    Ks, ks, _ = lb(ctx, Ct, ct, Ft, None)
                    out[f"{name}_zI"] = np_(I)
                    out[f"{name}_zI_K"], out[f"{name}_zI_k"] = np_(Ks[::-1]), np_(ks[::-1])
            save(f"riccati_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# C. pnqp box QP
# --------------------------------------------------------------------------
def case_pnqp():
    print("C. pnqp")
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            for m in (1, 3):
                rng = np.random.RandomState(3 + m)
                B = 64
                L = rng.normal(size=(B, m, m))
                H = L @ np.swapaxes(L, 1, 2) + 0.2 * np.eye(m)
                q = rng.normal(size=(B, m)) * 3
                lo = -rng.uniform(0.1, 1.5, (B, m))
                hi = rng.uniform(0.1, 1.5, (B, m))
                x0 = rng.uniform(-2, 2, (B, m))
                Ht, qt, lot, hit, x0t = (torch.tensor(a, dtype=dt) for a in (H, q, lo, hi, x0))
                out.update({f"m{m}_H": H, f"m{m}_q": q, f"m{m}_lo": lo, f"m{m}_hi": hi, f"m{m}_x0": x0})
                with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                    x, _, If, it = R.pnqp.pnqp(Ht, qt, lot, hit)
                    out[f"m{m}_x"], out[f"m{m}_If"], out[f"m{m}_it"] = np_(x), np_(If), np.array(it)
                    x, _, If, it = R.pnqp.pnqp(Ht, qt, -0.7, 0.7, x_init=x0t)
                    out[f"m{m}_xf"], out[f"m{m}_Iff"], out[f"m{m}_itf"] = np_(x), np_(If), np.array(it)
                    # per-problem calls (batch size 1): the reference semantics without batch coupling
                    xs, its = [], []
                    for b in range(B):
                        x, _, If, it = R.pnqp.pnqp(Ht[b:b+1], qt[b:b+1], lot[b:b+1], hit[b:b+1])
                        xs.append(np_(x)[0]); its.append(it)
                    out[f"m{m}_x_pp"], out[f"m{m}_it_pp"] = np.stack(xs), np.array(its)
            save(f"pnqp_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# helpers for the solver-level cases
# --------------------------------------------------------------------------
def xinit_for(name, B, rng):
    if name == "pendulum":       # il_env.py:63-66
        th = rng.uniform(-np.pi / 2, np.pi / 2, B)
        return np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, B)], 1)
    if name == "cartpole":       # il_env.py:71-75 without the *0
        th = rng.uniform(-np.pi, np.pi, B)
        return np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                         rng.uniform(-1, 1, B)], 1)
    if name == "rocket":         # near hover
        r = rng.uniform([0, -4, -2.5], [10, 4, 2.5], (B, 3))
        v = rng.normal(0, 0.1, (B, 3))
        q = np.array([1., 0, 0, 0]) + 0.05 * rng.normal(size=(B, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w = rng.normal(0, 0.02, (B, 3))
        return np.concatenate([r, v, q, w], 1)


def true_cost(dx, T, B, dt):
    q, p = dx.get_true_obj()       # il_env.py:159-162 materialisation
    Q = torch.diag(q).to(dt).unsqueeze(0).unsqueeze(0).repeat(T, B, 1, 1)
    P = p.to(dt).unsqueeze(0).repeat(T, B, 1)
    return Q, P


# --------------------------------------------------------------------------
# D. one LQRStep (explicit) forward: Riccati + rollout/line search
# --------------------------------------------------------------------------
def case_lqrstep():
    print("D. lqr step")
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            for tag, bounds in (("unc", None), ("box", (-5.0, 5.0))):
                dx = model("cartpole")
                T, B = 25, 16
                rng = np.random.RandomState(11)
                x0 = xinit_for("cartpole", B, rng)
                u = rng.uniform(-2, 2, (T, B, 1))
                X0, U = torch.tensor(x0, dtype=dt), torch.tensor(u, dtype=dt)
                Q, P = true_cost(dx, T, B, dt)
                mpc_ = R.mpc_explicit.MPC(5, 1, T, lqr_iter=1)
                with torch.no_grad():
                    X = R.util.get_traj(T, U, x_init=X0, dynamics=dx)
                    F, f = mpc_.linearize_dynamics(X, U, dx, diff=False)
                    kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
                    step = R.lqr_step_explicit.LQRStep(
                        5, 1, T, true_cost=R.mpc_explicit.QuadCost(Q, P), true_dynamics=dx,
                        current_x=X, current_u=U, linesearch_decay=0.5, max_linesearch_iter=2, **kw)
                    nx, nu, nqp, costs, du, malpha = step(X0, Q, P, F, f, None)
                out.update({f"{tag}_x0": x0, f"{tag}_u": u, f"{tag}_x": np_(X), f"{tag}_F": np_(F),
                            f"{tag}_f": np_(f), f"{tag}_nx": np_(nx), f"{tag}_nu": np_(nu),
                            f"{tag}_costs": np_(costs), f"{tag}_du": np_(du), f"{tag}_malpha": np_(malpha),
                            f"{tag}_nqp": np_(nqp)})
            save(f"lqrstep_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# E. full MPC (mpc_explicit) solves
# --------------------------------------------------------------------------
MPC_CASES = {
    # name: (model, T, B, lqr_iter, bounds, eps, not_improved_lim, decay, max_ls)
    "cart_unc": ("cartpole", 25, 64, 10, None, 0.0, 10 ** 9, 0.5, 2),
    "cart_box10": ("cartpole", 25, 64, 10, (-10.0, 10.0), 0.0, 10 ** 9, 0.5, 2),
    "cart_il": ("cartpole", 25, 64, 40, (-100.0, 100.0), 1e-4, 5, 0.5, 2),
    "pend_unc": ("pendulum", 10, 64, 10, None, 0.0, 10 ** 9, 0.2, 5),
    "pend_box": ("pendulum", 10, 64, 10, (-2.0, 2.0), 0.0, 10 ** 9, 0.2, 5),
    "rocket_unc": ("rocket", 30, 64, 5, None, 0.0, 10 ** 9, 0.2, 5),
}


def run_mpc(name, dt, lqr_iter_override=None):
    mname, T, B, it, bounds, eps, nil, decay, mls = MPC_CASES[name]
    dx = model(mname)
    rng = np.random.RandomState(0)
    x0 = xinit_for(mname, B, rng)
    X0 = torch.tensor(x0, dtype=dt)
    Q, P = true_cost(dx, T, B, dt)
    kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
    m = R.mpc_explicit.MPC(dx.n_state, dx.n_ctrl, T, lqr_iter=lqr_iter_override or it, eps=eps,
                           not_improved_lim=nil, linesearch_decay=decay, max_linesearch_iter=mls,
                           exit_unconverged=False, detach_unconverged=False, verbose=-1,
                           grad_method=R.mpc_explicit.GradMethods.ANALYTIC, **kw)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        x, u, costs = m(X0, R.mpc_explicit.QuadCost(Q, P), dx)
    return x0, np_(x), np_(u), np_(costs)


MPC_ITERATE_CASES = ("cart_unc", "cart_box10", "pend_box")   # per-iteration goldens (lqr_iter 1, 2, 3)


def case_mpc_iterates():
    """Only the per-iteration entries of MPC_ITERATE_CASES, merged into the
    existing mpc_{f64,f32}.npz (the rest of those files is left as it is)."""
    print("E'. mpc per-iteration entries")
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            for path in [os.path.join(OUT, f"mpc_{tname(dt)}.npz")] + sorted(
                    glob.glob(os.path.join(OUT, f"mpc_{tname(dt)}.part*.npz"))):
                with np.load(path) as old:
                    out.update({k: old[k] for k in old.files})
            for name in MPC_ITERATE_CASES:
                for k in (1, 2, 3):
                    _, x, u, costs = run_mpc(name, dt, lqr_iter_override=k)
                    out.update({f"{name}_it{k}_x": x, f"{name}_it{k}_u": u, f"{name}_it{k}_costs": costs})
            save(f"mpc_{tname(dt)}", **out)


def case_mpc():
    print("E. mpc")
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            for name in MPC_CASES:
                x0, x, u, costs = run_mpc(name, dt)
                out.update({f"{name}_x0": x0, f"{name}_x": x, f"{name}_u": u, f"{name}_costs": costs})
                if name in MPC_ITERATE_CASES:
                    for k in (1, 2, 3):
                        _, x, u, costs = run_mpc(name, dt, lqr_iter_override=k)
                        out.update({f"{name}_it{k}_x": x, f"{name}_it{k}_u": u, f"{name}_it{k}_costs": costs})
            save(f"mpc_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# F. classic differentiable LQR (mpc.py + lqr_step.py backward)
# --------------------------------------------------------------------------
def case_classic_adjoint():
    print("F. classic adjoint")
    dt = torch.float64
    with default_dtype(dt):
        out = {}
        for tag, (n, m, T, B, bounds) in {"m1": (5, 1, 10, 3, None), "m3": (4, 3, 8, 3, None),
                                            "m1box": (5, 1, 10, 3, (-0.5, 0.5)),
                                            "m3box": (4, 3, 8, 3, (-0.5, 0.5))}.items():
            rng = np.random.RandomState(21)
            C, c, F, f = random_lqr(n, m, T, B, rng)
            x0 = rng.normal(size=(B, n))
            wx, wu = rng.normal(size=(T, B, n)), rng.normal(size=(T, B, m))
            Ct, ct, Ft, ft, x0t = (torch.tensor(a, dtype=dt, requires_grad=True) for a in (C, c, F, f, x0))
            kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
            mpc_ = R.mpc.MPC(n, m, T, lqr_iter=1, n_batch=B, detach_unconverged=False,
                             exit_unconverged=False, verbose=-1, **kw)
            with contextlib.redirect_stdout(io.StringIO()):
                x, u, _ = mpc_(x0t, R.mpc.QuadCost(Ct, ct), R.mpc.LinDx(Ft, ft))
                loss = (x * torch.tensor(wx)).sum() + (u * torch.tensor(wu)).sum()
                loss.backward()
            out.update({f"{tag}_C": C, f"{tag}_c": c, f"{tag}_F": F, f"{tag}_f": f, f"{tag}_x0": x0,
                        f"{tag}_wx": wx, f"{tag}_wu": wu, f"{tag}_x": np_(x), f"{tag}_u": np_(u),
                        f"{tag}_dx0": np_(x0t.grad), f"{tag}_dC": np_(Ct.grad), f"{tag}_dc": np_(ct.grad),
                        f"{tag}_dF": np_(Ft.grad), f"{tag}_df": np_(ft.grad)})
        save("adjoint_f64", **out)


# --------------------------------------------------------------------------
# G. DiLQR implicit backward (lqr_step_explicit.py:653-712)
# --------------------------------------------------------------------------
def implicit_once(mname, T, B, bounds, x, u, x0, Q, P, wx, wu, dt):
    dx = model(mname)
    theta = dx.params.detach().clone().to(dt).requires_grad_(True)
    Qg, Pg = Q.clone().requires_grad_(True), P.clone().requires_grad_(True)
    m = R.mpc_explicit.MPC(dx.n_state, dx.n_ctrl, T, grad_method=R.mpc_explicit.GradMethods.ANALYTIC)
    X, U = torch.tensor(x, dtype=dt), torch.tensor(u, dtype=dt)
    F, f = m.linearize_dynamics(X, U, dx, diff=True)
    F, f = F.detach(), f.detach()
    kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
    step = R.lqr_step_explicit.LQRStep(
        dx.n_state, dx.n_ctrl, T, true_cost=R.mpc_explicit.QuadCost(Qg, Pg), true_dynamics=dx,
        current_x=X, current_u=U, back_eps=m.back_eps, no_op_forward=True, **kw)
    with contextlib.redirect_stdout(io.StringIO()):
        x2, u2 = step(torch.tensor(x0, dtype=dt), Qg, Pg, F, f, theta)
        loss = (x2 * torch.tensor(wx, dtype=dt)).sum() + (u2 * torch.tensor(wu, dtype=dt)).sum()
        loss.backward()
    return np_(Qg.grad), np_(Pg.grad), np_(theta.grad), np_(F), np_(f)


IMPLICIT_CASES = {
    # tag: (model, T, B, bounds, MPC_CASES entry for decay / max_ls)
    "cart_unc": ("cartpole", 10, 4, None, "cart_unc"),
    "cart_box": ("cartpole", 10, 4, (-5.0, 5.0), "cart_box10"),
    "pend_box": ("pendulum", 10, 4, (-2.0, 2.0), "pend_box"),
    # rocket: the reference's D_x/D_u/D_params/x_xtm1 builders (rocket.py:541-820)
    "rock_unc": ("rocket", 10, 4, None, "rocket_unc"),
    "rock_box": ("rocket", 10, 4, (-10.0, 10.0), "rocket_unc"),
}
# config 4's own horizon (SURVEY.md §8(c) case G): cartpole T=25, B=8; T*B=200
# stays under the reference's CPU-path threshold (lqr_step_explicit.py:699-700)
IMPLICIT25_CASES = {
    "cart25_unc": ("cartpole", 25, 8, None, "cart_unc"),
    "cart25_box10": ("cartpole", 25, 8, (-10.0, 10.0), "cart_box10"),
    "cart25_box100": ("cartpole", 25, 8, (-100.0, 100.0), "cart_box10"),
}


def case_implicit25():
    case_implicit(IMPLICIT25_CASES, "implicit25")


def case_implicit(cases=IMPLICIT_CASES, fname="implicit"):
    print(f"G. implicit backward ({fname})")
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            for tag, (mname, T, B, bounds, mpc_case) in cases.items():
                dx = model(mname)
                rng = np.random.RandomState(5)
                x0 = xinit_for(mname, B, rng)
                Q, P = true_cost(dx, T, B, dt)
                kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
                _, _, _, _, _, _, _, decay, mls = MPC_CASES[mpc_case]
                m = R.mpc_explicit.MPC(dx.n_state, dx.n_ctrl, T, lqr_iter=30, eps=1e-6,
                                       linesearch_decay=decay, max_linesearch_iter=mls,
                                       exit_unconverged=False, detach_unconverged=False, verbose=-1,
                                       grad_method=R.mpc_explicit.GradMethods.ANALYTIC, **kw)
                with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                    x, u, _ = m(torch.tensor(x0, dtype=dt), R.mpc_explicit.QuadCost(Q, P), dx)
                x, u = np_(x), np_(u)
                wx = rng.normal(size=x.shape)
                wu = rng.normal(size=u.shape)
                # MKL's batched getrf hangs on the rocket's 160x160 KKT systems with
                # 8 threads in this image (lqr_step_explicit.py:570); one thread is fine
                torch.set_num_threads(1 if mname == "rocket" or T * (dx.n_state + dx.n_ctrl) > 100 else 8)
                dQ, dP, dth, F, f = implicit_once(mname, T, B, bounds, x, u, x0, Q, P, wx, wu, dt)
                # per-problem d theta: weight only problem j
                dth_b = []
                for j in range(B):
                    mx, mu = np.zeros_like(wx), np.zeros_like(wu)
                    mx[:, j], mu[:, j] = wx[:, j], wu[:, j]
                    dth_b.append(implicit_once(mname, T, B, bounds, x, u, x0, Q, P, mx, mu, dt)[2])
                out.update({f"{tag}_x0": x0, f"{tag}_x": x, f"{tag}_u": u, f"{tag}_Q": np_(Q),
                            f"{tag}_P": np_(P), f"{tag}_wx": wx, f"{tag}_wu": wu, f"{tag}_F": F,
                            f"{tag}_f": f, f"{tag}_dQ": dQ, f"{tag}_dP": dP, f"{tag}_dtheta": dth,
                            f"{tag}_dtheta_b": np.stack(dth_b)})
            save(f"{fname}_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# H. the reference's own known-answer datasets (data/*.pkl), parsed statically
# --------------------------------------------------------------------------
def parse_dataset(path):
    data = open(path, "rb").read()
    ops = list(pickletools.genops(data))
    scalars, tensors = {}, {}
    last_key = None
    for i, (op, arg, _pos) in enumerate(ops):
        if op.name in ("SHORT_BINUNICODE", "BINUNICODE") and isinstance(arg, str):
            last_key = arg
        elif op.name in ("BININT1", "BININT2", "BININT", "BINFLOAT") and last_key is not None:
            scalars.setdefault(last_key, arg)
            last_key = None
        elif op.name == "BINBYTES":
            storage = torch.load(io.BytesIO(arg), weights_only=True)
            flat = torch.tensor(storage.tolist(), dtype=storage.dtype)
            # following ops: offset, size tuple, stride tuple (torch._utils._rebuild_tensor_v2)
            ints = []
            for op2, arg2, _ in ops[i + 1:i + 40]:
                if op2.name in ("BININT1", "BININT2", "BININT"):
                    ints.append(arg2)
                if op2.name in ("NEWTRUE", "NEWFALSE"):
                    break
            off, rest = ints[0], ints[1:]
            nd = len(rest) // 2
            size, stride = rest[:nd], rest[nd:]
            owner = [k for k in ("params", "goal_state", "goal_weights", "train_data", "val_data",
                                 "test_data") if k not in tensors][0]
            tensors[owner] = torch.as_strided(flat, size, stride, off).clone().numpy()
    return scalars, tensors


def case_datasets():
    print("H. datasets")
    out = {}
    for env in ("cartpole", "pendulum"):
        scalars, tensors = parse_dataset(os.path.join(REF, "data", env + ".pkl"))
        for k in ("train_data", "val_data", "test_data", "params"):
            out[f"{env}_{k}"] = tensors[k]
        for k in ("lqr_iter", "mpc_T", "linesearch_decay", "max_linesearch_iter", "mpc_eps", "lower", "upper"):
            out[f"{env}_{k}"] = np.array(scalars[k])
    save("datasets", **out)


# --------------------------------------------------------------------------
# I. the IL training loop (il_exp.py:183-429) on a reference dataset
# --------------------------------------------------------------------------
IL_CASES = {
    # name: (dataset, mode, learn_cost, learn_dx, n_train, n_batch, n_epoch, lqr_iter)
    "pend_sysid": ("pendulum", "sysid", False, True, 10, 5, 3, None),
    "pend_empc_dx": ("pendulum", "empc", False, True, 10, 5, 2, 30),
    "pend_empc_cost": ("pendulum", "empc", True, False, 10, 5, 2, 30),
    # the north-star model's dataset (data/cartpole.pkl: 2 train / 1 val / 1 test
    # trajectories, T=35, lqr_iter 100 from the dataset): n_batch 2 (the reference
    # prints matrix_rank(A[1]), lqr_step_explicit.py:561, so a batch needs 2), 4 epochs
    "cart_empc_dx": ("cartpole", "empc", False, True, 2, 2, 4, None),
}


def case_il():
    """IL_Exp(...).run() with its dataset handed over WITHOUT unpickling: the
    IL_Env is rebuilt from the statically parsed dataset and il_exp's `pkl.load`
    is pointed at it (pkl.dump of the best model is a no-op).  setproctitle and
    IPython (absent here) are stand-in modules used only by il_exp's process
    title and excepthook.  The losses/parameter histories come from the CSV
    files run() writes."""
    print("I. il loop")
    import csv
    import shutil
    import tempfile
    st = types.ModuleType("setproctitle")
    st.setproctitle = lambda *a, **k: None
    sys.modules.setdefault("setproctitle", st)
    ip, ipc, ub = types.ModuleType("IPython"), types.ModuleType("IPython.core"), types.ModuleType("IPython.core.ultratb")
    ub.FormattedTB = lambda *a, **k: sys.excepthook
    ip.core, ipc.ultratb = ipc, ub
    for k, v in (("IPython", ip), ("IPython.core", ipc), ("IPython.core.ultratb", ub)):
        sys.modules.setdefault(k, v)
    import il_env
    import il_exp
    out = {}
    for name, (ds, mode, lc, ldx, n_train, n_batch, n_epoch, lqr_iter) in IL_CASES.items():
        scalars, tensors = parse_dataset(os.path.join(REF, "data", ds + ".pkl"))
        env = il_env.IL_Env(ds, lqr_iter=lqr_iter or int(scalars["lqr_iter"]), mpc_T=int(scalars["mpc_T"]))
        for k in ("train_data", "val_data", "test_data"):
            setattr(env, k, torch.tensor(tensors[k], dtype=torch.float32))
        il_exp.pkl = types.SimpleNamespace(load=lambda f, _e=env: _e, dump=lambda *a, **k: None)
        # MKL's multi-threaded getrf/laswp fails on the >100-wide KKT systems
        # (T=35, d=6 -> 210) in this image (see case_implicit); one thread is fine
        torch.set_num_threads(1 if ds == "cartpole" else 8)
        work = tempfile.mkdtemp()
        lin = R.mpc_explicit.MPC.linearize_dynamics
        if mode == "empc":
            # SURVEY.md §8(c) implicit-backward recipe inside the reference's own
            # MPC: the closing linearisation (mpc_explicit.py:302-310) gets the
            # best iterate detached.  The reference makes x, u fresh leaves
            # (.detach().requires_grad_(True)) whose views get_linear_dyn then
            # writes through, which torch 2.10 refuses at backward ("leaf
            # variable has been moved into the graph interior"); those leaves'
            # gradients are consumed by nothing, so detaching them changes no
            # gradient that reaches the parameters (F is built from
            # params.detach(), f = dynamics(x, u) - F tau keeps the params graph,
            # and the no-op LQRStep gets theta = dx.params, 325).
            def lin_detached(self, x, u, dynamics, diff, _lin=lin):
                return _lin(self, x.detach() if diff else x, u.detach() if diff else u, dynamics, diff)
            R.mpc_explicit.MPC.linearize_dynamics = lin_detached
        try:
            exp = il_exp.IL_Exp(data=os.path.join(REF, "data", ds + ".pkl"), work=work, save=os.path.join(work, "s"),
                                n_batch=n_batch, mode=mode, learn_cost=lc, learn_dx=ldx, no_cuda=True, seed=5,
                                n_epoch=n_epoch, n_train=n_train, device="cpu")
            with contextlib.redirect_stdout(io.StringIO()):
                exp.run()
            rd = lambda f: np.array([[float(v) for v in row] for row in list(csv.reader(open(os.path.join(exp.save, f))))[1:]])
            out[f"{name}_train"] = rd("train_losses.csv")
            out[f"{name}_val_test"] = rd("val_test_losses.csv")
            if ldx:
                out[f"{name}_dx_hist"] = np.array([[float(v) for v in row] for row in csv.reader(open(os.path.join(exp.save, "dx_hist.csv")))])
            if lc:
                out[f"{name}_cost_hist"] = np.array([[float(v) for v in row] for row in csv.reader(open(os.path.join(exp.save, "cost_hist.csv")))])
            print(f"  {name}: ok")
        except Exception as e:          # the reference's own failure is recorded, not hidden
            print(f"  {name}: reference raised {type(e).__name__}: {e}")
            out[f"{name}_error"] = np.array(f"{type(e).__name__}: {e}")
        finally:
            R.mpc_explicit.MPC.linearize_dynamics = lin
            shutil.rmtree(work, ignore_errors=True)
    save("il", **out)


# --------------------------------------------------------------------------
# J. generic dynamics / costs: NNDynamics with
#    AUTO_DIFF / FINITE_DIFF / ANALYTIC (grad_input) linearisation through the
#    classic mpc.MPC (+ its backward into the network), an env_dx model with
#    AUTO_DIFF through mpc_explicit, a non-quadratic cost (approximate_cost),
#    and the slew-rate augmentation.  fp64 and fp32.
# --------------------------------------------------------------------------
class NQCost(torch.nn.Module):
    """A smooth non-quadratic stage cost: 1/2|tau|^2 + 0.1 sum tau^4 + w . tau."""

    def __init__(self, w):
        super().__init__()
        self.w = w

    def forward(self, tau):
        return 0.5 * (tau ** 2).sum(-1) + 0.1 * (tau ** 4).sum(-1) + (tau * self.w).sum(-1)


def case_generic():
    print("J. generic dynamics / costs")
    for dt in (torch.float64, torch.float32):
        generic_one(dt)


def generic_one(dt):
    import dynamics as ref_dyn
    out = {}
    with default_dtype(dt), contextlib.redirect_stdout(io.StringIO()):
        T, B = 10, 8
        rng = np.random.RandomState(21)
        # ---- NNDynamics (n=5, m=1, one hidden layer of 32 sigmoids), classic MPC
        torch.manual_seed(3)
        nn_dx = ref_dyn.NNDynamics(5, 1, hidden_sizes=[32], activation="sigmoid")
        for i, fc in enumerate(nn_dx.fcs):
            out[f"nn_W{i}"], out[f"nn_b{i}"] = np_(fc.weight), np_(fc.bias)
        x0 = 0.3 * rng.normal(size=(B, 5))
        L = rng.normal(size=(T, B, 6, 6)) * 0.3
        C = L @ np.swapaxes(L, -1, -2) + np.eye(6)
        c = 0.1 * rng.normal(size=(T, B, 6))
        wx, wu = rng.normal(size=(T, B, 5)), rng.normal(size=(T, B, 1))
        out.update(nn_x0=x0, nn_C=C, nn_c=c, nn_wx=wx, nn_wu=wu)
        for tag, gm in (("auto", R.mpc.GradMethods.AUTO_DIFF), ("fd", R.mpc.GradMethods.FINITE_DIFF),
                        ("analytic", R.mpc.GradMethods.ANALYTIC)):
            for p_ in nn_dx.parameters():
                p_.grad = None
            X0 = torch.tensor(x0, dtype=dt, requires_grad=True)
            Ct, ct = torch.tensor(C, dtype=dt, requires_grad=True), torch.tensor(c, dtype=dt, requires_grad=True)
            m = R.mpc.MPC(5, 1, T, lqr_iter=4, grad_method=gm, u_lower=-1.0, u_upper=1.0, n_batch=B,
                          exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2,
                          max_linesearch_iter=10)
            x, u, costs = m(X0, R.mpc.QuadCost(Ct, ct), nn_dx)
            ((x * torch.tensor(wx, dtype=dt)).sum() + (u * torch.tensor(wu, dtype=dt)).sum()).backward()
            out.update({f"nn_{tag}_x": np_(x), f"nn_{tag}_u": np_(u), f"nn_{tag}_costs": np_(costs),
                        f"nn_{tag}_dx0": np_(X0.grad), f"nn_{tag}_dC": np_(Ct.grad), f"nn_{tag}_dc": np_(ct.grad)})
            for i, fc in enumerate(nn_dx.fcs):
                out[f"nn_{tag}_dW{i}"] = np_(fc.weight.grad)
                out[f"nn_{tag}_db{i}"] = np_(fc.bias.grad)
        # ---- cartpole through mpc_explicit with AUTO_DIFF (forward)
        dx = model("cartpole")
        x0c = xinit_for("cartpole", B, rng)
        Q, P = true_cost(dx, T, B, dt)
        m = R.mpc_explicit.MPC(5, 1, T, lqr_iter=5, grad_method=R.mpc_explicit.GradMethods.AUTO_DIFF,
                               exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.5,
                               max_linesearch_iter=2, eps=0.0, not_improved_lim=10 ** 9)
        x, u, costs = m(torch.tensor(x0c, dtype=dt), R.mpc_explicit.QuadCost(Q, P), dx)
        out.update(cart_auto_x0=x0c, cart_auto_x=np_(x), cart_auto_u=np_(u), cart_auto_costs=np_(costs))
        # ---- cartpole with a slew-rate penalty: mpc_explicit ANALYTIC and mpc AUTO_DIFF (forward)
        for tag, mod, gm in (("slew_explicit", R.mpc_explicit, R.mpc_explicit.GradMethods.ANALYTIC),
                             ("slew_classic", R.mpc, R.mpc.GradMethods.AUTO_DIFF)):
            m = mod.MPC(5, 1, T, lqr_iter=5, grad_method=gm, slew_rate_penalty=0.1, exit_unconverged=False,
                        detach_unconverged=False, linesearch_decay=0.5, max_linesearch_iter=2, eps=0.0,
                        not_improved_lim=10 ** 9)
            x, u, costs = m(torch.tensor(x0c, dtype=dt), mod.QuadCost(Q, P), dx)
            out.update({f"{tag}_x": np_(x), f"{tag}_u": np_(u), f"{tag}_costs": np_(costs)})
        # ---- cartpole with the delta_u trust region (lqr_step_explicit.py:205-213)
        m = R.mpc_explicit.MPC(5, 1, T, lqr_iter=5, grad_method=R.mpc_explicit.GradMethods.ANALYTIC,
                               u_lower=-10.0, u_upper=10.0, delta_u=1.0, exit_unconverged=False,
                               detach_unconverged=False, linesearch_decay=0.5, max_linesearch_iter=2, eps=0.0,
                               not_improved_lim=10 ** 9)
        x, u, costs = m(torch.tensor(x0c, dtype=dt), R.mpc_explicit.QuadCost(Q, P), dx)
        out.update(delta_u_x=np_(x), delta_u_u=np_(u), delta_u_costs=np_(costs))
        # ---- pendulum with a non-quadratic cost: mpc AUTO_DIFF and mpc_explicit ANALYTIC (forward)
        dxp = model("pendulum")
        x0p = xinit_for("pendulum", B, rng)
        wq = 0.3 * rng.normal(size=4)
        out.update(nq_x0=x0p, nq_w=wq)
        for tag, mod, gm in (("nq_classic", R.mpc, R.mpc.GradMethods.AUTO_DIFF),
                             ("nq_explicit", R.mpc_explicit, R.mpc_explicit.GradMethods.ANALYTIC)):
            m = mod.MPC(3, 1, T, lqr_iter=5, grad_method=gm, n_batch=B, exit_unconverged=False,
                        detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=5, eps=0.0,
                        not_improved_lim=10 ** 9, u_lower=-2.0, u_upper=2.0)
            x, u, costs = m(torch.tensor(x0p, dtype=dt), NQCost(torch.tensor(wq, dtype=dt)), dxp)
            out.update({f"{tag}_x": np_(x), f"{tag}_u": np_(u), f"{tag}_costs": np_(costs)})
    save(f"generic_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# K. API options: delta_u on LQRStep, u_zero_I on both MPCs and the implicit step
# --------------------------------------------------------------------------
def case_api():
    print("K. api options")
    for dt in (torch.float64, torch.float32):
        out = {}
        with default_dtype(dt), contextlib.redirect_stdout(io.StringIO()):
            # ---- LQRStep(delta_u) (lqr_step_explicit.py:132-135, 205-213), the lqrstep 'box' setup
            dx = model("cartpole")
            T, B = 25, 16
            rng = np.random.RandomState(11)
            x0 = xinit_for("cartpole", B, rng)
            u = rng.uniform(-2, 2, (T, B, 1))
            X0, U = torch.tensor(x0, dtype=dt), torch.tensor(u, dtype=dt)
            Q, P = true_cost(dx, T, B, dt)
            mpc_ = R.mpc_explicit.MPC(5, 1, T, lqr_iter=1)
            with torch.no_grad():
                X = R.util.get_traj(T, U, x_init=X0, dynamics=dx)
                F, f = mpc_.linearize_dynamics(X, U, dx, diff=False)
                step = R.lqr_step_explicit.LQRStep(
                    5, 1, T, u_lower=-5.0, u_upper=5.0, delta_u=0.5, true_cost=R.mpc_explicit.QuadCost(Q, P),
                    true_dynamics=dx, current_x=X, current_u=U, linesearch_decay=0.5, max_linesearch_iter=2)
                nx, nu, nqp, costs, du, malpha = step(X0, Q, P, F, f, None)
            out.update(dlt_x0=x0, dlt_u=u, dlt_x=np_(X), dlt_F=np_(F), dlt_f=np_(f), dlt_nx=np_(nx),
                       dlt_nu=np_(nu), dlt_costs=np_(costs), dlt_malpha=np_(malpha))
            # ---- MPC(u_zero_I): cartpole unconstrained / +-10, rocket (m = 3) unconstrained
            for tag, mname, T, B, it, bounds in (("zi_cart", "cartpole", 10, 8, 5, None),
                                                 ("zi_cartbox", "cartpole", 10, 8, 5, (-10.0, 10.0)),
                                                 ("zi_rock", "rocket", 10, 4, 3, None)):
                dxm = model(mname)
                rng = np.random.RandomState(7)
                x0 = xinit_for(mname, B, rng)
                zI = rng.uniform(size=(T, B, dxm.n_ctrl)) < 0.25
                Q, P = true_cost(dxm, T, B, dt)
                kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
                decay, mls = (0.5, 2) if mname == "cartpole" else (0.2, 5)
                m = R.mpc_explicit.MPC(dxm.n_state, dxm.n_ctrl, T, lqr_iter=it, eps=0.0, not_improved_lim=10 ** 9,
                                       linesearch_decay=decay, max_linesearch_iter=mls, exit_unconverged=False,
                                       detach_unconverged=False, verbose=-1, u_zero_I=torch.tensor(zI),
                                       grad_method=R.mpc_explicit.GradMethods.ANALYTIC, **kw)
                with torch.no_grad():
                    x, uu, costs = m(torch.tensor(x0, dtype=dt), R.mpc_explicit.QuadCost(Q, P), dxm)
                out.update({f"{tag}_x0": x0, f"{tag}_zI": zI, f"{tag}_x": np_(x), f"{tag}_u": np_(uu),
                            f"{tag}_costs": np_(costs)})
            # ---- the DiLQR no-op step with u_zero_I (its Riccati gains feed the implicit backward)
            mname, T, B = "cartpole", 10, 4
            dxm = model(mname)
            rng = np.random.RandomState(9)
            x0 = xinit_for(mname, B, rng)
            u = rng.uniform(-1, 1, (T, B, 1))
            zI = rng.uniform(size=(T, B, 1)) < 0.25
            Q, P = true_cost(dxm, T, B, dt)
            wx, wu = rng.normal(size=(T, B, 5)), rng.normal(size=(T, B, 1))
            X = R.util.get_traj(T, torch.tensor(u, dtype=dt), x_init=torch.tensor(x0, dtype=dt), dynamics=dxm)
            theta = dxm.params.detach().clone().to(dt).requires_grad_(True)
            Qg, Pg = Q.clone().requires_grad_(True), P.clone().requires_grad_(True)
            mm = R.mpc_explicit.MPC(5, 1, T, grad_method=R.mpc_explicit.GradMethods.ANALYTIC)
            F, f = mm.linearize_dynamics(X, torch.tensor(u, dtype=dt), dxm, diff=True)
            step = R.lqr_step_explicit.LQRStep(5, 1, T, u_zero_I=torch.tensor(zI), true_cost=R.mpc_explicit.QuadCost(
                Qg, Pg), true_dynamics=dxm, current_x=X.detach(), current_u=torch.tensor(u, dtype=dt),
                back_eps=mm.back_eps, no_op_forward=True)
            x2, u2 = step(torch.tensor(x0, dtype=dt), Qg, Pg, F.detach(), f.detach(), theta)
            ((x2 * torch.tensor(wx, dtype=dt)).sum() + (u2 * torch.tensor(wu, dtype=dt)).sum()).backward()
            out.update(zim_x0=x0, zim_u=u, zim_x=np_(X), zim_zI=zI, zim_wx=wx, zim_wu=wu, zim_dQ=np_(Qg.grad),
                       zim_dP=np_(Pg.grad), zim_dtheta=np_(theta.grad))
        save(f"api_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# M. LQRStep (both variants) with a generic true_cost / true_dynamics: the line
#    search evaluates true_cost(new_xut) and true_dynamics(x, u)
#    (lqr_step_explicit.py:226-236, lqr_step.py:224-234)
# --------------------------------------------------------------------------
def case_stepgen():
    import dynamics as ref_dyn
    print("M. LQRStep with generic true_cost / true_dynamics")
    dt = torch.float64
    out = {}
    with default_dtype(dt), contextlib.redirect_stdout(io.StringIO()):
        # ---- pendulum, non-quadratic true_cost, the sweep on the true objective's C, c
        T, B = 10, 8
        rng = np.random.RandomState(31)
        dxp = model("pendulum")
        x0 = xinit_for("pendulum", B, rng)
        u = rng.uniform(-1, 1, (T, B, 1))
        wq = 0.3 * rng.normal(size=4)
        X0, U = torch.tensor(x0), torch.tensor(u)
        Q, P = true_cost(dxp, T, B, dt)
        cost = NQCost(torch.tensor(wq))
        with torch.no_grad():
            X = R.util.get_traj(T, U, x_init=X0, dynamics=dxp)
            F, f = R.mpc_explicit.MPC(3, 1, T, lqr_iter=1).linearize_dynamics(X, U, dxp, diff=False)
        out.update(nq_x0=x0, nq_u=u, nq_w=wq, nq_X=np_(X), nq_F=np_(F), nq_f=np_(f))
        for tag, mod in (("explicit", R.lqr_step_explicit), ("classic", R.lqr_step)):
            step = mod.LQRStep(3, 1, T, u_lower=-2.0, u_upper=2.0, true_cost=cost, true_dynamics=dxp,
                               current_x=X, current_u=U, linesearch_decay=0.2, max_linesearch_iter=5)
            args = (X0, Q, P, F, f) + ((None,) if tag == "explicit" else ())
            with torch.no_grad():
                nx, nu, nqp, costs, du, malpha = step(*args)
            out.update({f"nq_{tag}_nx": np_(nx), f"nq_{tag}_nu": np_(nu), f"nq_{tag}_costs": np_(costs),
                        f"nq_{tag}_du": np_(du), f"nq_{tag}_malpha": np_(malpha), f"nq_{tag}_nqp": np_(nqp)})
        # ---- NNDynamics true_dynamics (n=5, m=1), quadratic true_cost, AUTO_DIFF linearisation
        torch.manual_seed(5)
        nn_dx = ref_dyn.NNDynamics(5, 1, hidden_sizes=[32], activation="sigmoid")
        for i, fc in enumerate(nn_dx.fcs):
            out[f"nn_W{i}"], out[f"nn_b{i}"] = np_(fc.weight), np_(fc.bias)
        x0 = 0.3 * rng.normal(size=(B, 5))
        u = 0.3 * rng.normal(size=(T, B, 1))
        L = rng.normal(size=(T, B, 6, 6)) * 0.3
        C = L @ np.swapaxes(L, -1, -2) + np.eye(6)
        c = 0.1 * rng.normal(size=(T, B, 6))
        X0, U, Ct, ct = (torch.tensor(a) for a in (x0, u, C, c))
        X = R.util.get_traj(T, U, x_init=X0, dynamics=nn_dx).detach()
        F, f = R.mpc_explicit.MPC(5, 1, T, lqr_iter=1, grad_method=R.mpc_explicit.GradMethods.AUTO_DIFF
                                  ).linearize_dynamics(X, U, nn_dx, diff=False)
        F, f = F.detach(), f.detach()
        out.update(nn_x0=x0, nn_u=u, nn_C=C, nn_c=c, nn_X=np_(X), nn_F=np_(F), nn_f=np_(f))
        for tag, mod in (("explicit", R.lqr_step_explicit), ("classic", R.lqr_step)):
            step = mod.LQRStep(5, 1, T, u_lower=-1.0, u_upper=1.0, true_cost=R.mpc_explicit.QuadCost(Ct, ct),
                               true_dynamics=nn_dx, current_x=X, current_u=U, linesearch_decay=0.2,
                               max_linesearch_iter=10)
            args = (X0, Ct, ct, F, f) + ((None,) if tag == "explicit" else ())
            with torch.no_grad():
                nx, nu, nqp, costs, du, malpha = step(*args)
            out.update({f"nn_{tag}_nx": np_(nx), f"nn_{tag}_nu": np_(nu), f"nn_{tag}_costs": np_(costs),
                        f"nn_{tag}_du": np_(du), f"nn_{tag}_malpha": np_(malpha), f"nn_{tag}_nqp": np_(nqp)})
    save("stepgen_f64", **out)


# --------------------------------------------------------------------------
# L. the 5-parameter pendulum (pendulum.py simple=False, il_env.py:40-42
#    'pendulum-complex'): forward, its autograd Jacobian (the reference's own
#    closed forms unpack three parameters and fail for it), and MPC solves
#    through mpc_explicit.MPC with GradMethods.AUTO_DIFF, the runnable path
# --------------------------------------------------------------------------
COMPLEX_PARAMS = (10., 1., 1., 1.0, 0.1)        # il_env.py:41
COMPLEX_MPC = {
    # name: (T, B, lqr_iter, eps, not_improved_lim)  bounds +-2, decay 0.2, max_ls 5 (pendulum.py:52-58)
    "fixed": (20, 16, 10, 0.0, 10 ** 9),
    "il": (20, 16, 40, 1e-3, 5),
}


def case_complex():
    print("L. pendulum-complex")
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt):
            out = {}
            dxm = R.pendulum.PendulumDx(torch.tensor(COMPLEX_PARAMS, dtype=dt), simple=False)
            rng = np.random.RandomState(21)
            x, u = sample_states("pendulum", 256, rng)
            X = torch.tensor(x, dtype=dt, requires_grad=True)
            U = torch.tensor(u, dtype=dt, requires_grad=True)
            nx = dxm(X, U)
            rows = [torch.autograd.grad(nx[:, j].sum(), [X, U], retain_graph=True) for j in range(3)]
            D = torch.stack([torch.cat(r, 1) for r in rows], 1)          # [N, n, d], as AUTO_DIFF forms it
            out.update(x=x, u=u, fwd=np_(nx), jac=np_(D))
            for name, (T, B, it, eps, nil) in COMPLEX_MPC.items():
                rng = np.random.RandomState(3)
                x0 = xinit_for("pendulum", B, rng)
                Q, P = true_cost(dxm, T, B, dt)
                m = R.mpc_explicit.MPC(3, 1, T, u_lower=-2.0, u_upper=2.0, lqr_iter=it, eps=eps,
                                       not_improved_lim=nil, linesearch_decay=0.2, max_linesearch_iter=5,
                                       exit_unconverged=False, detach_unconverged=False, verbose=-1,
                                       grad_method=R.mpc_explicit.GradMethods.AUTO_DIFF)
                # AUTO_DIFF differentiates the dynamics with torch.autograd.grad
                # (mpc_explicit.py:562-566): grad mode stays on
                with contextlib.redirect_stdout(io.StringIO()):
                    xs, us, costs = m(torch.tensor(x0, dtype=dt), R.mpc_explicit.QuadCost(Q, P), dxm)
                out.update({f"{name}_x0": x0, f"{name}_x": np_(xs), f"{name}_u": np_(us),
                            f"{name}_costs": np_(costs)})
            save(f"complex_{tname(dt)}", **out)


# --------------------------------------------------------------------------
# N. dense, time-varying and asymmetric costs (tests/cost_cases.py): sweeps
#    through LQRStepFn.forward and mpc_explicit.MPC solves.  Writes only
#    costs_{f64,f32}.npz; the costs themselves are not stored (seeds + checksums)
# --------------------------------------------------------------------------
def _cost_cases():
    for p_ in (os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))):
        if p_ not in sys.path:
            sys.path.append(p_)
    import cost_cases
    from oracle import models as omodels

    def true_obj(mname):
        q, p = omodels.MODELS[mname].true_obj()
        rq, rp = model(mname).get_true_obj()          # the oracle's restatement is the reference's
        assert np.allclose(q, np_(rq), rtol=1e-6, atol=0) and np.allclose(p, np_(rp), rtol=1e-6, atol=0)
        return q, p
    return cost_cases, true_obj


def replay_spread32(CC, name, x0, C, c):
    """Each problem's fp32 conditioning under decision replay, measured with no
    kernel in the loop: the numpy oracle run in float32 (one problem at a time,
    as the device solves), its line-search and best-iterate decisions forced on
    the fp64 oracle, and the relative cost difference per problem: what the
    GPU tests' check_against_forced_oracle measures of the device."""
    from oracle import models as omodels
    from oracle import mpc as ompc
    mname, T, _B, it, bounds, decay, mls, _mixed = CC.MPC_CASES[name]
    lo, hi = bounds if bounds else (None, None)
    kw = dict(u_lower=lo, u_upper=hi, lqr_iter=it, eps=0.0, not_improved_lim=10 ** 9, linesearch_decay=decay,
              max_linesearch_iter=mls, per_problem=True)
    f = np.float32
    tr = []
    _, _, c32, _ = ompc.mpc_forward(omodels.MODELS[mname], x0.astype(f), C.astype(f), c.astype(f), T, trace=tr, **kw)
    force = lambda i: (tr[i]["alpha_free"].astype(np.float64), tr[i]["take_free"])  # noqa: E731
    _, _, c64, _ = ompc.mpc_forward(omodels.MODELS[mname], x0, C, c, T, force=force, **kw)
    return np.abs(c32 - c64) / np.maximum(1.0, np.abs(c64))


def sweep_via_forward(step_mod, n, m, T, C, c, F, x, u, **kw):
    """K, k (natural time order) of the sweep as LQRStepFn.forward runs it from
    current_x, current_u: c_back is formed inside forward
    (lqr_step_explicit.py:630-636, lqr_step_backup.py:388-394).  The closure's
    lqr_backward is wrapped to keep its result and lqr_forward (which needs
    true dynamics) is replaced by a stand-in."""
    fn = step_mod.LQRStep(n, m, T, current_x=x, current_u=u, **kw).__self__.forward
    cells = dict(zip(fn.__code__.co_freevars, fn.__closure__))
    inner = cells["lqr_backward"].cell_contents
    got = {}

    def keep(ctx, *a):
        got["Ks"], got["ks"], nqp = inner(ctx, *a)
        return got["Ks"], got["ks"], nqp
    none = types.SimpleNamespace(costs=None, full_du_norm=None, mean_alphas=None)
    cells["lqr_backward"].cell_contents = keep
    cells["lqr_forward"].cell_contents = lambda *a: (None, None, none)
    fn(types.SimpleNamespace(save_for_backward=lambda *a: None), x[0], C, c, F)
    return np_(got["Ks"][::-1]), np_(got["ks"][::-1])


COST_SWEEP_SEEDS = {"s31": 31, "s51": 51, "s42": 42, "s43": 43, "s133": 133}
# first seed tried per MPC case; the generator walks up from it until the
# conditioning condition below holds, and stores the seed it used
COST_MPC_SEED0 = {"cart_mixed_unc": 0, "cart_mixed_box10": 0, "pend_mixed_box": 0, "rocket_dense_unc": 0,
                  "rocket_dense_box20": 0, "rocket_diag_it10": 0}
COST_SPREAD_WIDE, COST_SPREAD_CAP = 1e-5, 1e-3     # at most 1 problem in 16 above WIDE, none above CAP
# A second, stricter condition on the same inputs.  The GPU tests hold a
# problem's cost to max(1e-5, 3 x the reference's fp32-vs-fp64 spread), which
# takes one fp32 run's error to bound another's within 3x.  The reference's
# free-running fp32 solve is a single sample and can understate a problem's
# sensitivity (seed 0, cart_mixed_box10 problem 0: reference spread 2.4e-6,
# the float32 numpy oracle under decision replay 4.4e-5; the swing-up error
# grows ~10x per iteration over the last iterations there).  So a fixture is
# used only if a second fp32 implementation that is not under test, the numpy
# oracle in float32 (replay_spread32), meets that bar with the same factor 3
# to spare on every problem.
COST_REPLAY_MARGIN = 3.0


def run_mpc_cost(CC, name, dt, x0, C, c):
    mname, T, _B, it, bounds, decay, mls, _mixed = CC.MPC_CASES[name]
    dx = model(mname)
    kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
    m = R.mpc_explicit.MPC(dx.n_state, dx.n_ctrl, T, lqr_iter=it, eps=0.0, not_improved_lim=10 ** 9,
                           linesearch_decay=decay, max_linesearch_iter=mls, exit_unconverged=False,
                           detach_unconverged=False, verbose=-1, u_init=None,
                           grad_method=R.mpc_explicit.GradMethods.ANALYTIC, **kw)
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        x, u, costs = m(torch.tensor(x0, dtype=dt), R.mpc_explicit.QuadCost(
            torch.tensor(C, dtype=dt), torch.tensor(c, dtype=dt)), dx)
    return np_(x).astype(np.float64), np_(u).astype(np.float64), np_(costs).astype(np.float64)


def case_costs():
    print("N. dense / time-varying / asymmetric costs")
    CC, true_obj = _cost_cases()
    out = {torch.float64: {}, torch.float32: {}}
    rel = lambda a, b: np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))  # noqa: E731
    # ---- sweeps
    for name, seed in COST_SWEEP_SEEDS.items():
        pr = CC.sweep_problem(name, true_obj, seed)
        n, m, T = pr["n"], pr["m"], CC.SWEEP_T
        for dt in out:
            o = out[dt]
            o[f"{name}_seed"] = np.array(seed)
            o[f"{name}_sum"] = CC.checksum(pr["C"], pr["c"], pr["C_box"], pr["c_box"], pr["F"], pr["x"], pr["u"])
            with default_dtype(dt), torch.no_grad():
                t_ = lambda a: torch.tensor(a, dtype=dt)  # noqa: E731
                F, x, u = t_(pr["F"]), t_(pr["x"]), t_(pr["u"])
                for mode in CC.SWEEP_MODES[name]:
                    C, c = (pr["C_box"], pr["c_box"]) if mode == "box" else (pr["C"], pr["c"])
                    mod = R.lqr_step_backup if mode == "chol" else R.lqr_step_explicit
                    kw = dict(u_lower=-CC.SWEEP_BOX, u_upper=CC.SWEEP_BOX) if mode == "box" else {}
                    K, k = sweep_via_forward(mod, n, m, T, t_(C), t_(c), F, x, u, **kw)
                    assert np.isfinite(K).all() and np.isfinite(k).all(), (name, mode)
                    o[f"{name}_{mode}_K"], o[f"{name}_{mode}_k"] = K, k
        print(f"  sweep {name}: modes {CC.SWEEP_MODES[name]}, fp32-vs-fp64 K " +
              ", ".join(f"{mo} {rel(out[torch.float32][f'{name}_{mo}_K'], out[torch.float64][f'{name}_{mo}_K']):.1e}"
                        for mo in CC.SWEEP_MODES[name]))
    # ---- MPC solves
    for name, (mname, T, Bf, it, bounds, decay, mls, mixed) in CC.MPC_CASES.items():
        for seed in range(COST_MPC_SEED0[name], COST_MPC_SEED0[name] + 40):
            x0 = CC.f32(xinit_for(mname, Bf, np.random.RandomState(seed)))
            C, c = CC.mpc_costs(name, true_obj, seed)
            res = {}
            for dt in out:
                with default_dtype(dt):
                    res[dt] = run_mpc_cost(CC, name, dt, x0, C, c)
            (x64, u64, c64), (x32, u32, c32) = res[torch.float64], res[torch.float32]
            spread = np.abs(c32 - c64) / np.maximum(1.0, np.abs(c64))
            ok = np.isfinite(c64).all() and np.isfinite(c32).all() and \
                int((spread > COST_SPREAD_WIDE).sum()) <= Bf // 16 and not (spread > COST_SPREAD_CAP).any()
            replay = replay_spread32(CC, name, x0, C, c)
            bar = np.maximum(COST_SPREAD_WIDE, 3 * spread) / COST_REPLAY_MARGIN
            ok = ok and bool(np.all(replay < bar))
            print(f"  mpc {name} seed {seed}: spread max {spread.max():.2e}, above {COST_SPREAD_WIDE:g}: "
                  f"{int((spread > COST_SPREAD_WIDE).sum())}/{Bf}, x {rel(x32, x64):.1e}, u {rel(u32, u64):.1e}; "
                  f"float32 oracle replay max {replay.max():.2e}, over its bar: {np.flatnonzero(replay >= bar)}"
                  f"{'' if ok else '  -> next seed'}")
            if ok:
                break
        # the condition on the inputs (the cap is fixed; a seed that misses it is not used)
        assert ok, name
        assert int((spread > COST_SPREAD_WIDE).sum()) <= Bf // 16 and spread.max() <= COST_SPREAD_CAP
        assert np.all(replay < np.maximum(COST_SPREAD_WIDE, 3 * spread) / COST_REPLAY_MARGIN)
        for dt, (x, u, costs) in res.items():
            out[dt].update({f"{name}_seed": np.array(seed), f"{name}_sum": CC.checksum(C, c), f"{name}_x0": x0,
                            f"{name}_x": x, f"{name}_u": u, f"{name}_costs": costs,
                            f"{name}_spread": spread, f"{name}_replay32": replay, f"{name}_spread_x": np.array(rel(x32, x64)),
                            f"{name}_spread_u": np.array(rel(u32, u64))})
    for dt in out:
        save(f"costs_{tname(dt)}", **out[dt])


# --------------------------------------------------------------------------
# O. the implicit backward on the fifteen cost classes of cost_cases.BACKWARD_CLASSES
#    (one problem of each, T = 10).  Writes implicit_costs_f64.npz; the costs are
#    regenerated from the seed (checksum stored)
# --------------------------------------------------------------------------
IMPLICIT_COST_CASES = {
    # tag (its model and the horizon are cost_cases.IMPLICIT_COSTS, IMPLICIT_COSTS_T):
    # (box half-widths to walk (None: unconstrained), MPC_CASES entry for decay / max_ls)
    "cart_unc": (None, "cart_unc"),
    "cart_box": ((5.0, 3.0, 2.0, 1.0), "cart_box10"),
    "pend_box": ((2.0, 1.5, 1.0, 0.5), "pend_box"),
    "rock_unc": (None, "rocket_unc"),
    "rock_box": ((10.0, 7.0, 5.0, 3.0), "rocket_unc"),
}
IC_ORACLE_BAR = {"cartpole": 1e-6, "pendulum": 1e-6, "rocket": 2e-5}     # test_implicit_backward_fast_f64's
IC_F32_BAR = 1e-4 / 3                # the float32 numpy oracle, per problem: a third of the device's bar
IC_NEAR = (1e-8, 1e-5)               # no control this close to a bound without being on it
# A last pass that wrongly keeps its registers (or reads C_ux for C_xu) must move
# the classes aimed at it by ten times the device's bar, measured on the fp64
# oracle with that pass's C, c replaced (pass_d_variant).  Required of the
# unconstrained fixtures (in a boxed one a class whose early controls are all
# active has y = 0 up to the changed step, so nothing to move), recorded for all.
IC_SENS = 1e-3
IC_SENS_REQUIRED = {
    "cartpole": {"c_regs": ("diag_tv", "tinv_dense", "dense", "asym", "asym_t0", "asym_mid", "asym_last",
                            "diag_mid", "pair_mid"),
                 "cv_regs": ("diag_cvar", "c_mid"), "xu_T": ("asym", "asym_mid", "asym_last")},
    "rocket": {"c_regs": ("diag_mid", "pair_mid"), "cv_regs": ("c_mid",), "xu_T": ("asym",)},
}


def pass_d_variant(om, wx, wu, C, c, F, x, u, K_rev, lo, hi, Cd, cd, xu_T=False):
    """dtheta of oracle.adjoint.implicit_backward_fast with the kernels' last
    pass reading (Cd, cd) where it should read (C, c): y from the true C, then
    lam, M_t, w, dlam from (Cd, cd); xu_T: C_ux^T for C_xu in dlam.  dC, dc
    depend on y alone, so only dtheta can tell."""
    from oracle import adjoint as oadj
    from oracle import lqr as olqr
    T, B, n = wx.shape
    m = wu.shape[2]
    d = n + m
    g = np.concatenate([wx, wu], 2)
    I = oadj._active_set(u, lo, hi)
    gD, gd, Dx, Du, *_ = om.grad_input(x, u, K_rev, None)
    Dtau = np.concatenate([Dx, Du], -1)
    xu = np.concatenate([x, u], 2)

    def lam_M(C_, c_):
        lams, prev = [None] * T, None
        for t in range(T - 1, -1, -1):
            lam = olqr.bmv(C_[t, :, :n], xu[t]) + c_[t, :, :n]
            if prev is not None:
                lam = lam + olqr.bmv(np.swapaxes(F[t, :, :, :n], 1, 2), prev)
            lams[t] = prev = lam
        M = np.zeros((T, B, d, d))
        for t in range(T - 1):
            M[t] = np.einsum("bi,bijk->bjk", lams[t + 1], Dtau[t])
        return lams, M
    y = oadj.adjoint_lqr_linear(C + np.swapaxes(lam_M(C, c)[1], 2, 3), g, F, n, m, I)
    lams, M = lam_M(Cd, cd)
    w = g - np.einsum("tbjk,tbj->tbk", M, y)
    dth, prev = np.zeros((B, om.n_params)), None
    dlam = [None] * T
    for t in range(T - 1, -1, -1):
        Cxu = np.swapaxes(Cd[t, :, n:, :n], 1, 2) if xu_T else Cd[t, :, :n, n:]
        dl = olqr.bmv(Cd[t, :, :n, :n], y[t, :, :n]) + olqr.bmv(Cxu, y[t, :, n:]) - w[t, :, :n]
        if prev is not None:
            dl = dl + olqr.bmv(np.swapaxes(F[t, :, :, :n], 1, 2), prev)
        dlam[t] = prev = dl
    for t in range(T - 1):
        dF = -(dlam[t + 1][:, :, None] * xu[t][:, None, :] + lams[t + 1][:, :, None] * y[t][:, None, :])
        dth += np.einsum("bnm,bnmk->bk", dF, gD[t]) - np.einsum("bn,bnk->bk", dlam[t + 1], gd[t])
    return dth


def ic_solver(CC, dx, mpc_case, T, C, c, bounds):
    """solve(x0) for one cost set: the reference's MPC solve rounded to float32
    and, per problem, the active and free counts, the controls near a bound
    without being on it, and whether the problem meets the conditions."""
    _, _, _, _, _, _, _, decay, mls = MPC_CASES[mpc_case]
    B = C.shape[1]
    Q, P = torch.tensor(C), torch.tensor(c)
    kw = {} if bounds is None else dict(u_lower=bounds[0], u_upper=bounds[1])
    mp = R.mpc_explicit.MPC(dx.n_state, dx.n_ctrl, T, lqr_iter=30, eps=1e-6, linesearch_decay=decay,
                            max_linesearch_iter=mls, exit_unconverged=False, detach_unconverged=False, verbose=-1,
                            grad_method=R.mpc_explicit.GradMethods.ANALYTIC, **kw)

    def solve(x0):
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            x, u, _ = mp(torch.tensor(x0), R.mpc_explicit.QuadCost(Q, P), dx)
        x, u = CC.f32(np_(x)), CC.f32(np_(u))
        good = np.isfinite(x).all((0, 2)) & np.isfinite(u).all((0, 2))
        if bounds is None:
            return x, u, np.full(B, -1), np.full(B, -1), np.zeros(B, int), good
        gap = np.minimum(np.abs(u - bounds[0]), np.abs(u - bounds[1]))
        act = gap <= IC_NEAR[0]
        na, nf = act.sum((0, 2)), (~act).sum((0, 2))
        nr = ((gap > IC_NEAR[0]) & (gap < IC_NEAR[1])).sum((0, 2))
        return x, u, na, nf, nr, good & (na >= 2) & (nf >= 2) & (nr == 0)
    return solve


def ic_walk_x0(CC, mname, B, n, seed, solve):
    """One box width serves every class only if each problem starts where its
    own cost saturates some controls and not all: problem b takes the first
    initial state, walking the x0 seed up from the cost seed, at which it meets
    the conditions (the problems already placed keep theirs while the rest
    walk).  Returns x0 [B,n], the seed of each (-1: none in 40)."""
    x0, x0_seed = np.zeros((B, n)), np.full(B, -1)
    for s in range(seed, seed + 40):
        cand = CC.f32(xinit_for(mname, B, np.random.RandomState(s)))
        good = solve(np.where((x0_seed < 0)[:, None], cand, x0))[5] & (x0_seed < 0)
        x0[good], x0_seed[good] = cand[good], s
        if (x0_seed >= 0).all():
            break
    return x0, x0_seed


def ic_oracles(om, n, m, x, u, wx, wu, C, c, lo, hi, dtype):
    """implicit_backward_fast in dtype on the fixture; also F and the reversed gains."""
    from oracle import adjoint as oadj
    from oracle import lqr as olqr
    from oracle import mpc as ompc
    f = lambda a: a.astype(dtype)  # noqa: E731
    Fo, fo = ompc.linearize(om, f(x), f(u))
    K, _, _ = olqr.lqr_backward(f(C), olqr.c_back(f(C), f(c), f(x), f(u)), Fo, n, m, u=f(u), u_lower=lo, u_upper=hi)
    got = oadj.implicit_backward_fast(om, f(wx), f(wu), f(C), f(c), Fo, fo, f(x), f(u), K[::-1], lo, hi)
    assert all(a.dtype == dtype for a in got)
    return got, Fo, K[::-1]


def ic_sensitivity(CC, om, wx, wu, C, c, Fo, x, u, K_rev, lo, hi, dth):
    """Per problem, how far dtheta moves when the last pass alone keeps step
    T-1's diagonal (c_regs), step T-1's c (cv_regs), or reads C_ux^T for C_xu."""
    T, d = C.shape[0], C.shape[-1]
    Cr, cr = np.zeros_like(C), np.zeros_like(c)
    Cr[:], cr[:] = C[T - 1] * np.eye(d), c[T - 1]
    return {mut: CC.per_problem(pass_d_variant(om, wx, wu, C, c, Fo, x, u, K_rev, lo, hi, Cd, cd, xu_T), dth, 0)
            for mut, (Cd, cd, xu_T) in {"c_regs": (Cr, c, False), "cv_regs": (C, cr, False),
                                        "xu_T": (C, c, True)}.items()}


def ic_reference(CC, label, mname, T, bounds, cls, x, u, x0, C, c, wx, wu, like):
    """The reference's backward, one problem at a time.  It cannot run a batch
    of one (fix_point_equ reads A[1], lqr_step_explicit.py:561), so the batch is
    the problem twice, the copy with zero loss weights: dtheta is the problem's
    own.  Then the batch run: the same per-problem dQ, dP, and its dtheta the
    sum (asserted to 1e-10).  Returns [dQ, dP, dtheta_b] (nan where the
    reference raised, allowed on an asymmetric class only), raised [B], the
    batch-vs-singles error of dQ/dP and of the dtheta sum."""
    dt = torch.float64
    Q, P = torch.tensor(C), torch.tensor(c)
    B = len(cls)
    ref = [np.full_like(a, np.nan) for a in like]
    raised = np.zeros(B, bool)
    mask = np.array([1.0, 0.0])[None, :, None]
    for j in range(B):
        s = [j, j]
        try:
            dQ, dP, dth, _, _ = implicit_once(mname, T, 2, bounds, x[:, s], u[:, s], x0[s], Q[:, s], P[:, s],
                                              wx[:, s] * mask, wu[:, s] * mask, dt)
            ref[0][:, j], ref[1][:, j], ref[2][j] = dQ[:, 0], dP[:, 0], dth
        except Exception as e:        # noqa: BLE001 (recorded by the caller)
            assert cls[j] in CC.ASYM, (label, cls[j], e)
            raised[j] = True
            print(label, f"the reference raised on {cls[j]}: {type(e).__name__}: {e}")
    ok = np.flatnonzero(~raised)
    bQ, bP, bth, _, _ = implicit_once(mname, T, ok.size, bounds, x[:, ok], u[:, ok], x0[ok], Q[:, ok], P[:, ok],
                                      wx[:, ok], wu[:, ok], dt)
    sum_err = np.max(np.abs(bth - ref[2][ok].sum(0))) / np.max(np.abs(bth))
    assert sum_err < 1e-10, (label, sum_err)
    bat_err = max(CC.per_problem(bQ, ref[0][:, ok], 1).max(), CC.per_problem(bP, ref[1][:, ok], 1).max())
    return ref, raised, bat_err, sum_err


def ic_attempt(CC, true_obj, tag, mpc_case, seed, width):
    """One cost seed and box width of one fixture: the arrays to store (keys
    without the tag), or None with the failed condition printed."""
    from oracle import models as omodels
    mname = CC.IMPLICIT_COSTS[tag]
    T, cls = CC.IMPLICIT_COSTS_T, list(CC.BACKWARD_CLASSES)
    B, pp = len(cls), CC.per_problem
    label = f"  {tag} seed {seed} width {width}:"
    dx, om = model(mname), omodels.MODELS[mname]
    n, m = dx.n_state, dx.n_ctrl
    q, p = true_obj(mname)
    lo, hi = (-width, width) if width else (None, None)
    bounds = (lo, hi) if width else None
    C, c = CC.make_backward_costs(q, p, n, T, cls, seed, sym_uu=width is not None and m > 1)
    solve = ic_solver(CC, dx, mpc_case, T, C, c, bounds)
    x0, x0_seed = ic_walk_x0(CC, mname, B, n, seed, solve)
    if (x0_seed < 0).any():
        print(label, f"no initial state in 40 for {[cls[j] for j in np.flatnonzero(x0_seed < 0)]} -> next")
        return None
    x, u, n_act, n_free, near, good = solve(x0)
    if not good.all():         # the reference's solve couples the batch (its line search)
        print(label, f"active {n_act}, free {n_free}, near a bound {near} -> next")
        return None
    rng = np.random.RandomState(seed + 1000)
    wx, wu = CC.f32(rng.normal(size=x.shape)), CC.f32(rng.normal(size=u.shape))
    # the two oracles and the sensitivity condition, before the (slow) reference
    o64, Fo, K_rev = ic_oracles(om, n, m, x, u, wx, wu, C, c, lo, hi, np.float64)
    o32 = ic_oracles(om, n, m, x, u, wx, wu, C, c, lo, hi, np.float32)[0]
    sens = ic_sensitivity(CC, om, wx, wu, C, c, Fo, x, u, K_rev, lo, hi, o64[2])
    if bounds is None:
        weak = [(mut, k, float(sens[mut][cls.index(k)])) for mut, ks in IC_SENS_REQUIRED[mname].items() for k in ks
                if sens[mut][cls.index(k)] < IC_SENS]
        if weak:
            print(label, f"a mutated last pass moves too little: {weak} -> next")
            return None
    ref, raised, bat_err, sum_err = ic_reference(CC, label, mname, T, bounds, cls, x, u, x0, C, c, wx, wu, o64)
    e64 = np.stack([pp(o64[0], ref[0], 1), pp(o64[1], ref[1], 1), pp(o64[2], ref[2], 0)], 1)
    e64[raised] = np.nan
    bar = IC_ORACLE_BAR[mname]
    off = raised | ~(e64.max(1) < bar)
    # an asymmetric class on which the reference raises or leaves the oracles is kept,
    # pinned to the fp64 oracle; any other class must meet the bar
    if any(cls[j] not in CC.ASYM for j in np.flatnonzero(off)):
        print(label, f"oracle vs reference {e64.max(1)} over {bar:g} on a symmetric class -> next")
        return None
    exp = [np.where(off.reshape((1, B) + (1,) * (a.ndim - 2)) if a.ndim > 2 else off[:, None], o, a)
           for a, o in zip(ref, o64)]
    e32 = np.stack([pp(o32[0], exp[0], 1), pp(o32[1], exp[1], 1), pp(o32[2], exp[2], 0)], 1)
    if not e32.max() < IC_F32_BAR:
        print(label, f"float32 oracle {e32.max(0)} over {IC_F32_BAR:.1e} -> next")
        return None
    # the conditions, once more, on what is stored
    assert bounds is None or (n_act.min() >= 2 and n_free.min() >= 2 and near.max() == 0)
    assert e32.max() < IC_F32_BAR and np.nanmax(np.where(off[:, None], 0.0, e64)) < bar
    print(f"  {tag}: seed {seed}, x0 seeds {x0_seed}, width {width}, active {n_act if bounds else '-'}; oracle vs reference "
          f"dC {np.nanmax(e64[:, 0]):.1e} dc {np.nanmax(e64[:, 1]):.1e} dtheta {np.nanmax(e64[:, 2]):.1e}; "
          f"float32 oracle dC {e32[:, 0].max():.1e} dc {e32[:, 1].max():.1e} dtheta {e32[:, 2].max():.1e}; "
          f"batch vs singles dQ/dP {bat_err:.1e}, sum dtheta {sum_err:.1e}; "
          f"oracle-pinned: {[cls[j] for j in np.flatnonzero(off)]}")
    for mut, e in sens.items():
        print(f"    last pass with {mut}: " + " ".join(f"{k} {v:.0e}" for k, v in zip(cls, e) if v > 0))
    return {"seed": np.array(seed), "width": np.array(width if width else 0.0), "sum": CC.checksum(C, c), "x0": x0,
            "x0_seed": x0_seed, "x": x, "u": u, "wx": wx, "wu": wu, "dQ": exp[0], "dP": exp[1], "dtheta": exp[2],
            "pinned": off, "raised": raised, "oracle_err": e64, "f32_err": e32, "n_active": n_act,
            "sum_err": np.array(sum_err),
            # the reference's own answer where the expected value is the oracle's
            "ref_dQ": ref[0][:, off], "ref_dP": ref[1][:, off], "ref_dtheta": ref[2][off],
            **{f"sens_{mut}": e for mut, e in sens.items()}}


def case_implicit_costs():
    print("O. implicit backward on the cost classes")
    CC, true_obj = _cost_cases()
    assert set(IMPLICIT_COST_CASES) == set(CC.IMPLICIT_COSTS)
    out = {"classes": np.array(CC.BACKWARD_CLASSES)}
    with default_dtype(torch.float64):
        for tag, (widths, mpc_case) in IMPLICIT_COST_CASES.items():
            torch.set_num_threads(1 if CC.IMPLICIT_COSTS[tag] == "rocket" else 8)      # see case_implicit
            tries = ((seed, width) for seed in range(20) for width in widths or (None,))
            res = next((r for r in (ic_attempt(CC, true_obj, tag, mpc_case, s, w) for s, w in tries) if r), None)
            assert res is not None, tag
            out.update({f"{tag}_{k}": v for k, v in res.items()})
    save("implicit_costs_f64", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["models", "riccati", "pnqp", "lqrstep", "mpc", "adjoint", "implicit",
                             "implicit25", "datasets", "il", "generic", "api", "complex", "stepgen", "costs",
                             "implicit_costs"]
    table = {"models": case_models, "riccati": case_riccati, "pnqp": case_pnqp,
             "lqrstep": case_lqrstep, "mpc": case_mpc, "mpc_iterates": case_mpc_iterates,
             "adjoint": case_classic_adjoint,
             "implicit": case_implicit, "implicit25": case_implicit25, "datasets": case_datasets, "il": case_il,
             "generic": case_generic, "api": case_api, "complex": case_complex, "stepgen": case_stepgen,
             "costs": case_costs, "implicit_costs": case_implicit_costs}
    for w in which:
        table[w]()
