#!/usr/bin/env python
"""Time a closed-loop (receding-horizon) MPC episode on the GPU:
dilqr.closed_loop.mpc_episode against the Python loop a user could write
without it, on the same inputs in one process.

Workload: cartpole, T = 25, 25 control steps, lqr_iter = 10, controls within
the model's bounds, the true objective, x0 near upright (angle within +-0.3);
once with the stop rule off (eps = 0, not_improved_lim huge: the fixed-count
solve) and once with eps = dx.mpc_eps.  Batches 32, 4096, 65536.  Arms:
  episode      mpc_episode (solve + advance launch per step, nothing on the host)
  loop         per step a new MPC(u_init=...).forward under no_grad with
               detach_unconverged=False (populate_data2's setting), the model's
               forward on the plan's first control, the shift with torch.cat
               and the reference's u_init[-2] = u_init[-3]
  loop_detach  the same with MPC's default detach_unconverged=True, whose
               float(full_du_norm.max()) waits for the GPU at every step
Per batch, mode and arm: warm-up episodes, then repeated episodes timed with
device events, the arms alternating; the median, min and max per control step
are printed and the arms' trajectories compared.  Then, at that batch, the two
launches an episode's step adds around the solve kernel, each timed alone over
many back-to-back calls: the advance (ops.mpc_advance) and gather_best (the
copy of the best slot the advance reads), with their share of the episode's
step.

    python tools/bench_closed_loop.py [--batches 32,4096,65536] [--modes fixed,stop] [--out FILE]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "differentiable-ilqr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

T, STEPS, LQR_ITER = 25, 25, 10
ARMS = ("episode", "loop", "loop_detach")


def commit():
    try:
        out = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True)
        if out.returncode == 0:
            return out.stdout.strip() + ("+changes" if dirty.stdout.strip() else "")
    except OSError:
        pass
    return os.environ.get("DILQR_COMMIT", "unknown")


def problem(dx, B, dev):
    g = torch.Generator().manual_seed(1234)

    def uniform(lo, hi):
        return torch.rand(B, generator=g) * (hi - lo) + lo
    th = uniform(-0.3, 0.3)
    x0 = torch.stack((uniform(-.5, .5), uniform(-.5, .5), torch.cos(th), torch.sin(th), uniform(-1., 1.)), 1)
    q, p = dx.get_true_obj()
    return x0.to(dev), torch.diag(q).repeat(T, B, 1, 1).to(dev), p.repeat(T, B, 1).to(dev)


def settings(dx, mode, **kw):
    stop = dict(eps=0.0, not_improved_lim=10 ** 9) if mode == "fixed" else dict(eps=dx.mpc_eps)
    return dict(u_lower=float(dx.lower), u_upper=float(dx.upper), lqr_iter=LQR_ITER, verbose=-1,
                exit_unconverged=False, linesearch_decay=dx.linesearch_decay,
                max_linesearch_iter=dx.max_linesearch_iter, **stop, **kw)


def python_loop(dx, x0, cost, mode, detach):
    """The loop a user writes around MPC.forward (il_env.py:116-140, batched)."""
    import dilqr
    x, u_init = x0, None
    xs, us = [x], []
    with torch.no_grad():
        for _ in range(STEPS):
            mpc = dilqr.MPC(dx.n_state, dx.n_ctrl, T, u_init=u_init, **settings(dx, mode, detach_unconverged=detach))
            _, actions, _ = mpc(x, cost, dx)
            x = dx(x, actions[0])
            xs.append(x)
            us.append(actions[0])
            u_init = torch.cat((actions[1:], torch.zeros_like(actions[:1])), dim=0)
            u_init[-2] = u_init[-3]
    return torch.stack(xs), torch.stack(us)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def per_call(fn, calls=200):
    """ms per call of a launch queued back to back (device events around `calls` of them)."""
    for _ in range(10):
        fn()
    ts = []
    for _ in range(5):
        ms, _ = timed(lambda: [fn() for _ in range(calls)])
        ts.append(ms / calls)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,4096,65536")
    ap.add_argument("--modes", default="fixed,stop")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    if not arms or any(a not in ARMS for a in arms) or arms[0] != "episode":
        sys.exit("bench_closed_loop: --arms takes episode first, then any of " + ",".join(ARMS[1:]))
    if not torch.cuda.is_available():
        sys.exit("bench_closed_loop: needs a GPU (no CPU timing)")
    import dilqr
    from dilqr import ops
    from dilqr.closed_loop import mpc_episode
    from dilqr.env_dx.cartpole import CartpoleDx
    dev = torch.device("cuda:0")
    dx = CartpoleDx(torch.tensor((9.8, 1.0, 0.1, 0.5), device=dev))        # parameters on the device: no upload per call
    lines = [f"# bench_closed_loop  commit {commit()}  lib {os.environ.get('DILQR_LIB', 'dilqr/libdilqr.so')}",
             f"# cartpole T={T} steps={STEPS} lqr_iter={LQR_ITER}, bounds and line search from the model, true "
             f"objective; one episode per timing, device events; ms per control step",
             f"# {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             "B        mode   arm          n   median_ms      min_ms      max_ms  vs_episode  max_abs_x_diff"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for s in lines:
        print(s, flush=True)
    for B in [int(b) for b in args.batches.split(",")]:
        x0, C, c = problem(dx, B, dev)
        cost = dilqr.QuadCost(C, c)
        med_episode = {}
        for mode in args.modes.split(","):
            mpc = dilqr.MPC(5, 1, T, **settings(dx, mode, detach_unconverged=False))
            run = {"episode": lambda: mpc_episode(mpc, x0, cost, dx, STEPS)[:2],
                   "loop": lambda: python_loop(dx, x0, cost, mode, False),
                   "loop_detach": lambda: python_loop(dx, x0, cost, mode, True)}
            times, outs = {a: [] for a in arms}, {}
            for a in arms:
                for _ in range(args.warmup):
                    timed(run[a])
            for _ in range(args.repeats):                  # the arms alternate
                for a in arms:
                    ms, outs[a] = timed(run[a])
                    times[a].append(ms / STEPS)
            med = {a: statistics.median(times[a]) for a in arms}
            med_episode[mode] = med["episode"]
            for a in arms:
                t = times[a]
                diff = float((outs[a][0] - outs["episode"][0]).abs().max())
                emit(f"{B:<8d} {mode:<6s} {a:<12s} {len(t):<3d} {med[a]:11.4f} {min(t):11.4f} {max(t):11.4f} "
                     f"{med[a] / med['episode']:9.2f}   {diff:.2e}")
        # the two launches a step adds around the solve kernel, each alone
        fixed = "fixed" in med_episode
        sv = ops.MPCSolve(T, B, 5, 1, dev, fixed_iters=LQR_ITER if fixed else None)
        bounds, _ = ops.N.make_bounds(float(dx.lower), float(dx.upper))
        theta = ops.theta_of(dx, x0)
        if fixed:
            sv.solve_fixed(dx.model_id, theta, x0, C, c, bounds, dx.linesearch_decay, dx.max_linesearch_iter, 1e-4)
        else:
            sv.begin(dx.model_id, theta, x0)
        _, plan = sv.gather_best()
        x_cur, u_warm = x0.clone(), torch.empty_like(plan)
        x_log, u_log, cost_log = torch.empty(B, 5, device=dev), torch.empty(B, 1, device=dev), torch.empty(B, device=dev)
        t_adv = per_call(lambda: ops.mpc_advance(dx.model_id, theta, plan, x_cur, u_warm, "reference", x_log, u_log,
                                                 C, c, cost_log))
        t_gather = per_call(sv.gather_best)
        shares = ", ".join(f"{mode} {100 * t_adv / t:.1f}% + {100 * t_gather / t:.1f}%" for mode, t in
                           med_episode.items())
        emit(f"# B={B}: advance {t_adv:.4f} ms, gather_best {t_gather:.4f} ms per call (each alone, back to back); "
             f"share of the episode's step (advance + gather_best): {shares}")
        del x0, C, c, cost, sv, plan
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
