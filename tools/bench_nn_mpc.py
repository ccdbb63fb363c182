#!/usr/bin/env python
"""Time an MPC solve with learned dynamics (NNDynamics) on the GPU, device MLP
kernels against the torch loop, on the same inputs in one process.

Workload: NNDynamics(5, 1, [100], sigmoid), T = 25, lqr_iter = 10 fixed-count
(eps = 0, not_improved_lim huge), controls in [-1, 1], a dense SPD cost, one
whole mpc.MPC.forward under no_grad.  Batches 32, 4096, 65536.  Three arms:
"torch", generic.DEVICE_MLP = False, the torch loop (the path before the MLP
kernels existed); "device", the four launches per iteration (ops.MLP_FUSED =
False); "fused", the route ops.mlp_solve_route picks with ops.MLP_FUSED on (the
fused iteration per launch); and on request "small", that with the one-launch
solve switched on for the batches one workgroup holds.  Per batch
and arm: warm-up solves, then repeated solves timed with device events, the
arms alternating; median, min and max are printed, the costs are compared with
the first arm's, and the fused route is held against the four launches' median
and spread (the routing rule of DESIGN.md §6b).  Then the linearisation kernel alone
at the largest batch, with its bytes and FLOPs per row.  --hidden 64,64 takes a
network with two hidden layers instead: the device arm then also turns
generic.DEVICE_MLP_DEEP on (csrc/tu_mlp2.hip), the torch arm is the same loop.

--slew-rate-penalty G or --delta-u D (one of them) times the same solve with that
MPC option.  Two arms then: "torch", the path such a solve takes as shipped
(generic.DEVICE_MLP_SLEW / DEVICE_MLP_DELTA_U off: the torch loop, its rollouts
and linearisation on the device model for one hidden layer, every line search
T sequential evaluations of the Module), and "device", the option's switch on
(and DEVICE_MLP_DEEP for two hidden layers): ops.mpc_solve_unfused on
ops.slew_dynamics, or with delta_u, four launches per iteration.  The fused arms
do not apply, and the linearisation kernel is not timed again.

    python tools/bench_nn_mpc.py [--batches 32,4096,65536] [--arms device,fused] [--hidden 64,64] [--out FILE]
                                 [--slew-rate-penalty G | --delta-u D]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "differentiable-ilqr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

N_STATE, N_CTRL, HIDDEN, T, LQR_ITER = 5, 1, 100, 25, 10
PEAK_FP32_FMA = 157.3e12 / 2      # v_fma_f32, unpacked: half the packed-FMA vector peak
PEAK_HBM = 6.29e12                # measured float4 copy


def commit():
    try:
        out = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True)
        if out.returncode == 0:
            return out.stdout.strip() + ("+changes" if dirty.stdout.strip() else "")
    except OSError:
        pass
    return os.environ.get("DILQR_COMMIT", "unknown")


def problem(B, dev):
    g = torch.Generator().manual_seed(1234)
    d = N_STATE + N_CTRL
    L = torch.randn(T, B, d, d, generator=g)
    C = L @ L.transpose(-1, -2) + 0.5 * torch.eye(d)
    c = torch.randn(T, B, d, generator=g)
    x0 = torch.randn(B, N_STATE, generator=g)
    return x0.to(dev), C.to(dev), c.to(dev)


def solver(B, slew_rate_penalty=None, delta_u=None):
    import dilqr.mpc as cmpc
    return cmpc.MPC(N_STATE, N_CTRL, T, lqr_iter=LQR_ITER, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0,
                    u_upper=1.0, n_batch=B, eps=0.0, not_improved_lim=10 ** 9, exit_unconverged=False,
                    detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=10, verbose=-1,
                    slew_rate_penalty=slew_rate_penalty, delta_u=delta_u)


def timed_solve(mpc, x0, cost, dx):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    with torch.no_grad():
        x, u, costs = mpc(x0, cost, dx)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), costs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,4096,65536")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--budget", type=float, default=60.0, help="seconds of timed solves per batch and arm")
    ap.add_argument("--hidden", default=str(HIDDEN), help="hidden widths: one (default) or two, as 64,64")
    ap.add_argument("--arms", default=None, help="arms to time, the first one the baseline (default torch,device,"
                    "fused; torch,device with an MPC option)")
    ap.add_argument("--slew-rate-penalty", type=float, default=None, help="MPC(slew_rate_penalty=G)")
    ap.add_argument("--delta-u", type=float, default=None, help="MPC(delta_u=D)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    option = args.slew_rate_penalty is not None or args.delta_u is not None
    if args.slew_rate_penalty is not None and args.delta_u is not None:
        sys.exit("bench_nn_mpc: --slew-rate-penalty and --delta-u do not go together (no device route for both)")
    if args.arms is None:
        args.arms = "torch,device" if option else "torch,device,fused"
    hidden = [int(h) for h in args.hidden.split(",")]
    if len(hidden) not in (1, 2):
        sys.exit("bench_nn_mpc: --hidden takes one or two widths")
    deep = len(hidden) == 2
    if not torch.cuda.is_available():
        sys.exit("bench_nn_mpc: needs a GPU (no CPU timing)")
    from dilqr import QuadCost, generic, ops
    from dilqr.dynamics import NNDynamics
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dx = NNDynamics(N_STATE, N_CTRL, hidden_sizes=hidden, activation="sigmoid").to(dev)
    lines = [f"# bench_nn_mpc  commit {commit()}  lib {os.environ.get('DILQR_LIB', 'dilqr/libdilqr.so')}",
             f"# NNDynamics({N_STATE},{N_CTRL},{hidden},sigmoid) T={T} lqr_iter={LQR_ITER} fixed-count, u in [-1,1], "
             f"dense SPD cost; one mpc.MPC.forward under no_grad; device events; ms",
             *([f"# MPC option: slew_rate_penalty={args.slew_rate_penalty} delta_u={args.delta_u}; arm torch = the "
                f"option's switch off (as shipped), arm device = on"] if option else []),
             f"# {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
             "B        arm     n   median_ms      min_ms      max_ms   speedup   max_rel_cost_diff"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for s in lines:
        print(s, flush=True)
    # the arms: the torch loop (the path before the MLP kernels existed), the
    # four launches per iteration (ops.MLP_FUSED off: linearise, sweep, line
    # search, best/stop rule), and the route ops.mlp_solve_route picks with
    # ops.MLP_FUSED on (the fused iteration per launch; two hidden layers stay
    # on the four launches)
    # ("small": the fused arm with the one-launch solve switched on up to ops.SMALL_BATCH_MAX; it
    # ships off, so "fused" is the fused iteration per launch at every batch)
    ARMS = {"torch": (False, False), "device": (True, False), "fused": (True, True), "small": (True, True)}
    small_max = ops.MLP_SMALL_MAX_BATCH
    arms = [a for a in args.arms.split(",") if a]
    if not arms or any(a not in ARMS for a in arms):
        sys.exit("bench_nn_mpc: --arms takes a list of " + ",".join(ARMS))
    if option and any(a not in ("torch", "device") for a in arms):
        sys.exit("bench_nn_mpc: with an MPC option the arms are torch and device")

    def arm(name):
        flag, fused = ARMS[name]
        if option:
            # the shipped route against the option's switch (DEVICE_MLP stays on in both)
            generic.DEVICE_MLP_SLEW = flag and args.slew_rate_penalty is not None
            generic.DEVICE_MLP_DELTA_U = flag and args.delta_u is not None
            generic.DEVICE_MLP_DEEP = flag and deep
            return
        generic.DEVICE_MLP = flag
        generic.DEVICE_MLP_DEEP = flag and deep
        ops.MLP_FUSED = fused
        ops.MLP_SMALL_MAX_BATCH = ops.SMALL_BATCH_MAX if name == "small" else small_max

    for B in [int(b) for b in args.batches.split(",")]:
        x0, C, c = problem(B, dev)
        cost, mpc = QuadCost(C, c), solver(B, args.slew_rate_penalty, args.delta_u)
        times, costs = {a: [] for a in arms}, {}
        for a in arms:
            arm(a)
            for _ in range(1 if a == "torch" else args.warmup):
                timed_solve(mpc, x0, cost, dx)
        spent = {a: 0.0 for a in arms}
        for r in range(args.repeats):                      # the arms alternate
            for a in arms:
                if r >= 3 and spent[a] > args.budget:
                    continue
                arm(a)
                t0 = time.perf_counter()
                ms, cs = timed_solve(mpc, x0, cost, dx)
                spent[a] += time.perf_counter() - t0
                times[a].append(ms)
                costs[a] = cs
        generic.DEVICE_MLP, generic.DEVICE_MLP_DEEP, ops.MLP_FUSED = True, False, True
        generic.DEVICE_MLP_SLEW = generic.DEVICE_MLP_DELTA_U = False
        ops.MLP_SMALL_MAX_BATCH = small_max
        base = arms[0]                                     # speed-up and cost difference against the first arm
        med = {a: statistics.median(times[a]) for a in arms}
        for a in arms:
            t = times[a]
            rel = float(((costs[a] - costs[base]).abs() / costs[base].abs().clamp(min=1.0)).max())
            emit(f"{B:<8d} {a:<7s} {len(t):<3d} {med[a]:11.3f} {min(t):11.3f} {max(t):11.3f} "
                 f"{med[base] / med[a]:9.2f}   {rel:.2e}")
        for a in ("fused", "small"):
            if "device" not in arms or a not in arms:
                continue
            # the routing rule of DESIGN.md 6b: a route is taken where it is not slower than the
            # four launches' median by more than that arm's own min-max spread
            spread = max(times["device"]) - min(times["device"])
            same = bool(torch.equal(costs[a], costs["device"]))
            arm(a)
            route = ops.mlp_solve_route(dx.device_model(x0, deep=deep), B, LQR_ITER, None, -1)
            arm("fused")
            emit(f"# B={B}: arm {a} took route {route}, {a} - four-launch medians {med[a] - med['device']:+.3f} ms, "
                 f"four-launch spread {spread:.3f} ms: {'ok' if med[a] <= med['device'] + spread else 'SLOWER'}; "
                 f"costs {'equal bits' if same else 'DIFFER'}")
        del x0, C, c, cost
        torch.cuda.empty_cache()
    if option:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    # the linearisation kernel alone at the largest batch
    B = max(int(b) for b in args.batches.split(","))
    md = dx.device_model(torch.zeros(1, device=dev), deep=deep)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, N_STATE, generator=g).to(dev)
    u = torch.randn(T, B, N_CTRL, generator=g).clamp(-1, 1).to(dev)
    for _ in range(3):
        ops.mlp_linearize(md, x, u)
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.mlp_linearize(md, x, u)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    n, m, d = N_STATE, N_CTRL, N_STATE + N_CTRL
    rows = (T - 1) * B
    byts = (d + n * d + n) * 4
    if deep:
        # layer 1; per (layer-2 unit, layer-1 unit) one FMA for z2, one product and d FMAs for the
        # tangent; per (output, layer-2 unit) the same for the value and the Jacobian
        H1, H2 = hidden
        flops = 2 * H1 * d + (H2 * H1 + n * H2) * (2 * d + 3)
    else:
        H = hidden[0]
        flops = 2 * H * (d + 2 * n + n * d)
    t = statistics.median(ts) * 1e-3
    emit(f"# mlp_linearize B={B}: {rows} rows, call (allocation + kernel, device events) median "
         f"{t * 1e3:.3f} ms, min {min(ts):.3f}, max {max(ts):.3f}")
    emit(f"#   per row {byts} B, {flops} FLOP: {rows * byts / t / 1e12:.3f} TB/s "
         f"({100 * rows * byts / t / PEAK_HBM:.1f}% of {PEAK_HBM / 1e12:.2f} TB/s measured copy), "
         f"{rows * flops / t / 1e12:.2f} TFLOP/s ({100 * rows * flops / t / PEAK_FP32_FMA:.1f}% of "
         f"{PEAK_FP32_FMA / 1e12:.1f} TFLOP/s unpacked fp32 FMA)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
