#!/usr/bin/env python
"""Time the gradient of an MPC solve into learned dynamics (NNDynamics): the
part of a training step after the solve, device VJP of the linearisation
against the torch graph through NNDynamics.grad_input.

Workload: NNDynamics(5, 1, [100], sigmoid), T = 25, bench_nn_mpc.py's solver
settings and inputs; one mpc.MPC.forward with gradients, then
(x . wx + u . wu).sum().backward().  Batches 32, 4096, 65536.  Timed with
device events: from the entry of generic.final_step (the differentiable
linearisation and the no-op LQR step) to the end of the backward; the peak of
torch.cuda.max_memory_allocated over that part is recorded too.

Arms.  On a tree that has generic.DEVICE_MLP_VJP the switch alternates on
("device") and off ("torch") run by run; on an older tree there is the single
arm "torch".  --parent DIR runs the same workload in a process of its own
against the package of another checkout (the parent commit, with its own built
library):

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/differentiable-ilqr_amd
    python tools/bench_nn_backward.py --parent /tmp/parent --out profiles/nn_mlp_vjp/bench_nn_backward.txt

Per batch and arm: one warm-up, then --runs timed runs (3), arms alternating;
the median, min and max are reported, and the weight gradients of the arms of
one tree are compared.

--hidden H1,H2 takes a two-hidden-layer network (the [64, 64] of the
reference's IL experiment).  Both arms then solve on device
(generic.DEVICE_MLP_DEEP on) and only the backward differs: "device" turns
generic.DEVICE_MLP_DEEP_VJP on (ops.mlp2_linearize_diff), "torch" leaves it off
(the torch graph through grad_input); a tree without that switch has the arm
"torch" alone.  An arm that runs out of memory is reported as such.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STATE, N_CTRL, HIDDEN, T, LQR_ITER = 5, 1, 100, 25, 10


def widths_of(args):
    w = [int(v) for v in str(args.hidden).split(",")]
    if len(w) not in (1, 2) or min(w) < 1:
        sys.exit("bench_nn_backward: --hidden takes H or H1,H2")
    return w


def commit(root):
    try:
        out = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        dirty = subprocess.run(["git", "-C", root, "status", "--porcelain"], capture_output=True, text=True)
        if out.returncode == 0:
            return out.stdout.strip() + ("+changes" if dirty.stdout.strip() else "")
    except OSError:
        pass
    return os.environ.get("DILQR_COMMIT", "unknown")


def worker(args):
    """The workload on the package under args.pkg; one JSON line per batch."""
    sys.path.insert(0, os.path.join(args.pkg, "differentiable-ilqr_amd"))
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_nn_backward: needs a GPU (no CPU timing)")
    import dilqr.mpc as cmpc
    from dilqr import QuadCost, generic
    from dilqr.dynamics import NNDynamics
    print("DEVICE " + f"{torch.cuda.get_device_name(0)}  torch {torch.__version__}", flush=True)
    assert os.path.realpath(generic.__file__).startswith(os.path.realpath(args.pkg)), generic.__file__
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    widths = widths_of(args)
    deep = len(widths) == 2
    dx = NNDynamics(N_STATE, N_CTRL, hidden_sizes=widths, activation="sigmoid").to(dev)
    params = list(dx.parameters())
    # the switch that alternates between the arms
    switch = "DEVICE_MLP_DEEP_VJP" if deep else "DEVICE_MLP_VJP"
    arms = ["device", "torch"] if hasattr(generic, switch) else ["torch"]
    if deep:
        if not hasattr(generic, "DEVICE_MLP_DEEP"):
            sys.exit("bench_nn_backward: this tree has no device model for two hidden layers")
        generic.DEVICE_MLP_DEEP = True              # both arms solve on device
    start = {}
    inner = generic.final_step

    def final_step(*a, **k):
        torch.cuda.reset_peak_memory_stats()
        start["ev"] = torch.cuda.Event(enable_timing=True)
        start["ev"].record()
        return inner(*a, **k)

    generic.final_step = final_step

    def run(B, arm, x0, C, c, wx, wu):
        if len(arms) > 1:
            setattr(generic, switch, arm == "device")
        for p in params:
            p.grad = None
        mpc = cmpc.MPC(N_STATE, N_CTRL, T, lqr_iter=LQR_ITER, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0,
                       u_upper=1.0, n_batch=B, eps=0.0, not_improved_lim=10 ** 9, exit_unconverged=False,
                       detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=10, verbose=-1)
        torch.cuda.synchronize()
        try:
            x, u, _ = mpc(x0, QuadCost(C, c), dx)
            ((x * wx).sum() + (u * wu).sum()).backward()
        except torch.cuda.OutOfMemoryError:
            x = u = None
            for p in params:
                p.grad = None
            torch.cuda.empty_cache()
            return None, None, None
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        torch.cuda.synchronize()
        return start["ev"].elapsed_time(end), torch.cuda.max_memory_allocated() / 2 ** 20, [p.grad.clone() for p in params]

    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(1234)                  # bench_nn_mpc.py's problem
        d = N_STATE + N_CTRL
        L = torch.randn(T, B, d, d, generator=g)
        C = (L @ L.transpose(-1, -2) + 0.5 * torch.eye(d)).to(dev)
        c = torch.randn(T, B, d, generator=g).to(dev)
        x0 = torch.randn(B, N_STATE, generator=g).to(dev)
        wx = torch.randn(T, B, N_STATE, generator=g).to(dev)
        wu = torch.randn(T, B, N_CTRL, generator=g).to(dev)
        del L
        times, mem, grads = {a: [] for a in arms}, {a: [] for a in arms}, {}
        oom = {arm for arm in arms if run(B, arm, x0, C, c, wx, wu)[0] is None}    # the warm-up
        for _ in range(args.runs):
            for arm in arms:
                if arm in oom:
                    continue
                ms, mib, grads[arm] = run(B, arm, x0, C, c, wx, wu)
                if ms is None:
                    oom.add(arm)
                    continue
                times[arm].append(ms)
                mem[arm].append(mib)
        for arm in oom:
            times[arm], mem[arm] = [], []
        rel = None
        if len(arms) > 1 and not oom:
            rel = max(float((a - b).abs().max() / b.abs().max().clamp(min=1.0))
                      for a, b in zip(grads["device"], grads["torch"]))
        print("RESULT " + json.dumps({"B": B, "times": times,
                                      "peak_mib": {a: max(v) if v else None for a, v in mem.items()},
                                      "max_rel_grad_diff": rel}), flush=True)
        del C, c, x0, wx, wu, grads
        torch.cuda.empty_cache()
        if len(arms) > 1:
            (kernel_alone2 if deep else kernel_alone)(B, dx, dev)
    if len(arms) > 1:
        setattr(generic, switch, not deep)          # as shipped
    if deep:
        generic.DEVICE_MLP_DEEP = False


def kernel_alone(B, dx, dev):
    """ops.mlp_linearize_vjp by itself (allocations + the two launches)."""
    import torch
    from dilqr import ops
    md = dx.device_model(torch.zeros(1, device=dev))
    n, m, d, H = N_STATE, N_CTRL, N_STATE + N_CTRL, md.H
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, n, generator=g).to(dev)
    u = torch.randn(T, B, m, generator=g).clamp(-1, 1).to(dev)
    gF = torch.randn(T - 1, B, n, d, generator=g).to(dev)
    gf = torch.randn(T - 1, B, n, generator=g).to(dev)
    for _ in range(3):
        ops.mlp_linearize_vjp(md, x, u, gF, gf)
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.mlp_linearize_vjp(md, x, u, gF, gf)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    rows = (T - 1) * B
    # per row: tau, gF, gf read once from HBM; per hidden unit z (2d), r and q (4nd), p and s (4n), the
    # dW2 column (4n), zh (8), the dW1 row (4d)
    byts, flops = (d + n * d + n) * 4, H * (4 * n * d + 6 * d + 8 * n + 8) + 2 * n * d
    t = statistics.median(ts) * 1e-3
    print("NOTE " + f"# mlp_linearize_vjp B={B}: {rows} rows, call median {t * 1e3:.3f} ms, min {min(ts):.3f}, "
          f"max {max(ts):.3f}; per row {byts} B, {flops} FLOP: {rows * byts / t / 1e12:.3f} TB/s, "
          f"{rows * flops / t / 1e12:.2f} TFLOP/s", flush=True)


def vjp2_flops(n, m, H1, H2):
    """FLOP per row of csrc/tu_mlp2_vjp.hip as built, sigmoid: an
    FMA is 2; LB units per wave, the last block's spare places included (they
    are computed and dropped); an activation as its arithmetic around the
    exp / rcp (4).  Every one of the NB waves of a chunk repeats layer 1, and
    for H1 > 64 each of the ceil(H1 / 64) waves of a block everything but the
    second walk."""
    d = n + m
    C = d + 1
    LB = 4 if n * d <= 30 else 2
    NB = (H2 + LB - 1) // LB
    layer1 = H1 * (2 * d + 4)
    walk = H1 * LB * (2 * d + 3)                                 # z2, w2 g1, P
    derive = LB * (4 + 2 * n + 2 * n * d + 2 * d + 4 + d)        # act, p2, U, s2, zh2, dP
    dw3 = LB * n * (2 * d + 3)
    eg = 128 * LB * C                                            # X^T [a1 | g1] over the chunk's 64 rows
    pass2 = H1 * (LB * (2 * d + 4) + 6)                          # da1, dg1, zh1
    s1 = 128 * C                                                 # zh1^T [tau | 1]
    TT = (H1 + 63) // 64                                         # waves per block: each owns 64 first-layer units
    return NB * (TT * (layer1 + walk + derive + dw3 + eg + s1) + pass2)


def kernel_alone2(B, dx, dev):
    """ops.mlp2_linearize_vjp by itself (allocations + the three launches)."""
    import torch
    from dilqr import ops
    md = dx.device_model(torch.zeros(1, device=dev), deep=True)
    n, m, d = N_STATE, N_CTRL, N_STATE + N_CTRL
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, B, n, generator=g).to(dev)
    u = torch.randn(T, B, m, generator=g).clamp(-1, 1).to(dev)
    gF = torch.randn(T - 1, B, n, d, generator=g).to(dev)
    gf = torch.randn(T - 1, B, n, generator=g).to(dev)
    for _ in range(3):
        ops.mlp2_linearize_vjp(md, x, u, gF, gf)
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.mlp2_linearize_vjp(md, x, u, gF, gf)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    rows = (T - 1) * B
    flops = vjp2_flops(n, m, md.H1, md.H2)
    t = statistics.median(ts) * 1e-3
    print("NOTE " + f"# mlp2_linearize_vjp B={B}: {rows} rows, call median {t * 1e3:.3f} ms, min {min(ts):.3f}, "
          f"max {max(ts):.3f}; per row {flops} FLOP: {rows * flops / t / 1e12:.2f} TFLOP/s", flush=True)


def spawn(pkg, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg", pkg, "--batches", args.batches,
           "--runs", str(args.runs), "--hidden", str(args.hidden)]
    env = {k: v for k, v in os.environ.items() if k != "DILQR_LIB"}         # each tree loads its own library
    out = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if out.returncode != 0:
        sys.exit(f"bench_nn_backward: worker on {pkg} failed\n{out.stdout}\n{out.stderr}")
    device = [line[7:] for line in out.stdout.splitlines() if line.startswith("DEVICE ")][0]
    notes = [line[5:] for line in out.stdout.splitlines() if line.startswith("NOTE ")]
    return device, [json.loads(line[7:]) for line in out.stdout.splitlines() if line.startswith("RESULT ")], notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,4096,65536")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--hidden", default=str(HIDDEN), help="H (one hidden layer, default) or H1,H2 (two)")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--parent-commit", default=None, help="its commit, when it is not a git checkout")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pkg", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # this process never opens the GPU: each tree runs in a child of its own
    trees = [("tree", ROOT, commit(ROOT))]
    if args.parent:
        trees.insert(0, ("parent", args.parent, args.parent_commit or commit(args.parent)))
    rows, notes, device = [], [], ""
    for name, pkg, _ in trees:
        device, results, more = spawn(pkg, args)
        notes += more
        for r in results:
            for arm, t in r["times"].items():
                rel = "-" if r["max_rel_grad_diff"] is None else f"{r['max_rel_grad_diff']:.2e}"
                if not t:
                    rows.append(f"{r['B']:<8d} {name:<7s} {arm:<7s} 0   out of memory")
                    continue
                rows.append(f"{r['B']:<8d} {name:<7s} {arm:<7s} {len(t):<3d} {statistics.median(t):11.3f} {min(t):11.3f} "
                            f"{max(t):11.3f} {r['peak_mib'][arm]:11.1f}   {rel}")
    lines = [f"# bench_nn_backward  commit {trees[-1][2]}" + (f"  parent {trees[0][2]}" if args.parent else ""),
             f"# NNDynamics({N_STATE},{N_CTRL},{widths_of(args)},sigmoid) T={T} lqr_iter={LQR_ITER} fixed-count, u in [-1,1], "
             f"dense SPD cost; mpc.MPC.forward with gradients + backward; device events from the entry of "
             f"final_step to the end of the backward; {args.runs} runs per arm, alternating; ms, MiB",
             f"# {device}",
             "B        tree    arm     n   median_ms      min_ms      max_ms    peak_MiB   max_rel_grad_diff"] + rows + notes
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
