"""GPU checks of the device VJP of the MLP linearisation (csrc/tu_mlp_vjp.hip,
dilqr_mlp_linearize_vjp_f32): the gradient of F = [R S], f = x' - F tau into
W1, b1, W2, b2.

Oracle: the fp64 CPU copy of the module, autograd through forward + grad_input
of L = (F . gF).sum() + (f . gf).sum(), on fp32-representable inputs; relu rows
keep every pre-activation clear of 0 (draw_rows, as tests/test_mlp_gpu.py).
Tolerance 1e-4 as relerr with the max(1, .) normaliser, the project's bound
for F, f and Jacobians: the same sum by fp32 torch autograd sits at 5.5e-7 of
the fp64 oracle, so 1e-4 leaves room for __expf / v_rcp_f32 and another
summation order and for nothing else.  Every measured error is printed
(profiles/nn_mlp_vjp/parity_errors.txt keeps a copy)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
NAMES = ("dW1", "db1", "dW2", "db2")


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


def make_models(n, m, H, act, pt, seed):
    """The same network twice: fp32 on the GPU (whose storage the kernels
    read), and its fp64 copy on the CPU (the oracle)."""
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(seed)
    dx32 = NNDynamics(n, m, hidden_sizes=[H], activation=act, passthrough=pt)
    return copy.deepcopy(dx32).to(DEV), copy.deepcopy(dx32).double()


def draw_rows(dx64, rows, n, m, relu):
    """Inputs [rows, n], [rows, m] in fp32-representable fp64.  For relu every
    pre-activation stays clear of 0 (|z| > 1e-3 in fp64), so the fp32 gate
    (a > 0) cannot legitimately differ from the oracle's: rows that come too
    close are drawn again."""
    x = torch.randn(rows, n).double()
    u = torch.randn(rows, m).double()
    if relu:
        W, b = dx64.fcs[0].weight.detach(), dx64.fcs[0].bias.detach()
        for _ in range(200):
            z = torch.cat((x, u), 1) @ W.t() + b
            bad = (z.abs() <= 1e-3).any(1)
            if not bool(bad.any()):
                break
            k = int(bad.sum())
            x[bad], u[bad] = torch.randn(k, n).double(), torch.randn(k, m).double()
        z = torch.cat((x, u), 1) @ W.t() + b
        assert float(z.abs().min()) > 1e-3
    return x, u


def oracle(dx64, x, u, gF, gf):
    """(dW1, db1, dW2, db2) in fp64 by autograd through the module."""
    dx64.zero_grad()
    xs, us = x.clone().requires_grad_(True), u.clone().requires_grad_(True)   # grad_input's differentiable branch
    new_x = dx64(xs, us)
    R, S = dx64.grad_input(xs, us)
    F = torch.cat((R, S), 2)
    f = new_x - (F @ torch.cat((xs, us), 1).unsqueeze(-1)).squeeze(-1)
    ((F * gF).sum() + (f * gf).sum()).backward()
    fc1, fc2 = dx64.fcs
    return tuple(p.grad.detach().clone().numpy() for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias))


def case(n, m, H, act, pt, rows, seed):
    """A model pair, `rows` rows as x [2, rows, n], u [2, rows, m] (T = 2: the
    second time step is not read), incoming gradients, and the oracle's result."""
    dxg, dx64 = make_models(n, m, H, act, pt, seed)
    x, u = draw_rows(dx64, rows, n, m, act == "relu")
    gF, gf = torch.randn(rows, n, n + m).float().double(), torch.randn(rows, n).float().double()
    ref = oracle(dx64, x, u, gF, gf)
    md = dxg.device_model(torch.zeros(1, device=DEV))
    assert md is not None and (md.n, md.m, md.H) == (n, m, H)
    xg = torch.stack((x, x)).float().to(DEV)
    ug = torch.stack((u, u)).float().to(DEV)
    return dxg, md, xg, ug, gF.float().to(DEV)[None], gf.float().to(DEV)[None], ref


def check(tag, out, ref):
    errs = {k: relerr(cpu(a), b) for k, a, b in zip(NAMES, out, ref)}
    print(f"\n[mlp vjp {tag}] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    for a, b in zip(out, ref):
        assert tuple(a.shape) == b.shape
    assert max(errs.values()) < TOL, errs


# ------------------------------------------------------------------ 5. kernel vs oracle
@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("H", [1, 33, 100])
@pytest.mark.parametrize("nm", [(5, 1), (4, 2), (2, 1)], ids=["5x1", "4x2", "2x1"])
def test_kernel_against_oracle(nm, H, act, pt):
    """T = 3, B = 65: 130 rows, two full waves and a 2-lane tail."""
    from dilqr import ops
    n, m = nm
    dxg, md, xg, ug, gF, gf, ref = case(n, m, H, act, pt, 130, seed=2000 * n + 200 * m + H)
    T, B = 3, 65
    x = torch.cat((xg[0].view(2, B, n), xg[0, :B].view(1, B, n)))         # the last step is not read
    u = torch.cat((ug[0].view(2, B, m), ug[0, :B].view(1, B, m)))
    out = ops.mlp_linearize_vjp(md, x, u, gF.view(T - 1, B, n, n + m), gf.view(T - 1, B, n))
    check(f"n={n} m={m} H={H} {act} pt={pt} rows=130", out, ref)


# ------------------------------------------------------------------ 6. row-count edges
@pytest.mark.parametrize("rows,max_waves", [(1, 0), (63, 0), (64, 0), (65, 0), (200, 1), (200, 2)])
def test_row_count_edges(rows, max_waves):
    """One lane, one lane short of a wave, a full wave, a wave and a lane; 200
    rows on one group of waves (four chunks, the last partial) and on two."""
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(5, 1, 33, "sigmoid", True, rows, seed=300 + rows + max_waves)
    out = ops.mlp_linearize_vjp(md, xg, ug, gF, gf, max_waves=max_waves)
    check(f"n=5 m=1 H=33 sigmoid rows={rows} max_waves={max_waves}", out, ref)
    again = ops.mlp_linearize_vjp(md, xg, ug, gF, gf, max_waves=max_waves)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


def test_widest_hidden_layer():
    from dilqr import _native as N
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(6, 2, N.MLP_MAX_HIDDEN, "sigmoid", True, 65, seed=62)
    out = ops.mlp_linearize_vjp(md, xg, ug, gF, gf)
    check(f"n=6 m=2 H={N.MLP_MAX_HIDDEN} sigmoid rows=65", out, ref)
    again = ops.mlp_linearize_vjp(md, xg, ug, gF, gf)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


# ------------------------------------------------------------------ 7. NULL = zeros
def test_null_gradient_is_zeros_bit_for_bit():
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, _ = case(5, 1, 33, "sigmoid", True, 130, seed=77)
    for a, b in (((None, gf), (torch.zeros_like(gF), gf)), ((gF, None), (gF, torch.zeros_like(gf)))):
        out, ref = ops.mlp_linearize_vjp(md, xg, ug, *a), ops.mlp_linearize_vjp(md, xg, ug, *b)
        assert all(torch.equal(p, q) for p, q in zip(out, ref))
        assert all(bool(torch.isfinite(p).all()) for p in out) and float(out[0].abs().max()) > 0


# ------------------------------------------------------------------ 8. written, not accumulated
def test_outputs_are_written_not_accumulated():
    """The raw launch into NaN-filled outputs and a NaN-filled workspace."""
    from dilqr import _native as N
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(5, 1, 33, "sigmoid", True, 130, seed=88)
    n, m, H = 5, 1, 33
    res = []
    for _ in range(2):
        out = tuple(torch.full(s, float("nan"), device=DEV) for s in ((H, n + m), (H,), (n, H), (n,)))
        ops.Dynamics(md, n, m).linearize_vjp(xg, ug, gF, gf, *out)
        res.append(out)
    assert all(bool(torch.isfinite(p).all()) for p in res[0])
    assert all(torch.equal(p, q) for p, q in zip(*res))
    check("NaN-prefilled outputs", res[0], ref)
    # the caller's workspace needs no initialisation either
    nbytes = N.lib().dilqr_mlp_linearize_vjp_ws_bytes(n, m, 2, 130, H, 0)
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    out = tuple(torch.full(s, float("nan"), device=DEV) for s in ((H, n + m), (H,), (n, H), (n,)))
    N.call("dilqr_mlp_linearize_vjp_f32", n, m, 2, 130, md.desc, N.ptr(xg), N.ptr(ug), N.ptr(gF), N.ptr(gf),
           *(N.ptr(t) for t in out), 0, N.ptr(ws), nbytes, N.stream(xg.device))
    assert all(torch.equal(p, q) for p, q in zip(out, res[0]))
    # no rows: zeros
    z = ops.mlp_linearize_vjp(md, xg[:1], ug[:1], None, None)
    assert [tuple(t.shape) for t in z] == [(H, n + m), (H,), (n, H), (n,)] and not any(bool(t.any()) for t in z)


# ------------------------------------------------------------------ 9. the autograd Function
def params_of(dx):
    return (dx.fcs[0].weight, dx.fcs[0].bias, dx.fcs[1].weight, dx.fcs[1].bias)


def test_function():
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(5, 1, 33, "sigmoid", True, 130, seed=99)
    ps = params_of(dxg)
    F0, f0 = ops.mlp_linearize(md, xg, ug)
    F, f = ops.mlp_linearize_diff(md, ps, xg, ug)
    assert torch.equal(F, F0) and torch.equal(f, f0) and F.requires_grad and f.requires_grad
    ((F * gF).sum() + (f * gf).sum()).backward()
    once = [p.grad.clone() for p in ps]
    check("Function.backward", once, ref)
    direct = ops.mlp_linearize_vjp(md, xg, ug, gF, gf)
    assert all(torch.equal(a, b) for a, b in zip(once, direct))
    # .backward() accumulates into .grad
    F, f = ops.mlp_linearize_diff(md, ps, xg, ug)
    ((F * gF).sum() + (f * gf).sum()).backward()
    for p, g1 in zip(ps, once):
        assert relerr(cpu(p.grad), 2 * cpu(g1)) < 1e-6
    # only F used: gf arrives as None
    for p in ps:
        p.grad = None
    F, f = ops.mlp_linearize_diff(md, ps, xg, ug)
    (F * gF).sum().backward()
    only_F = ops.mlp_linearize_vjp(md, xg, ug, gF, None)
    assert all(torch.equal(p.grad, g) for p, g in zip(ps, only_F))
    # a frozen parameter gets no gradient, the others the same ones
    for p in ps:
        p.grad = None
    ps[1].requires_grad_(False)
    F, f = ops.mlp_linearize_diff(md, ps, xg, ug)
    ((F * gF).sum() + (f * gf).sum()).backward()
    assert ps[1].grad is None
    assert all(torch.equal(ps[i].grad, once[i]) for i in (0, 2, 3))
    ps[1].requires_grad_(True)
    # an in-place update between forward and backward is refused
    F, f = ops.mlp_linearize_diff(md, ps, xg, ug)
    with torch.no_grad():
        ps[0].add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        ((F * gF).sum() + (f * gf).sum()).backward()
    # parameters that are not the ones the model reads
    with pytest.raises(ValueError, match="four parameters"):
        ops.mlp_linearize_diff(md, [p.clone() for p in ps], xg, ug)


# ------------------------------------------------------------------ 10. end to end
def golden_model(g):
    from dilqr.dynamics import NNDynamics
    dx = NNDynamics(5, 1, hidden_sizes=[32], activation="sigmoid").to(DEV)
    with torch.no_grad():
        for i, fc in enumerate(dx.fcs):
            fc.weight.copy_(gpu(g[f"nn_W{i}"]))
            fc.bias.copy_(gpu(g[f"nn_b{i}"]))
    return dx


def solve_and_backward(g):
    """tests/test_mlp_gpu.py::test_backward_reaches_the_weights' set-up: the
    reference's eight NN problems (T = 10, H = 32: 72 rows), mpc.MPC with
    gradients, then the golden's loss."""
    import dilqr.mpc as cmpc
    from dilqr import QuadCost
    dx = golden_model(g)
    T, B = g["nn_C"].shape[:2]
    X0, C, c = gpu(g["nn_x0"], True), gpu(g["nn_C"], True), gpu(g["nn_c"], True)
    m = cmpc.MPC(5, 1, T, lqr_iter=4, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0, u_upper=1.0, n_batch=B,
                 exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2, max_linesearch_iter=10)
    x, u, costs = m(X0, QuadCost(C, c), dx)
    ((x * gpu(g["nn_wx"])).sum() + (u * gpu(g["nn_wu"])).sum()).backward()
    out = {"dx0": cpu(X0.grad), "dC": cpu(C.grad), "dc": cpu(c.grad)}
    for i, fc in enumerate(dx.fcs):
        out[f"dW{i}"], out[f"db{i}"] = cpu(fc.weight.grad), cpu(fc.bias.grad)
    return out, cpu(x), cpu(u)


def test_end_to_end_on_the_reference_golden(golden, monkeypatch):
    from dilqr import generic
    from dilqr.dynamics import NNDynamics
    g = golden("generic_f32")
    assert generic.DEVICE_MLP is True and generic.DEVICE_MLP_VJP is True

    def boom(self, x, u):
        raise AssertionError("NNDynamics.grad_input called")

    with monkeypatch.context() as mp:
        mp.setattr(NNDynamics, "grad_input", boom)
        dev, xd, ud = solve_and_backward(g)
    errs = {k: relerr(v, g[f"nn_analytic_{k}"]) for k, v in dev.items()}
    print("\n[mlp vjp MPC backward vs reference] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert max(errs.values()) < 5e-3, errs
    # the torch graph on the same solve: only the linearisation's rounding differs
    monkeypatch.setattr(generic, "DEVICE_MLP_VJP", False)
    ref, xt, ut = solve_and_backward(g)
    assert np.array_equal(xd, xt) and np.array_equal(ud, ut)
    errs = {k: relerr(dev[k], ref[k]) for k in ("dW0", "db0", "dW1", "db1")}
    print("[mlp vjp MPC backward, device vs torch graph] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert max(errs.values()) < TOL, errs
