"""GPU checks of the device VJP of the two-hidden-layer MLP linearisation
(csrc/tu_mlp2_vjp.hip, dilqr_mlp2_linearize_vjp_f32): the gradient of
F = [R S], f = x' - F tau into W1, b1, W2, b2, W3, b3.

Oracle: the fp64 CPU copy of the module, autograd through forward + grad_input
of L = (F . gF).sum() + (f . gf).sum(), on fp32-representable inputs; relu rows
keep every pre-activation of both layers clear of 0 (draw_rows, as
tests/test_mlp2_gpu.py).  Tolerance 1e-4 as relerr with the max(1, .)
normaliser, the project's bound for F, f, Jacobians and the one-layer VJP: the
same sum by fp32 torch autograd stays within 1.0e-6 of the fp64 oracle over
these shapes, so 1e-4 leaves room for __expf / v_rcp_f32 and another summation
order and for nothing else.  Every measured error is printed
(profiles/nn_mlp2_vjp/parity_errors.txt keeps a copy)."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
NAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3")


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


def pre_activations(dx64, x, u):
    """Every hidden pre-activation of a row, both layers, in fp64: [rows, H1 + H2]."""
    z, out = torch.cat((x, u), 1), []
    for fc in dx64.fcs[:-1]:
        z = z @ fc.weight.detach().t() + fc.bias.detach()
        out.append(z)
        z = torch.relu(z) if dx64.activation == "relu" else torch.sigmoid(z)
    return torch.cat(out, 1)


def draw_rows(dx64, rows, n, m, relu):
    """Inputs [rows, n], [rows, m] in fp32-representable fp64.  For relu every
    pre-activation of both layers stays clear of 0 (|z| > 1e-3 in fp64), so the
    fp32 gate (a > 0) cannot legitimately differ from the oracle's: rows that
    come too close are drawn again, 200 rounds at the most."""
    x = torch.randn(rows, n).double()
    u = torch.randn(rows, m).double()
    if relu:
        for _ in range(200):
            bad = (pre_activations(dx64, x, u).abs() <= 1e-3).any(1)
            if not bool(bad.any()):
                break
            k = int(bad.sum())
            x[bad], u[bad] = torch.randn(k, n).double(), torch.randn(k, m).double()
        assert float(pre_activations(dx64, x, u).abs().min()) > 1e-3
    return x, u


def params_of(dx):
    return tuple(p for fc in dx.fcs for p in (fc.weight, fc.bias))


def oracle(dx64, x, u, gF, gf):
    """(dW1, db1, dW2, db2, dW3, db3) in fp64 by autograd through the module."""
    dx64.zero_grad()
    xs, us = x.clone().requires_grad_(True), u.clone().requires_grad_(True)   # grad_input's differentiable branch
    new_x = dx64(xs, us)
    R, S = dx64.grad_input(xs, us)
    F = torch.cat((R, S), 2)
    f = new_x - (F @ torch.cat((xs, us), 1).unsqueeze(-1)).squeeze(-1)
    ((F * gF).sum() + (f * gf).sum()).backward()
    return tuple(p.grad.detach().clone().numpy() for p in params_of(dx64))


@functools.lru_cache(maxsize=None)
def case(n, m, widths, act, pt, rows, seed):
    """A model pair (fp32 on the GPU, whose storage the kernels read, and its
    fp64 CPU copy), `rows` rows as x [2, rows, n], u [2, rows, m] (T = 2: the
    second time step is not read), incoming gradients, and the oracle's result.
    Computed once per case and shared; nothing in it is changed by a test that
    shares it."""
    from dilqr.dynamics import NNDynamics
    torch.manual_seed(seed)
    dx32 = NNDynamics(n, m, hidden_sizes=list(widths), activation=act, passthrough=pt)
    dxg, dx64 = copy.deepcopy(dx32).to(DEV), copy.deepcopy(dx32).double()
    x, u = draw_rows(dx64, rows, n, m, act == "relu")
    gF, gf = torch.randn(rows, n, n + m).float().double(), torch.randn(rows, n).float().double()
    ref = oracle(dx64, x, u, gF, gf)
    md = dxg.device_model(torch.zeros(1, device=DEV), deep=True)
    assert md is not None and (md.n, md.m, md.H1, md.H2) == (n, m) + tuple(widths) and md.vjp_ok
    xg = torch.stack((x, x)).float().to(DEV)
    ug = torch.stack((u, u)).float().to(DEV)
    return dxg, md, xg, ug, gF.float().to(DEV)[None], gf.float().to(DEV)[None], ref


def check(tag, out, ref):
    errs = {k: relerr(cpu(a), b) for k, a, b in zip(NAMES, out, ref)}
    print(f"\n[mlp2 vjp {tag}] " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert len(out) == len(ref) == 6
    for a, b in zip(out, ref):
        assert tuple(a.shape) == b.shape
    assert max(errs.values()) < TOL, errs


def as_t3(n, m, xg, ug, gF, gf):
    """130 rows as T = 3, B = 65 (the last step is not read)."""
    T, B = 3, 65
    x = torch.cat((xg[0].view(2, B, n), xg[0, :B].view(1, B, n)))
    u = torch.cat((ug[0].view(2, B, m), ug[0, :B].view(1, B, m)))
    return x, u, gF.view(T - 1, B, n, n + m), gf.view(T - 1, B, n)


# ------------------------------------------------------------------ 5. kernel vs oracle
WIDTHS = [(1, 1), (33, 7), (7, 33), (64, 64)]


@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("widths", WIDTHS, ids=[f"{a}-{b}" for a, b in WIDTHS])
@pytest.mark.parametrize("nm", [(5, 1), (4, 2), (2, 1)], ids=["5x1", "4x2", "2x1"])
def test_kernel_against_oracle(nm, widths, act, pt):
    """T = 3, B = 65: 130 rows, two full waves and a 2-lane tail.  A single
    unit per layer, H2 not a multiple of the unit block, H1 not filling the
    transposed lanes, and the IL shape."""
    from dilqr import ops
    n, m = nm
    dxg, md, xg, ug, gF, gf, ref = case(n, m, widths, act, pt, 130, 2000 * n + 200 * m + 3 * widths[0] + widths[1])
    out = ops.mlp2_linearize_vjp(md, *as_t3(n, m, xg, ug, gF, gf))
    check(f"n={n} m={m} widths={widths} {act} pt={pt} rows=130", out, ref)


def test_widest_row():
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(6, 2, (64, 64), "sigmoid", True, 130, 6264)
    out = ops.mlp2_linearize_vjp(md, *as_t3(6, 2, xg, ug, gF, gf))
    check("n=6 m=2 widths=(64, 64) sigmoid rows=130", out, ref)


# ------------------------------------------------------------------ 6. H1 above one lane tile and at the cap
def test_first_width_at_the_cap():
    """(cap, 3); (65, 5) when the cap is above one lane tile of 64."""
    from dilqr import _native as N
    from dilqr import ops
    cap = N.MLP2_VJP_MAX_HIDDEN1
    for widths in ([(65, 5)] if cap > 64 else []) + [(cap, 3)]:
        dxg, md, xg, ug, gF, gf, ref = case(5, 1, widths, "sigmoid", True, 65, 650 + widths[0])
        out = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf)
        check(f"n=5 m=1 widths={widths} sigmoid rows=65", out, ref)
        again = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf)
        assert all(torch.equal(a, b) for a, b in zip(out, again))


# ------------------------------------------------------------------ 7. widest H2
def test_widest_second_layer():
    from dilqr import _native as N
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(6, 2, (7, N.MLP_MAX_HIDDEN), "sigmoid", True, 65, 62)
    out = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf)
    check(f"n=6 m=2 widths=(7, {N.MLP_MAX_HIDDEN}) sigmoid rows=65", out, ref)
    again = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


# ------------------------------------------------------------------ 8. row-count edges
@pytest.mark.parametrize("rows,max_waves", [(1, 0), (63, 0), (64, 0), (65, 0), (200, 1), (200, 2)])
def test_row_count_edges(rows, max_waves):
    """One lane, one lane short of a wave, a full wave, a wave and a lane; 200
    rows on one group of waves (four chunks, the last partial) and on two."""
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(5, 1, (33, 7), "sigmoid", True, rows, 300 + rows)
    out = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf, max_waves=max_waves)
    check(f"n=5 m=1 widths=(33, 7) sigmoid rows={rows} max_waves={max_waves}", out, ref)
    again = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf, max_waves=max_waves)
    assert all(torch.equal(a, b) for a, b in zip(out, again))


# ------------------------------------------------------------------ 9. NULL = zeros
def test_null_gradient_is_zeros_bit_for_bit():
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, _ = case(5, 1, (33, 7), "sigmoid", True, 130, 77)
    for a, b in (((None, gf), (torch.zeros_like(gF), gf)), ((gF, None), (gF, torch.zeros_like(gf)))):
        out, ref = ops.mlp2_linearize_vjp(md, xg, ug, *a), ops.mlp2_linearize_vjp(md, xg, ug, *b)
        assert all(torch.equal(p, q) for p, q in zip(out, ref))
        assert all(bool(torch.isfinite(p).all()) for p in out)
        assert all(float(p.abs().max()) > 0 for p in (out[0], out[2], out[4]))


# ------------------------------------------------------------------ 10. written, not accumulated
def test_outputs_are_written_not_accumulated():
    """The raw launch into NaN-filled outputs and a NaN-filled workspace."""
    from dilqr import _native as N
    from dilqr import ops
    n, m, widths = 5, 1, (33, 7)
    dxg, md, xg, ug, gF, gf, ref = case(n, m, widths, "sigmoid", True, 130, 88)
    shapes = [tuple(t.shape) for t in md.tensors]
    wrapped = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf)
    nbytes = N.lib().dilqr_mlp2_linearize_vjp_ws_bytes(n, m, 2, 130, widths[0], widths[1], 0)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    out = tuple(torch.full(s, float("nan"), device=DEV) for s in shapes)
    N.call("dilqr_mlp2_linearize_vjp_f32", n, m, 2, 130, md.desc, N.ptr(xg), N.ptr(ug), N.ptr(gF), N.ptr(gf),
           *(N.ptr(t) for t in out), 0, N.ptr(ws), nbytes, N.stream(xg.device))
    assert all(bool(torch.isfinite(p).all()) for p in out)
    assert all(torch.equal(p, q) for p, q in zip(out, wrapped))
    check("NaN-prefilled outputs and workspace", out, ref)
    # no rows: zeros
    z = ops.mlp2_linearize_vjp(md, xg[:1], ug[:1], None, None)
    assert [tuple(t.shape) for t in z] == shapes and not any(bool(t.any()) for t in z)


# ------------------------------------------------------------------ 11. the autograd Function
def test_function():
    from dilqr import ops
    dxg, md, xg, ug, gF, gf, ref = case(5, 1, (33, 7), "sigmoid", True, 130, 99)
    dxg = copy.deepcopy(dxg)                       # this test updates a parameter: its own module and model
    md = dxg.device_model(torch.zeros(1, device=DEV), deep=True)
    ps = params_of(dxg)
    F0, f0 = ops.mlp_linearize(md, xg, ug)
    F, f = ops.mlp2_linearize_diff(md, ps, xg, ug)
    assert torch.equal(F, F0) and torch.equal(f, f0) and F.requires_grad and f.requires_grad
    ((F * gF).sum() + (f * gf).sum()).backward()
    once = [p.grad.clone() for p in ps]
    check("Function.backward", once, ref)
    direct = ops.mlp2_linearize_vjp(md, xg, ug, gF, gf)
    assert all(torch.equal(a, b) for a, b in zip(once, direct))
    # .backward() accumulates into .grad
    F, f = ops.mlp2_linearize_diff(md, ps, xg, ug)
    ((F * gF).sum() + (f * gf).sum()).backward()
    for p, g1 in zip(ps, once):
        assert relerr(cpu(p.grad), 2 * cpu(g1)) < 1e-6
    # only F, or only f, used: the other gradient arrives as None
    for use_F in (True, False):
        for p in ps:
            p.grad = None
        F, f = ops.mlp2_linearize_diff(md, ps, xg, ug)
        ((F * gF).sum() if use_F else (f * gf).sum()).backward()
        only = ops.mlp2_linearize_vjp(md, xg, ug, gF if use_F else None, None if use_F else gf)
        assert all(torch.equal(p.grad, g) for p, g in zip(ps, only))
    # x and u get no gradient
    xr, ur = xg.clone().requires_grad_(True), ug.clone().requires_grad_(True)
    F, f = ops.mlp2_linearize_diff(md, ps, xr, ur)
    (F * gF).sum().backward()
    assert xr.grad is None and ur.grad is None
    # an in-place update between forward and backward is refused
    F, f = ops.mlp2_linearize_diff(md, ps, xg, ug)
    with torch.no_grad():
        ps[2].add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        ((F * gF).sum() + (f * gf).sum()).backward()


# ------------------------------------------------------------------ 12. end to end
B65 = 65


def test_end_to_end_against_the_torch_graph(golden, monkeypatch):
    """tests/test_mlp2_gpu.py::test_backward_reaches_the_weights' workload (the
    reference's eight NN problems tiled to 65, [32, 32]): mpc.MPC forward +
    backward with every switch on against the same tree with only
    DEVICE_MLP_DEEP_VJP off (the torch graph through grad_input)."""
    import dilqr.mpc as cmpc
    from dilqr import QuadCost, generic, ops
    from dilqr.dynamics import NNDynamics
    g = golden("generic_f32")
    idx = np.arange(B65) % 8
    T = g["nn_C"].shape[0]
    wx, wu = gpu(g["nn_wx"][:, idx]), gpu(g["nn_wu"][:, idx])
    calls = {"vjp": 0, "grad_input_diff": 0}
    vjp, grad_input = ops.mlp2_linearize_vjp, NNDynamics.grad_input

    def spy_vjp(*a, **k):
        calls["vjp"] += 1
        return vjp(*a, **k)

    def spy_grad_input(self, x, u):
        calls["grad_input_diff"] += int(x.requires_grad or u.requires_grad)
        return grad_input(self, x, u)

    monkeypatch.setattr(ops, "mlp2_linearize_vjp", spy_vjp)
    monkeypatch.setattr(NNDynamics, "grad_input", spy_grad_input)

    def run():
        torch.manual_seed(2024)
        dx = NNDynamics(5, 1, hidden_sizes=[32, 32]).to(DEV)
        X0, C, c = gpu(g["nn_x0"][idx], True), gpu(g["nn_C"][:, idx], True), gpu(g["nn_c"][:, idx], True)
        mpc = cmpc.MPC(5, 1, T, lqr_iter=4, grad_method=cmpc.GradMethods.ANALYTIC, u_lower=-1.0, u_upper=1.0,
                       n_batch=B65, exit_unconverged=False, detach_unconverged=False, linesearch_decay=0.2,
                       max_linesearch_iter=10)
        x, u, costs = mpc(X0, QuadCost(C, c), dx)
        ((x * wx).sum() + (u * wu).sum()).backward()
        out = {"dx0": X0.grad, "dC": C.grad, "dc": c.grad}
        for i, fc in enumerate(dx.fcs):
            out[f"dW{i}"], out[f"db{i}"] = fc.weight.grad, fc.bias.grad
        assert all(v is not None for v in out.values())
        return {k: cpu(v) for k, v in out.items()}, cpu(x), cpu(u)

    assert generic.DEVICE_MLP is True and generic.DEVICE_MLP_VJP is True and generic.DEVICE_MLP_DEEP_VJP is False
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP", True)
    ref, xt, ut = run()
    torch_graph_calls = calls["grad_input_diff"]
    assert calls["vjp"] == 0 and torch_graph_calls >= 1
    monkeypatch.setattr(generic, "DEVICE_MLP_DEEP_VJP", True)
    got, xd, ud = run()
    # the device VJP ran, and grad_input was not called in differentiable mode again
    assert calls == {"vjp": 1, "grad_input_diff": torch_graph_calls}
    fwd = max(relerr(xd, xt), relerr(ud, ut))
    errs = {k: relerr(got[k], ref[k]) for k in ref}
    print(f"\n[mlp2 vjp MPC, device VJP vs torch graph] forward {fwd:.2e}; "
          + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
    assert len(errs) == 9 and max(errs.values()) < 5e-3, errs
    assert fwd < 5e-3
