"""GPU checks of the DiLQR implicit backward on a one-hidden-layer network
(csrc/tu_mlp_implicit.hip, ops.mlp_implicit_backward, the dilqr.MPC route of
generic.final_step).

Oracle: tests/mlp_oracle.py implicit_oracle in fp64 at the GPU's own fp32
(x, u) (tests/test_mlp_implicit_cpu.py shows it is the literal restatement and
the derivative of the fixed point).  Bound per output: max(1e-4, 3 x err32) of
the output's largest magnitude, err32 being the error of the same oracle run in
float32 numpy on that case — the `ref_spread` convention of
tests/test_gpu_parity.py.  Every measured error is printed (DESIGN.md section
6b keeps the worst per output: sigmoid 2.4e-5, relu 1.2e-5, against err32 of
4.2e-5 and 2.0e-5).

relu cases: a solve on a relu network ends on the network's kinks, where the
gate of a pre-activation that is zero to rounding decides every output and the
float32 oracle itself is 0.1 to 0.5 off the float64 one (first run on the
device: 4 of 36 relu cases outside the bound with errors of 0.1 to 0.7, others
inside it only because err32 was that large).  off_the_kinks moves those rows
clear of 0, as tests/test_mlp_vjp_gpu.py draws its rows; the cases, the bound
and the reference are unchanged."""
import functools

import numpy as np
import pytest
import torch

from mlp_oracle import MlpOracle, err32, implicit_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("dx_init", "dC", "dc", "dF", "df")
WNAMES = ("dW1", "db1", "dW2", "db2")
T_ = 6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def gpu(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV, requires_grad=grad)


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def f32(v):
    """A box value the fp32 kernels and the fp64 oracle agree on bit for bit."""
    return float(np.float32(v))


def network(n, m, H, act, pt, rng):
    """NNDynamics on the GPU with weights 0.5 N(0,1), its device model and its fp64 oracle copy."""
    from dilqr.dynamics import NNDynamics
    dx = NNDynamics(n, m, hidden_sizes=[H], activation=act, passthrough=pt).to(DEV)
    ws = [0.5 * rng.randn(H, n + m), 0.5 * rng.randn(H), 0.5 * rng.randn(n, H), 0.5 * rng.randn(n)]
    with torch.no_grad():
        for p, w in zip((dx.fcs[0].weight, dx.fcs[0].bias, dx.fcs[1].weight, dx.fcs[1].bias), ws):
            p.copy_(gpu(w))
    md = dx.device_model(torch.zeros(1, device=DEV))
    assert md is not None and (md.n, md.m, md.H) == (n, m, H)
    model = MlpOracle(*(cpu(t) for t in md.tensors), act, pt)
    return dx, md, model


def costs(n, m, T, B, rng):
    d = n + m
    L = rng.randn(T, B, d, d)
    return L @ np.swapaxes(L, 2, 3) + np.eye(d), 0.3 * rng.randn(T, B, d)


def off_the_kinks(model, x, u, lo, hi, rng):
    """relu only.  A solve on a relu network ends ON the network's kinks: the
    cost is piecewise quadratic and the iteration chatters across a kink until
    a pre-activation is zero to rounding (fp64 oracle solver on these inputs:
    43 to 61 of 65 problems end with some |z_j| < 1e-4, most below 1e-6).
    There the gate (a > 0) and with it F and every output is decided by the
    rounding of z: the float32 oracle is 0.1 to 0.5 off the float64 one, and so
    is any device.  So, as tests/test_mlp_vjp_gpu.py draw_rows does, every row
    the backward linearises (t < T-1) is kept clear of 0: a row with a
    pre-activation within 1e-3 of it gets its state and its free controls
    (never one on a bound: the active set stays) moved by 1e-2 N(0,1), drawn
    again until clear.  The backward needs no fixed point; the result is still
    fp32-representable."""
    T, B, n = x.shape
    x, u = x.copy(), u.copy()
    free = np.ones_like(u, bool) if hi is None else ~(np.abs(np.abs(u) - hi) <= 1e-8)

    def near(xx, uu):
        z = np.concatenate([xx, uu], -1)[:-1] @ model.W1.T + model.b1
        return np.concatenate([(np.abs(z) <= 1e-3).any(-1), np.zeros((1, B), bool)])

    x0, u0 = x.copy(), u.copy()
    for _ in range(200):
        bad = near(x, u)
        if not bad.any():
            break
        k = int(bad.sum())
        x[bad] = (x0[bad] + 1e-2 * rng.randn(k, n)).astype(np.float32)
        u[bad] = np.where(free[bad], (u0[bad] + 1e-2 * rng.randn(k, u.shape[2])).astype(np.float32), u0[bad])
        if hi is not None:
            u[bad] = np.where(free[bad], np.clip(u[bad], -0.99 * hi, 0.99 * hi).astype(np.float32), u[bad])
    assert not near(x, u).any()
    return x, u


@functools.lru_cache(maxsize=None)
def solved_case(n, m, H, act, pt, B, box, T=T_):
    """A converged device solve (ops.mpc_solve_unfused) on dense SPD costs, loss
    gradients, and the fp64 oracle's outputs with the float32 oracle's errors.
    box: the median magnitude of the free solve's controls, so that about half
    of them end on a bound."""
    from dilqr import ops
    rng = np.random.RandomState(1000 * n + 100 * m + H + 7 * B + (act == "relu") + 2 * pt)
    dx, md, model = network(n, m, H, act, pt, rng)
    C, c = costs(n, m, T, B, rng)
    x0 = 0.5 * rng.randn(B, n)
    wx, wu = rng.randn(T, B, n), rng.randn(T, B, m)
    Cg, cg, x0g = gpu(C), gpu(c), gpu(x0)
    kw = dict(lqr_iter=40, eps=1e-7, not_improved_lim=5, best_cost_eps=1e-4)
    sv = ops.mpc_solve_unfused(md, None, x0g, Cg, cg, T, **kw)
    lo = hi = None
    if box:
        hi = f32(np.median(np.abs(cpu(sv.best_u))))
        lo = -hi
        sv = ops.mpc_solve_unfused(md, None, x0g, Cg, cg, T, u_lower=lo, u_upper=hi, **kw)
    x, u = sv.best_x.clone(), sv.best_u.clone()
    if act == "relu":
        x, u = (gpu(a) for a in off_the_kinks(model, cpu(x), cpu(u), lo, hi, rng))
    C32, c32, wx32, wu32 = cpu(Cg), cpu(cg), cpu(gpu(wx)), cpu(gpu(wu))
    ref, e32 = err32(model, wx32, wu32, C32, c32, cpu(x), cpu(u), lo, hi)
    return dict(dx=dx, md=md, model=model, C=Cg, c=cg, x=x, u=u, wx=gpu(wx), wu=gpu(wu), lo=lo, hi=hi, ref=ref,
                e32=e32, n=n, m=m, T=T, B=B)


def check(tag, out, ref, e32, names=NAMES):
    errs, bounds = {}, {}
    for k, a, b, e in zip(names, out, ref, e32):
        a = cpu(a)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.isfinite(a).all(), k
        errs[k] = float(np.abs(a - b).max() / np.abs(b).max()) if b.size else 0.0
        bounds[k] = max(1e-4, 3 * e)
    print(f"\n[mlp implicit {tag}] " + ", ".join(f"{k} {errs[k]:.1e} (err32 {e:.1e})" for k, e in zip(names, e32)))
    bad = {k: (errs[k], bounds[k]) for k in errs if not errs[k] <= bounds[k]}
    assert not bad, bad


def run(cs, want_dF=True):
    from dilqr import ops
    return ops.mlp_implicit_backward(cs["md"], cs["wx"], cs["wu"], cs["C"], cs["c"], cs["x"], cs["u"], cs["lo"],
                                     cs["hi"], want_dF=want_dF)


# ------------------------------------------------------------------ 1. kernel vs oracle
@pytest.mark.parametrize("box", [False, True], ids=["free", "box"])
@pytest.mark.parametrize("B", [3, 65, 130])
@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("nmH", [(2, 1, 5), (5, 1, 32), (6, 2, 7)], ids=["2x1H5", "5x1H32", "6x2H7"])
def test_kernel_against_oracle(nmH, act, pt, B, box):
    """H = 5 is no multiple of the walk's unroll of 4; (6, 2) is the largest
    shape, with two controls to mask; B = 3, 65, 130: a tail wave, a wave and a
    lane, two waves and a tail."""
    n, m, H = nmH
    cs = solved_case(n, m, H, act, pt, B, box)
    if box:
        active = np.abs(np.abs(cpu(cs["u"])) - cs["hi"]) <= 1e-8
        assert 0 < active.sum() < active.size, (active.sum(), active.size)
    check(f"n={n} m={m} H={H} {act} pt={pt} B={B} {'box' if box else 'free'}", run(cs), cs["ref"], cs["e32"])


# ------------------------------------------------------------------ 2. short horizons
@pytest.mark.parametrize("T", [1, 2, 3])
def test_short_horizons(T):
    """(x, u) need not be a solution: controls drawn and clamped into the box
    (about a third on a bound), states rolled out on the network."""
    from dilqr import ops
    n, m, H, B = 5, 1, 32, 65
    rng = np.random.RandomState(40 + T)
    dx, md, model = network(n, m, H, "sigmoid", True, rng)
    C, c = costs(n, m, T, B, rng)
    hi = f32(0.5)
    u = gpu(np.clip(0.5 * rng.randn(T, B, m), -hi, hi))
    x0 = gpu(0.5 * rng.randn(B, n))
    x = ops.mlp_rollout(md, x0, u) if T > 1 else x0[None].clone()
    wx, wu = gpu(rng.randn(T, B, n)), gpu(rng.randn(T, B, m))
    active = np.abs(np.abs(cpu(u)) - hi) <= 1e-8
    assert 0 < active.sum() < active.size
    Cg, cg = gpu(C), gpu(c)
    out = ops.mlp_implicit_backward(md, wx, wu, Cg, cg, x, u, -hi, hi)
    ref, e32 = err32(model, cpu(wx), cpu(wu), cpu(Cg), cpu(cg), cpu(x), cpu(u), -hi, hi)
    assert tuple(out[3].shape) == (T - 1, B, n, n + m) and tuple(out[4].shape) == (T - 1, B, n)
    check(f"T={T} n=5 m=1 H=32 B=65 box", out, ref, e32)
    if T == 1:
        # y_x = 0, y_u = g_u / C_uu on the free controls: a division and a few
        # products in fp32, far inside 1e-5
        C64, gx, gu, tau = cpu(Cg)[0], cpu(wx)[0], cpu(wu)[0], np.concatenate([cpu(x)[0], cpu(u)[0]], 1)
        y = np.zeros((B, n + m))
        y[:, n] = np.where(active[0, :, 0], 0.0, gu[:, 0] / C64[:, n, n])
        closed = (gx - C64[:, :n, n] * y[:, n:], -0.5 * (y[:, :, None] * tau[:, None] + tau[:, :, None] * y[:, None]),
                  -y)
        for k, a, b in zip(NAMES, out, closed):
            assert np.abs(cpu(a).reshape(b.shape) - b).max() <= 1e-5 * np.abs(b).max(), k


# ------------------------------------------------------------------ 3. slice invariance
def test_slice_invariance():
    """Problems 60..69 of B = 130 alone give the bits they give inside the batch."""
    from dilqr import ops
    cs = solved_case(5, 1, 32, "sigmoid", True, 130, True)
    full = run(cs)
    s = slice(60, 70)
    part = ops.mlp_implicit_backward(cs["md"], *(cs[k][:, s].contiguous() for k in ("wx", "wu", "C", "c", "x", "u")),
                                     cs["lo"], cs["hi"])
    assert torch.equal(part[0], full[0][s])
    for a, b in zip(part[1:], full[1:]):
        assert torch.equal(a, b[:, s])
    again = run(cs)
    assert all(torch.equal(a, b) for a, b in zip(full, again))


# ------------------------------------------------------------------ 4..6: through the MPC modules
def mpc_problem(act, hidden=(32,), seed=5):
    from dilqr.dynamics import NNDynamics
    n, m, T, B = 5, 1, T_, 8
    rng = np.random.RandomState(seed)
    if len(hidden) == 1:
        dx, md, model = network(n, m, hidden[0], act, True, rng)
    else:
        torch.manual_seed(seed)
        dx, model = NNDynamics(n, m, hidden_sizes=list(hidden), activation=act).to(DEV), None
    C, c = costs(n, m, T, B, rng)
    return dict(dx=dx, model=model, C=C, c=c, x0=0.5 * rng.randn(B, n), wx=rng.randn(T, B, n),
                wu=rng.randn(T, B, m), n=n, m=m, T=T, B=B)


def mpc_backward(p, module, weights=True, **kw):
    """Solve and backpropagate sum(wx x) + sum(wu u) through `module`.MPC;
    returns the gradients by name and the solution."""
    import dilqr
    dx = p["dx"]
    for q in dx.parameters():
        q.grad = None
        q.requires_grad_(weights)
    X0, C, c = gpu(p["x0"], True), gpu(p["C"], True), gpu(p["c"], True)
    opts = dict(u_lower=-1.0, u_upper=1.0, lqr_iter=20, n_batch=p["B"], exit_unconverged=False,
                detach_unconverged=False)
    opts.update(kw)
    mpc = module.MPC(p["n"], p["m"], p["T"], **opts)
    x, u, _ = mpc(X0, dilqr.QuadCost(C, c), dx)
    ((x * gpu(p["wx"])).sum() + (u * gpu(p["wu"])).sum()).backward()
    out = {"dx_init": X0.grad, "dC": C.grad, "dc": c.grad}
    if weights:
        fc1, fc2 = dx.fcs
        out.update(dW1=fc1.weight.grad, db1=fc1.bias.grad, dW2=fc2.weight.grad, db2=fc2.bias.grad)
    return out, x.detach(), u.detach(), (X0, C, c)


def oracle_chain(p, x, u, lo=-1.0, hi=1.0):
    """fp64 (dx_init, dC, dc, dW1, db1, dW2, db2) at the GPU's (x, u), and the float32 oracle's errors."""
    g32 = lambda a: cpu(gpu(a))                                   # noqa: E731
    ref, e32 = err32(p["model"], g32(p["wx"]), g32(p["wu"]), g32(p["C"]), g32(p["c"]), cpu(x), cpu(u), lo, hi,
                     extra=lambda md, xx, uu, o: md.param_vjp(xx, uu, o[3], o[4]))
    keep = (0, 1, 2, 5, 6, 7, 8)
    return [ref[i] for i in keep], [e32[i] for i in keep]


ALL = ("dx_init", "dC", "dc") + WNAMES


def test_relu_consistency_with_the_classic_adjoint():
    """relu: M = 0, so dilqr.MPC's gradients are dilqr.mpc.MPC's; two kernels
    compute the same sums, within 3 x the classic path's own error against the
    fp64 oracle."""
    import dilqr
    import dilqr.mpc as cmpc
    p = mpc_problem("relu")
    imp, x, u, _ = mpc_backward(p, dilqr)
    imp = {k: v.clone() for k, v in imp.items()}
    cla, xc, uc, _ = mpc_backward(p, cmpc)
    assert torch.equal(x, xc) and torch.equal(u, uc)
    ref, _ = oracle_chain(p, x, u)
    for k, r in zip(ALL, ref):
        e_cla = np.abs(cpu(cla[k]) - r).max()
        diff = np.abs(cpu(imp[k]) - cpu(cla[k])).max()
        print(f"\n[mlp implicit relu vs classic] {k}: |implicit - classic| {diff:.2e}, classic error {e_cla:.2e} "
              f"(scale {np.abs(r).max():.2e})")
        assert diff <= 3 * e_cla, (k, diff, e_cla)


def test_end_to_end(monkeypatch):
    import dilqr
    from dilqr import generic
    from dilqr.dynamics import NNDynamics
    p = mpc_problem("sigmoid")
    assert generic.DEVICE_MLP_IMPLICIT is True

    def boom(self, *a):
        raise AssertionError("NNDynamics.grad_input / forward called")

    with monkeypatch.context() as mp:
        mp.setattr(NNDynamics, "grad_input", boom)
        mp.setattr(NNDynamics, "forward", boom)
        out, x, u, _ = mpc_backward(p, dilqr)
    ref, e32 = oracle_chain(p, x, u)
    check("dilqr.MPC end to end, n=5 m=1 H=32 sigmoid T=6 B=8 box 1", [out[k] for k in ALL], ref, e32, names=ALL)
    # outside the switch or the envelope: the refusal final_step has always given
    refusal = "needs an env_dx model"
    with monkeypatch.context() as mp:
        mp.setattr(generic, "DEVICE_MLP_IMPLICIT", False)
        with pytest.raises(NotImplementedError, match=refusal):
            mpc_backward(p, dilqr)
    with pytest.raises(NotImplementedError, match=refusal):
        mpc_backward(mpc_problem("sigmoid", hidden=(16, 16)), dilqr)
    with pytest.raises(NotImplementedError, match=refusal):
        mpc_backward(p, dilqr, delta_u=0.5)
    with pytest.raises(NotImplementedError, match="slew-rate"):
        mpc_backward(p, dilqr, slew_rate_penalty=0.1)


def test_no_wasted_work(monkeypatch):
    """Only C and c want a gradient: no dF, df, no VJP launch, the same dC, dc."""
    import dilqr
    from dilqr import ops
    p = mpc_problem("sigmoid")
    seen = []
    real = ops.mlp_implicit_backward

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw.get("want_dF", True), out))
        return out

    def boom(*a, **kw):
        raise AssertionError("a weight-gradient launch")

    monkeypatch.setattr(ops, "mlp_implicit_backward", spy)
    monkeypatch.setattr(ops, "mlp_linearize_vjp", boom)
    out, x, u, (X0, C, c) = mpc_backward(p, dilqr, weights=False)
    assert len(seen) == 1 and not seen[0][0] and seen[0][1][3] is None and seen[0][1][4] is None
    md = p["dx"].device_model(x)
    full = real(md, gpu(p["wx"]), gpu(p["wu"]), C.detach(), c.detach(), x, u, -1.0, 1.0, want_dF=True)
    assert full[3] is not None and full[4] is not None
    for k, a in zip(("dx_init", "dC", "dc"), full):
        assert torch.equal(out[k], a), k
    ref, e32 = oracle_chain(p, x, u)
    check("C, c only", [out[k] for k in ("dx_init", "dC", "dc")], ref[:3], e32[:3], names=NAMES[:3])
