"""GPU checks of the DiLQR implicit backward on a two-hidden-layer network
(csrc/tu_mlp2_implicit.hip, ops.mlp_implicit_backward on an Mlp2Model, the
dilqr.MPC route of generic.final_step behind DEVICE_MLP_DEEP_IMPLICIT).  The
structure and the helpers are those of tests/test_mlp_implicit_gpu.py.

Oracle: tests/mlp_oracle.py implicit_oracle on tests/mlp2_oracle.py Mlp2Oracle
in fp64 at the GPU's own fp32 (x, u) (tests/test_mlp2_implicit_cpu.py shows it
is the derivative of the fixed point).  Bound per output: max(1e-4, 3 x err32)
of the output's largest magnitude, err32 being the error of the same oracle run
in float32 numpy on that case; and err32 <= 1e-4 is asserted on every case, so
the bound never exceeds 3e-4 (a missing term of M moves the outputs by 1e-3 to
9e-1).  Every measured error is printed (DESIGN.md section 6b keeps the worst
per output).

relu cases: as in tests/test_mlp_implicit_gpu.py a solve on a relu network ends
on the network's kinks, so every row the backward linearises is moved clear of
the kinks of both layers (|z1_j|, |z2_l| > 1e-3); the backward needs no fixed
point."""
import functools

import numpy as np
import pytest
import torch

from mlp2_oracle import Mlp2Oracle, extra_weights
from mlp_oracle import err32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("dx_init", "dC", "dc", "dF", "df")
WNAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3")
ALL = ("dx_init", "dC", "dc") + WNAMES
T_ = 6
DEEP = ("DEVICE_MLP_DEEP", "DEVICE_MLP_DEEP_IMPLICIT")
DRAWS = 4


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


def network(n, m, H1, H2, act, pt, rng, fan_in=False):
    """NNDynamics on the GPU with weights 0.5 N(0,1) (fan_in: N(0,1) / sqrt(fan_in)),
    its device model and its fp64 oracle copy."""
    from dilqr import _native as N
    from dilqr.dynamics import NNDynamics
    dx = NNDynamics(n, m, hidden_sizes=[H1, H2], activation=act, passthrough=pt).to(DEV)
    with torch.no_grad():
        for fc in dx.fcs:
            scale = 1 / np.sqrt(fc.weight.shape[1]) if fan_in else 0.5
            for p in (fc.weight, fc.bias):
                p.copy_(gpu(scale * rng.randn(*p.shape)))
    md = dx.device_model(torch.zeros(1, device=DEV), deep=True)
    assert md is not None and (md.n, md.m, md.H1, md.H2) == (n, m, H1, H2)
    assert md.implicit_ok == (H1 <= N.MLP2_IMPLICIT_MAX_HIDDEN1)
    model = Mlp2Oracle(*(cpu(t) for t in md.tensors), act, pt)
    return dx, md, model


def costs(n, m, T, B, rng):
    d = n + m
    L = rng.randn(T, B, d, d)
    return L @ np.swapaxes(L, 2, 3) + np.eye(d), 0.3 * rng.randn(T, B, d)


def off_the_kinks(model, x, u, lo, hi, rng):
    """relu only: tests/test_mlp_implicit_gpu.py off_the_kinks for two layers.
    Every row the backward linearises (t < T-1) with a pre-activation of either
    layer within 1e-3 of 0 gets its state and its free controls (never one on a
    bound: the active set stays) moved by 1e-2 N(0,1), drawn again until clear.
    The result is still fp32-representable."""
    T, B, n = x.shape
    x, u = x.copy(), u.copy()
    free = np.ones_like(u, bool) if hi is None else ~(np.abs(np.abs(u) - hi) <= 1e-8)

    def near(xx, uu):
        (z1, _, _, _), (z2, _, _, _) = model.hidden(np.concatenate([xx, uu], -1)[:-1])
        close = (np.abs(z1) <= 1e-3).any(-1) | (np.abs(z2) <= 1e-3).any(-1)
        return np.concatenate([close, np.zeros((1, B), bool)])

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
def solved_case(n, m, H1, H2, act, pt, B, box, fan_in=False, T=T_):
    """A converged device solve (ops.mpc_solve_unfused on the Mlp2Model) on dense
    SPD costs, loss gradients, and the fp64 oracle's outputs with the float32
    oracle's errors.  box: the median magnitude of the free solve's controls,
    so that about half of them end on a bound.

    The draw is judged before the kernel under test has run, by the reference
    alone: a draw whose float32 oracle is more than 1e-4 off the float64 one
    (with B = 3 a single badly conditioned relu problem does that: first run on
    the device, err32 1.7e-4 on one case), or whose box leaves no control or
    every control on a bound, is drawn again from the next seed, DRAWS times at
    the most; the tests assert both conditions on what is returned."""
    seed = 1000 * n + 100 * m + H1 + 11 * H2 + 7 * B + (act == "relu") + 2 * pt
    for k in range(DRAWS):
        cs = draw_case(seed + 100003 * k, n, m, H1, H2, act, pt, B, box, fan_in, T)
        active = np.abs(np.abs(cpu(cs["u"])) - cs["hi"]) <= 1e-8 if box else None
        if max(cs["e32"]) <= 1e-4 and (not box or 0 < active.sum() < active.size):
            break
    return cs


def draw_case(seed, n, m, H1, H2, act, pt, B, box, fan_in, T):
    from dilqr import ops
    rng = np.random.RandomState(seed)
    dx, md, model = network(n, m, H1, H2, act, pt, rng, fan_in)
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
    print(f"\n[mlp2 implicit {tag}] " + ", ".join(f"{k} {errs[k]:.1e} (err32 {e:.1e})" for k, e in zip(names, e32)))
    loose = {k: e for k, e in zip(names, e32) if not e <= 1e-4}
    assert not loose, ("err32 above 1e-4", loose)
    bad = {k: (errs[k], bounds[k]) for k in errs if not errs[k] <= bounds[k]}
    assert not bad, bad


def run(cs, want_dF=True):
    from dilqr import ops
    return ops.mlp_implicit_backward(cs["md"], cs["wx"], cs["wu"], cs["C"], cs["c"], cs["x"], cs["u"], cs["lo"],
                                     cs["hi"], want_dF=want_dF)


def assert_some_active(cs):
    active = np.abs(np.abs(cpu(cs["u"])) - cs["hi"]) <= 1e-8
    assert 0 < active.sum() < active.size, (active.sum(), active.size)


# ------------------------------------------------------------------ 1. kernel vs oracle
SHAPES = [(2, 1, 5, 3), (5, 1, 33, 9), (6, 2, 7, 12)]


@pytest.mark.parametrize("box", [False, True], ids=["free", "box"])
@pytest.mark.parametrize("B", [3, 65, 130])
@pytest.mark.parametrize("pt", [True, False], ids=["pass", "nopass"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("nmH", SHAPES, ids=["2x1H5-3", "5x1H33-9", "6x2H7-12"])
def test_kernel_against_oracle(nmH, act, pt, B, box):
    """H1 = 5, 33, 7 are no multiples of the first-layer unroll of 8; H2 = 3 and
    9 leave a remainder after blocks of 4, 12 leaves none; (6, 2) is the largest
    d, with two controls to mask; B = 3, 65, 130: a tail wave, a wave and a
    lane, two waves and a tail."""
    n, m, H1, H2 = nmH
    cs = solved_case(n, m, H1, H2, act, pt, B, box)
    if box:
        assert_some_active(cs)
    check(f"n={n} m={m} H=({H1},{H2}) {act} pt={pt} B={B} {'box' if box else 'free'}", run(cs), cs["ref"], cs["e32"])


def test_the_reference_network():
    """NNDynamics(5, 1, [64, 64]), weights N(0,1) / sqrt(fan_in)."""
    cs = solved_case(5, 1, 64, 64, "sigmoid", True, 65, True, fan_in=True)
    assert_some_active(cs)
    check("n=5 m=1 H=(64,64) sigmoid B=65 box", run(cs), cs["ref"], cs["e32"])


def test_first_width_at_the_cap():
    """The LDS budget at its limit, at the largest staging area."""
    from dilqr import _native as N
    cap = N.MLP2_IMPLICIT_MAX_HIDDEN1
    cs = solved_case(6, 2, cap, 5, "sigmoid", True, 65, True, fan_in=True)
    assert_some_active(cs)
    check(f"n=6 m=2 H=({cap},5) sigmoid B=65 box", run(cs), cs["ref"], cs["e32"])


# ------------------------------------------------------------------ 2. short horizons
@pytest.mark.parametrize("T", [1, 2, 3])
def test_short_horizons(T):
    """(x, u) need not be a solution: controls drawn and clamped into the box
    (about a third on a bound), states rolled out on the network."""
    from dilqr import ops
    n, m, H1, H2, B = 5, 1, 33, 9, 65
    rng = np.random.RandomState(40 + T)
    dx, md, model = network(n, m, H1, H2, "sigmoid", True, rng)
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
    check(f"T={T} n=5 m=1 H=(33,9) B=65 box", out, ref, e32)
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


# ------------------------------------------------------------------ 3. slice invariance and determinism
def test_slice_invariance_and_determinism():
    """Problems 60..69 of B = 130 alone give the bits they give inside the batch; a second run gives the same bits."""
    from dilqr import ops
    cs = solved_case(5, 1, 33, 9, "sigmoid", True, 130, True)
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
def mpc_problem(act, hidden=(32, 16), seed=5):
    from dilqr.dynamics import NNDynamics
    n, m, T, B = 5, 1, T_, 8
    rng = np.random.RandomState(seed)
    if len(hidden) == 2:
        dx, md, model = network(n, m, hidden[0], hidden[1], act, True, rng)
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
        grads = [q.grad for fc in dx.fcs for q in (fc.weight, fc.bias)]
        out.update(zip(WNAMES, grads))
    return out, x.detach(), u.detach(), (X0, C, c)


def oracle_chain(p, x, u, lo=-1.0, hi=1.0):
    """fp64 (dx_init, dC, dc, dW1, db1, dW2, db2, dW3, db3) at the GPU's (x, u), and the float32 chain's errors."""
    g32 = lambda a: cpu(gpu(a))                                   # noqa: E731
    ref, e32 = err32(p["model"], g32(p["wx"]), g32(p["wu"]), g32(p["C"]), g32(p["c"]), cpu(x), cpu(u), lo, hi,
                     extra=extra_weights)
    keep = (0, 1, 2, 5, 6, 7, 8, 9, 10)
    return [ref[i] for i in keep], [e32[i] for i in keep]


def switches(mp, vjp):
    from dilqr import generic
    assert generic.DEVICE_MLP is True and generic.DEVICE_MLP_IMPLICIT is True and generic.DEVICE_MLP_VJP is True
    for name in DEEP:
        mp.setattr(generic, name, True)
    mp.setattr(generic, "DEVICE_MLP_DEEP_VJP", vjp)


def test_relu_consistency_with_the_classic_adjoint(monkeypatch):
    """relu: M = 0, so dilqr.MPC's gradients are dilqr.mpc.MPC's; two kernels
    compute the same sums, within 3 x the classic path's own error against the
    fp64 oracle chain."""
    import dilqr
    import dilqr.mpc as cmpc
    switches(monkeypatch, True)
    p = mpc_problem("relu")
    imp, x, u, _ = mpc_backward(p, dilqr)
    imp = {k: v.clone() for k, v in imp.items()}
    cla, xc, uc, _ = mpc_backward(p, cmpc)
    assert torch.equal(x, xc) and torch.equal(u, uc)
    ref, _ = oracle_chain(p, x, u)
    for k, r in zip(ALL, ref):
        e_cla = np.abs(cpu(cla[k]) - r).max()
        diff = np.abs(cpu(imp[k]) - cpu(cla[k])).max()
        print(f"\n[mlp2 implicit relu vs classic] {k}: |implicit - classic| {diff:.2e}, classic error {e_cla:.2e} "
              f"(scale {np.abs(r).max():.2e})")
        assert diff <= 3 * e_cla, (k, diff, e_cla)


def test_end_to_end(monkeypatch):
    import dilqr
    from dilqr import _native as N
    from dilqr import generic
    from dilqr.dynamics import NNDynamics
    p = mpc_problem("sigmoid")
    assert generic.DEVICE_MLP_DEEP_IMPLICIT is False

    def boom(self, *a):
        raise AssertionError("NNDynamics.grad_input / forward called")

    # the device VJP carries dF, df: nothing falls back to torch
    with monkeypatch.context() as mp:
        switches(mp, True)
        mp.setattr(NNDynamics, "grad_input", boom)
        mp.setattr(NNDynamics, "forward", boom)
        out, x, u, _ = mpc_backward(p, dilqr)
    ref, e32 = oracle_chain(p, x, u)
    check("dilqr.MPC end to end (device VJP), n=5 m=1 H=(32,16) sigmoid T=6 B=8 box 1", [out[k] for k in ALL], ref,
          e32, names=ALL)
    # the torch graph through grad_input carries dF, df
    with monkeypatch.context() as mp:
        switches(mp, False)
        out2, x2, u2, _ = mpc_backward(p, dilqr)
    assert torch.equal(x, x2) and torch.equal(u, u2)
    check("dilqr.MPC end to end (torch graph), n=5 m=1 H=(32,16) sigmoid T=6 B=8 box 1", [out2[k] for k in ALL], ref,
          e32, names=ALL)
    # outside the switch or the envelope: the refusal final_step has always given
    refusal = "needs an env_dx model"
    with monkeypatch.context() as mp:
        switches(mp, True)
        mp.setattr(generic, "DEVICE_MLP_DEEP_IMPLICIT", False)
        with pytest.raises(NotImplementedError, match=refusal):
            mpc_backward(p, dilqr)
    with monkeypatch.context() as mp:
        switches(mp, True)
        with pytest.raises(NotImplementedError, match=refusal):
            mpc_backward(mpc_problem("sigmoid", hidden=(N.MLP2_IMPLICIT_MAX_HIDDEN1 + 1, 16)), dilqr)
        with pytest.raises(NotImplementedError, match=refusal):
            mpc_backward(mpc_problem("sigmoid", hidden=(16, 16, 16)), dilqr)
        with pytest.raises(NotImplementedError, match=refusal):
            mpc_backward(p, dilqr, delta_u=0.5)
        with pytest.raises(NotImplementedError, match="slew-rate"):
            mpc_backward(p, dilqr, slew_rate_penalty=0.1)


def test_no_wasted_work(monkeypatch):
    """Only C and c want a gradient: no dF, df, no VJP launch, the same dC, dc."""
    import dilqr
    from dilqr import ops
    switches(monkeypatch, True)
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
    monkeypatch.setattr(ops, "mlp2_linearize_vjp", boom)
    out, x, u, (X0, C, c) = mpc_backward(p, dilqr, weights=False)
    assert len(seen) == 1 and not seen[0][0] and seen[0][1][3] is None and seen[0][1][4] is None
    md = p["dx"].device_model(x, deep=True)
    assert isinstance(md, ops.Mlp2Model)
    full = real(md, gpu(p["wx"]), gpu(p["wu"]), C.detach(), c.detach(), x, u, -1.0, 1.0, want_dF=True)
    assert full[3] is not None and full[4] is not None
    for k, a in zip(("dx_init", "dC", "dc"), full):
        assert torch.equal(out[k], a), k
    ref, e32 = oracle_chain(p, x, u)
    check("C, c only", [out[k] for k in ("dx_init", "dC", "dc")], ref[:3], e32[:3], names=NAMES[:3])
