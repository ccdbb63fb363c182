"""The DiLQR implicit backward on dense, time-varying and asymmetric costs.

k_implicit_backward (tu_implicit.hip; pendulum, cartpole, one lane per
problem) and the rocket group kernel (dilqr_implicit_group.h, 16 lanes per
problem, one per row of C) use all of C: C_t + M_t^T in the modified Riccati
step, full rows in the costates, C_xx y_x + C_xu y_u in dlam.  They also choose
a path per problem (rocket: per row) from the bits of C and c: the first pass
scans them (c_offd, c_dif, cv_dif) and the last pass takes C, c from registers
or reads them again.  The fifteen classes of cost_cases.BACKWARD_CLASSES put
every outcome of that scan in one batch; tests/golden/implicit_costs_f64.npz
(gen_golden.py case_implicit_costs) holds the reference's own
LQRStep(no_op_forward=True) backward on them, T = 10, one problem per class,
for cartpole (unconstrained, box), pendulum (box) and rocket (unconstrained,
box with C_uu symmetric), and tests/test_oracle_golden.py pins both numpy
oracles on the same file.

Every error here is per problem: max|err| over the problem's entries divided
by max|ref| over the same entries (cost_cases.per_problem), at the 1e-4 bar of
the existing implicit tests.

Oracle-pinned problems: on rocket unconstrained the four asym classes have an
asymmetric C_uu with m = 3.  The reference's nested adjoint solve factors Q_uu
by Cholesky there (one triangle read); the kernels, like
oracle.adjoint.implicit_backward_fast, eliminate the asymmetric matrix as it
is.  The two differ by up to 7e-2 (dC, dc) and 1.4e-1 (dtheta), so those four
problems expect implicit_backward_fast's fp64 value, stored in the golden file
next to the reference's own (DESIGN.md sections 4 and 7).  Every other problem,
the asym classes of the other four fixtures included, expects the reference's.

The *_t0 classes change C_0 or c_0 only.  The last pass's outputs do not depend
on C_0, c_0 (lam_0 and dlam_0 feed only the gradient to x_init), so its results
are the same whether or not the scan sees step 0 and whichever path is then
taken: on the device these classes detect nothing that tinv_diag does not (a
scan that misses t = 0 included); only the numpy path_bits test pins what they
are.  They stay as the cases they were asked to be.  The *_mid classes make
the same change at t = T//2 and the generator asserts, on the fp64 oracle,
that a last pass which keeps its registers there moves dtheta by more than ten
times the bar.

Measured (MI355X, one run; worst class, dC / dc / dtheta): cart_unc 2.0e-7 /
1.7e-7 / 2.5e-6, cart_box 1.8e-7 / 1.4e-7 / 2.0e-6, pend_box 6.5e-7 / 6.1e-7 /
4.9e-6, rock_unc 2.6e-6 / 2.5e-6 / 1.4e-5, rock_box 2.2e-7 / 2.3e-7 / 1.3e-5;
widened tensor bounds <= 7.7e-6; T = 2, 3 <= 1.5e-6.  Before dC_entry
(dilqr_common.h) dC was asymmetric by an ulp and the bit-for-bit symmetry
assertion failed on every fixture.
Mutation checks (not committed), classes over the bar in the value tests:
c_regs forced true in k_implicit_backward: diag_tv, tinv_dense, dense, the four
asym, diag_mid, pair_mid (dtheta off by 4e-3 ... 6); cv_regs forced true:
diag_cvar, c_mid (and diag_tv, dense, asym*); Ct[n + a][i] for Ct[i][n + a] in
the last pass's dlam: asym, asym_mid, asym_last only; crow_regs forced true in
the rocket kernel: pair_mid (3e-3 unconstrained, 8e-4 box), diag_mid and the
dense classes.  No mutant moves diag_t0, c_t0 or pair_t0.
"""
import numpy as np
import pytest
import torch

import cost_cases as CC
import test_gpu_parity as P
from oracle import adjoint as oadj
from oracle import models as omodels

pytestmark = pytest.mark.gpu

DEV = P.DEV
gpu, cpu = P.gpu, P.cpu
BAR = 1e-4
NCLS = len(CC.BACKWARD_CLASSES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def true_obj(mname):
    return omodels.MODELS[mname].true_obj()


def per_class(classes, err):
    classes = np.array(classes)
    return ", ".join(f"{k} {err[classes == k].max():.1e}" for k in CC.BACKWARD_CLASSES if (classes == k).any())


def errors(got, exp):
    """[B, 3]: per-problem errors of (dC, dc, dtheta)."""
    return np.stack([CC.per_problem(cpu(got[0]), exp[0], 1), CC.per_problem(cpu(got[1]), exp[1], 1),
                     CC.per_problem(cpu(got[2]), exp[2], 0)], 1)


def check(label, classes, got, exp):
    err = errors(got, exp)
    for k, name in enumerate(("dC", "dc", "dtheta")):
        print(f"\n[{label}] {name}: {per_class(classes, err[:, k])}", end="")
    print()
    bad = {f"{classes[b]}[{b}]": err[b] for b in np.flatnonzero(~(err.max(1) < BAR))}
    assert not bad, bad
    return err


def backward(dx, pr, idx=None, lo=None, hi=None):
    """dilqr.implicit.implicit_backward with K from ops.lqr_backward on the
    fixture's problems idx (all of them if None); returns (dC, dc, dtheta), K."""
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    pick = (lambda a: a) if idx is None else (lambda a: np.take(a, idx, axis=1))
    x, u, C, c, wx, wu = (gpu(pick(pr[k])).contiguous() for k in ("x", "u", "C", "c", "wx", "wu"))
    F = ops.linearize(dx.model_id, ops.theta_of(dx, C), x, u)[0]
    K, _, _ = ops.lqr_backward(C, c, F, pr["n"], pr["m"], x=x, u=u, u_lower=lo, u_upper=hi)
    return implicit_backward(dx, wx, wu, C, c, None, None, x, u, K, lo, hi, None), K


_base = {}


def base_run(golden, tag):
    """The fixture and its B = 15 device run, computed once and shared."""
    if tag not in _base:
        pr = CC.implicit_costs_problem(golden("implicit_costs_f64"), tag, true_obj)
        dx = P.dilqr_models()[pr["mname"]]()
        _base[tag] = (pr, dx, backward(dx, pr, lo=pr["lo"], hi=pr["hi"])[0])
    return _base[tag]


# ------------------------------------------------------------------ a. values
@pytest.mark.parametrize("tag", list(CC.IMPLICIT_COSTS))
def test_implicit_costs_values(golden, tag):
    """dC, dc and per-problem dtheta of the kernel against the golden, per
    problem at 1e-4 (rocket unconstrained's four asym problems against the
    fp64 fast oracle, see the module docstring); then the same fixture through
    dilqr.LQRStep(no_op_forward=True) and autograd: Q.grad, P.grad at the same
    bar per problem, theta.grad (the batch sum) at 1e-4 of its max magnitude
    and equal to the sum of the kernel's per-problem rows within a float32
    sum's rounding, and Q.grad symmetric bit for bit."""
    import dilqr
    from dilqr import ops
    pr, dx, got = base_run(golden, tag)
    exp = (pr["dQ"], pr["dP"], pr["dtheta"])
    check(tag, pr["classes"], got, exp)
    pin = pr["pinned"]
    if pin.any():
        g = golden("implicit_costs_f64")
        sel = np.flatnonzero(pin)
        ref = (g[f"{tag}_ref_dQ"], g[f"{tag}_ref_dP"], g[f"{tag}_ref_dtheta"])
        off = errors([got[0][:, sel], got[1][:, sel], got[2][sel]], ref)
        print(f"[{tag}] oracle-pinned {[pr['classes'][j] for j in sel]}: from the reference's own answer "
              f"dC {off[:, 0].max():.1e} dc {off[:, 1].max():.1e} dtheta {off[:, 2].max():.1e}")
    x, u, x0 = gpu(pr["x"]), gpu(pr["u"]), gpu(pr["x0"])
    Qg, Pg = gpu(pr["C"]).requires_grad_(True), gpu(pr["c"]).requires_grad_(True)
    theta = dx.params.clone().to(DEV).requires_grad_(True)
    F, f = ops.linearize(dx.model_id, ops.theta_of(dx, Qg), x, u)
    step = dilqr.LQRStep(pr["n"], pr["m"], pr["T"], u_lower=pr["lo"], u_upper=pr["hi"],
                         true_cost=dilqr.QuadCost(Qg, Pg), true_dynamics=dx, current_x=x, current_u=u,
                         no_op_forward=True)
    x2, u2 = step(x0, Qg, Pg, F, f, theta)
    ((x2 * gpu(pr["wx"])).sum() + (u2 * gpu(pr["wu"])).sum()).backward()
    eQ, eP = CC.per_problem(cpu(Qg.grad), exp[0], 1), CC.per_problem(cpu(Pg.grad), exp[1], 1)
    eth = float(np.max(np.abs(cpu(theta.grad) - exp[2].sum(0))) / np.max(np.abs(exp[2].sum(0))))
    print(f"[{tag} autograd] Q.grad {eQ.max():.1e} P.grad {eP.max():.1e} theta.grad {eth:.1e}")
    assert eQ.max() < BAR and eP.max() < BAR and eth < BAR
    assert torch.equal(Qg.grad, Qg.grad.transpose(2, 3))
    assert torch.equal(Qg.grad, got[0]) and torch.equal(Pg.grad, got[1])
    # theta.grad is the per-problem rows (each held to the bar above) summed by autograd: nothing
    # but a float32 sum of B terms lies between them, whatever its order ((B - 1) eps sum|terms|)
    rows = cpu(got[2])
    slack = (len(rows) - 1) * np.finfo(np.float32).eps * np.abs(rows).sum(0)
    assert (np.abs(cpu(theta.grad) - rows.sum(0)) <= slack).all(), (cpu(theta.grad) - rows.sum(0), slack)


# ------------------------------------------------------------------ b. paths are per problem
@pytest.mark.parametrize("tag", list(CC.IMPLICIT_COSTS))
def test_implicit_costs_paths_per_problem(golden, tag):
    """The fixture tiled to 128 and 129 problems (rocket: 36 and 37, four
    problems to a wave, so the last wave is partial mid-group) in a rotated
    class order, problem b taking class (b + 5) % 15: every wave mixes every
    path in other lanes than the B = 15 run does.  Each problem's dC, dc,
    dtheta are the B = 15 run's bits for its class."""
    pr, dx, base = base_run(golden, tag)
    for B in (36, 37) if pr["mname"] == "rocket" else (128, 129):
        idx = (np.arange(B) + 5) % NCLS
        got, _ = backward(dx, pr, idx, pr["lo"], pr["hi"])
        it = torch.as_tensor(idx, device=DEV)
        for name, a, ref, ax in (("dC", got[0], base[0], 1), ("dc", got[1], base[1], 1), ("dtheta", got[2], base[2], 0)):
            same = (a == ref.index_select(ax, it)).movedim(ax, 0).reshape(B, -1).all(1).cpu().numpy()
            bad = [f"{pr['classes'][idx[b]]}[{b}]" for b in np.flatnonzero(~same)]
            assert not bad, (B, name, bad)


# ------------------------------------------------------------------ c. tensor bounds
def widened(pr, seed=11):
    """[T,B,m] bounds: the fixture's scalar ones, pushed out by 1 on half of
    the (t, b, a) entries; a control on its bound there becomes free.  Of a
    problem's active controls every second one, in (t, a) order, is widened
    (the fixtures have at least two, so one stays and one is freed); of the
    others a seeded half."""
    T, B, m = pr["u"].shape
    wide = np.random.RandomState(seed).uniform(size=(T, B, m)) < 0.5
    was = (np.abs(pr["u"] - pr["lo"]) <= 1e-8) | (np.abs(pr["u"] - pr["hi"]) <= 1e-8)
    for b in range(B):
        on = np.argwhere(was[:, b])
        for k, (t, a) in enumerate(on):
            wide[t, b, a] = k % 2 == 1
    return np.where(wide, pr["lo"] - 1.0, pr["lo"]), np.where(wide, pr["hi"] + 1.0, pr["hi"]), wide


@pytest.mark.parametrize("tag", [t for t in CC.IMPLICIT_COSTS if t.endswith("_box")])
def test_implicit_costs_tensor_bounds(golden, tag):
    """active() with [T,B,m] tensor bounds.  The scalar bounds passed as
    tensors give the scalar run's bits.  Then the bounds are widened for half
    of the (t, b, a) entries, so the active set differs across t, b and
    (rocket) a and every problem keeps active and free controls (asserted):
    against the fp64 fast oracle on the same float32 inputs, the device's own
    gains in the reference's reversed stacking, per problem at 1e-4."""
    pr, dx, base = base_run(golden, tag)
    T, B, m = pr["u"].shape
    full = lambda v: torch.full((T, B, m), v, device=DEV)  # noqa: E731
    got, _ = backward(dx, pr, None, full(pr["lo"]), full(pr["hi"]))
    assert all(torch.equal(a, b) for a, b in zip(got, base))
    lo, hi, wide = widened(pr)
    u = pr["u"]
    act = (np.abs(u - lo) <= 1e-8) | (np.abs(u - hi) <= 1e-8)
    was = (np.abs(u - pr["lo"]) <= 1e-8) | (np.abs(u - pr["hi"]) <= 1e-8)
    assert (act.sum((0, 2)) >= 1).all() and ((~act).sum((0, 2)) >= 1).all()
    assert ((was & ~act).sum((0, 2)) >= 1).all()            # the widening frees a control in every problem
    assert len({tuple(act[t].ravel()) for t in range(T)}) > 1 and len({tuple(act[:, b].ravel()) for b in range(B)}) > 1
    assert m == 1 or len({tuple(act[:, :, a].ravel()) for a in range(m)}) > 1
    got, K = backward(dx, pr, None, gpu(lo), gpu(hi))
    M = omodels.MODELS[pr["mname"]]
    from oracle import mpc as ompc
    Fo, fo = ompc.linearize(M, pr["x"], u)
    exp = oadj.implicit_backward_fast(M, pr["wx"], pr["wu"], pr["C"], pr["c"], Fo, fo, pr["x"], u,
                                      cpu(K)[::-1].copy(), lo, hi)
    err = check(tag + " widened tensor bounds", pr["classes"], got, exp)
    # and the widening matters: the scalar-bounds answer is not within the bar of this one
    assert (errors(base, exp).max(1) > BAR).any() and err.max() < BAR


# ------------------------------------------------------------------ d. short horizons
@pytest.mark.parametrize("model", ["cartpole", "rocket"])
@pytest.mark.parametrize("T", [2, 3])
def test_implicit_costs_short_horizons(model, T):
    """test_implicit_backward_short_horizons' T = 2 and T = 3 cases with the
    fifteen classes (two problems of each; at T = 2 and 3 the *_mid step is
    t = 1, which at T = 2 is also the step the scan compares against): the
    device's solve on those costs, then the backward against the fp64 fast
    oracle on the same float32 solution, per problem at 1e-4; bounds active
    for cartpole."""
    from dilqr import ops
    from dilqr.implicit import implicit_backward
    B = 2 * NCLS
    cls = CC.backward_classes_of(B)
    if model == "cartpole":
        rng = np.random.RandomState(T)
        th = rng.uniform(-np.pi, np.pi, B)
        x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                       rng.uniform(-1, 1, B)], 1)
        bounds, decay, mls, om = (-2.0, 2.0), 0.5, 2, omodels.Cartpole
    else:
        x0 = P.rocket_x0(B, seed=T)
        bounds, decay, mls, om = None, 0.2, 5, omodels.Rocket
    q, p = om.true_obj()
    n = CC.STATES[model]
    m = q.size - n
    Cn, cn = CC.make_backward_costs(q, p, n, T, cls, 100 + T, sym_uu=False)
    x, u, _ = P.run_gpu_mpc(x0, model, T, 5, bounds, 0.0, 10 ** 9, decay, mls, cost=(Cn, cn))
    assert torch.isfinite(x).all() and torch.isfinite(u).all()
    dx = P.dilqr_models()[model]()
    C, c = gpu(Cn).contiguous(), gpu(cn).contiguous()
    g = torch.Generator(device=DEV).manual_seed(T)
    wx = torch.randn(T, B, n, device=DEV, generator=g)
    wu = torch.randn(T, B, m, device=DEV, generator=g)
    lo, hi = bounds if bounds else (None, None)
    F = ops.linearize(dx.model_id, ops.theta_of(dx, C), x, u)[0]
    K, _, _ = ops.lqr_backward(C, c, F, n, m, x=x, u=u, u_lower=lo, u_upper=hi)
    got = implicit_backward(dx, wx, wu, C, c, None, None, x, u, K, lo, hi, None)
    if bounds:
        n_act = int(((u.abs() - hi).abs() <= 1e-8).sum())
        print(f"\n[{model} T={T}] {n_act} of {T * B} controls active", end="")
        assert 0 < n_act < T * B
    exp = oadj.implicit_backward_fast(om, cpu(wx), cpu(wu), Cn, cn, cpu(F), None, cpu(x), cpu(u), cpu(K)[::-1].copy(),
                                      lo, hi)
    check(f"{model} T={T}", cls, got, exp)
