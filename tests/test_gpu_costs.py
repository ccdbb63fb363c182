"""Dense, time-varying and asymmetric costs against the reference.

dilqr.MPC takes any QuadCost [T,B,d,d]; the solve kernels choose a cost path
per problem from the bits of C (cost_sym flags, dilqr_fused.h) and the Riccati
step has a SYM and a non-SYM form (RiccatiState::step, dilqr_device.h) switched
by `symsofar`.  The cases of tests/cost_cases.py put every path and every
position of that switch in one batch; the goldens (tests/golden/costs_*.npz,
gen_golden.py case_costs) are the reference's own sweeps and mpc_explicit.MPC
solves on them, and tests/test_oracle_golden.py pins the oracle on the same
goldens before the decision replays here rely on it.

The device batch is the fixture tiled (problem b is fixture problem b % Bf):
B = 130 for the single-lane models (two full waves and a two-lane tail), 65
for the sweeps and rocket.  Every copy of a fixture problem must have the same
bits.  Bars are the project's existing ones: K, k 1e-4 relative (relerr);
decision replay as check_against_forced_oracle (trajectories 1e-4, costs 1e-5
or 3x the reference's own fp32-vs-fp64 spread, every differing decision a
near-tie below 1e-5); costs against the reference's fp64 solve at
max(1e-4, 3 x spread).  The generator asserts the conditions on the inputs: at
most 1 problem in 16 with a spread above 1e-5, none above 1e-3; and, stricter,
the numpy oracle run in float32 under decision replay meets the cost bar with a
factor 3 to spare on every problem (gen_golden.py COST_REPLAY_MARGIN, where the
reason is written down).  Seeds: pendulum and rocket 0; the two cartpole cases
1.  Their seed 0 met the first condition but not the second, on its two
tinv_diag problems 0 and 32 (swing-ups whose fp32 error grows ~10x per
iteration at the end): the float32 oracle was 4.4e-5 / 4.9e-5 from the forced
fp64 oracle on cart_mixed_box10 where the reference's fp32 spread was 2.4e-6 /
3.0e-5, and the device, run once on that seed, 4.6e-5 / 9.0e-5 (bars 1e-5 /
9.0e-5; every other problem and case passed).

The 16-lane rocket kernels write two cost_sym values only (7: a time-invariant
diagonal cost in registers, 0: the caller's rows), so the rocket cases expect
7 for tinv_diag and 0 for every other class.

Measured (MI355X, one run of the whole GPU suite; maxima over the eight classes
unless a class is named; no class stands out, the asym* ones included):
  * sweeps, K / k against the reference: (3,1) 1.4e-7 / 7.2e-7, (5,1) 1.2e-7 /
    4.3e-7, (4,2) 2.1e-7 / 1.0e-7, (4,3) 2.0e-7 / 1.6e-7 (Cholesky engine
    included), (13,3) 4.7e-6 / 1.8e-6 unconstrained, 3.0e-6 / 4.4e-6 box,
    1.6e-5 / 7.0e-6 Cholesky (asym_last; the reference's own fp32 sweep is
    1.0e-5 from its fp64 there)
  * decision replay, cost / u / x against the forced fp64 oracle, near-tie flips:
    cart_mixed_unc 2.8e-6 / 2.8e-6 / 8.8e-7, 14 of 800;
    cart_mixed_box10 2.2e-6 / 1.5e-5 / 1.6e-6, 21 of 800;
    pend_mixed_box 3.9e-7 / 4.0e-7 / 8.7e-8, 22 of 800;
    rocket_dense_unc 3.0e-7 / 3.7e-7 / 1.0e-7, 24 of 320;
    rocket_dense_box20 3.5e-7 / 1.4e-6 / 5.2e-7, 26 of 320;
    rocket_diag_it10 3.2e-7 / 5.5e-6 / 7.8e-7, 12 of 320
  * costs against the reference's fp64 solves: cart 2.8e-6 / 2.2e-6 (asym_last),
    pend 2.5e-6 (asym), rocket 2.8e-7 / 3.2e-7 / 3.2e-7
  * the full-size rocket slice (test_gpu_parity.py): cost 7.5e-8, u 7.1e-7, x
    1.1e-7, no flips in 60
Mutation check (not committed): with the non-SYM branch of RiccatiState::step
made to mirror its upper triangle, the sweep tests of the four single-lane
shapes fail in every mode with K errors of 0.04-0.46 on the asym* classes
(all four of them unconstrained, with the Cholesky engine and with the m > 1
box; asym and asym_last with the m = 1 box, whose clamped controls zero the
gain) and unchanged errors (<= 4.3e-7) on the other four classes, and the three
cartpole / pendulum replays fail at iteration 1 on asym* problems only (step
sizes that differ without being a near-tie); the (13,3) and rocket tests,
which run the group kernels' own step, are unaffected.
"""
import numpy as np
import pytest
import torch

import cost_cases as CC
import test_gpu_parity as P
from oracle import models as omodels

pytestmark = pytest.mark.gpu

DEV = P.DEV
gpu, cpu, same_bits = P.gpu, P.cpu, P.same_bits


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def true_obj(mname):
    return omodels.MODELS[mname].true_obj()


def per_class(classes, err):
    """'class max' pairs of a per-problem error array."""
    classes = np.array(classes)
    return ", ".join(f"{k} {err[classes == k].max():.1e}" for k in CC.CLASSES if (classes == k).any())


def copies_same_bits(t, Bf, axis=1):
    """Every copy of a fixture problem (b % Bf) equals the first one, bit for bit."""
    idx = torch.arange(t.shape[axis], device=t.device) % Bf
    return same_bits(t, t.index_select(axis, idx))


# ------------------------------------------------------------------ a. sweeps vs the reference
SWEEP_B = 65


@pytest.mark.parametrize("name,mode", [(n_, mo) for n_ in CC.SWEEP_SHAPES for mo in CC.SWEEP_MODES[n_]])
def test_sweep_cost_classes_vs_reference(golden, name, mode):
    """ops.lqr_backward (c_back formed in the kernel from x, u) on the eight
    cost classes, T = 9, the 16 fixture problems tiled to B = 65, against the
    reference's sweep (LQRStepFn.forward, fp64): unconstrained, box +-0.5 and,
    for m = 3, the Cholesky engine.  The reference is finite on an asymmetric
    C_uu in every mode, so every mode runs all eight classes (the box keeps
    C_uu symmetric for m > 1, as cost_cases defines the bounded cases)."""
    from dilqr import _native as N
    from dilqr import ops
    g = golden("costs_f64")
    pr = CC.sweep_problem(name, true_obj, int(g[f"{name}_seed"]))
    CC.check(g[f"{name}_sum"], pr["C"], pr["c"], pr["C_box"], pr["c_box"], pr["F"], pr["x"], pr["u"])
    n, m, Bf = pr["n"], pr["m"], CC.SWEEP_B
    C, c = (pr["C_box"], pr["c_box"]) if mode == "box" else (pr["C"], pr["c"])
    kw = {}
    if mode == "box":
        kw = dict(u_lower=-CC.SWEEP_BOX, u_upper=CC.SWEEP_BOX)
    elif mode == "chol":
        kw = dict(m_solver=N.SOLVE_CHOL)
    t = lambda a: gpu(CC.tile(a, SWEEP_B)).contiguous()  # noqa: E731
    K, k, _ = ops.lqr_backward(t(C), t(c), t(pr["F"]), n, m, x=t(pr["x"]), u=t(pr["u"]), **kw)
    assert copies_same_bits(K, Bf) and copies_same_bits(k, Bf)
    Kr, kr = g[f"{name}_{mode}_K"], g[f"{name}_{mode}_k"]
    eK = np.abs(cpu(K[:, :Bf]) - Kr).max(axis=(0, 2, 3)) / max(1.0, np.abs(Kr).max())
    ek = np.abs(cpu(k[:, :Bf]) - kr).max(axis=(0, 2)) / max(1.0, np.abs(kr).max())
    print(f"\n[sweep {name} {mode}] K: {per_class(pr['classes'], eK)}; k: {per_class(pr['classes'], ek)}")
    assert P.relerr(cpu(K[:, :Bf]), Kr) < 1e-4
    assert P.relerr(cpu(k[:, :Bf]), kr) < 1e-4


# ------------------------------------------------------------------ b. MPC solves by decision replay
def device_batch(name):
    return 65 if CC.MPC_CASES[name][0] == "rocket" else 130


def fixture(golden, name):
    """The case's settings, x0 [Bf, n] and regenerated (C, c), checksum asserted."""
    g = golden("costs_f64")
    C, c = CC.mpc_costs(name, true_obj, int(g[f"{name}_seed"]))
    CC.check(g[f"{name}_sum"], C, c)
    return g, g[f"{name}_x0"], C, c


def tiled(x0, C, c, B):
    return CC.tile(x0, B, axis=0), (CC.tile(C, B), CC.tile(c, B))


@pytest.mark.parametrize("name", list(CC.MPC_CASES))
def test_mpc_cost_classes_by_decision_replay(golden, name):
    """The per-iteration solve path on the mixed-class fixtures (rocket: at
    config 3's 10 iterations, dense and asymmetric costs through the 8-lane
    sweep's dense-cost grid, and the true diagonal cost): the fp64 oracle made
    to take the device's decisions, then the costs against the reference's own
    fp64 solve, and the cost_sym flag of every problem."""
    mname, T, Bf, it, bounds, decay, mls, mixed = CC.MPC_CASES[name]
    g, x0, C, c = fixture(golden, name)
    B = device_batch(name)
    x0d, costd = tiled(x0, C, c, B)
    flags = []
    x, u, costs, alphas, takes = P.gpu_solve_with_decisions(x0d, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls,
                                                            cost=costd, flags_out=flags)
    assert len(alphas) == it
    assert copies_same_bits(x, Bf) and copies_same_bits(u, Bf) and copies_same_bits(costs, Bf, axis=0)
    classes = CC.classes_of(Bf) if mixed else ["tinv_diag"] * Bf
    want = CC.flags_of(classes, rocket=mname == "rocket")
    assert np.array_equal(flags[0], CC.tile(want, B, axis=0)), flags[0]
    spread = g[f"{name}_spread"]
    detail = {}
    P.check_against_forced_oracle(omodels.MODELS[mname], x0, T, bounds, decay, mls, x[:, :Bf], u[:, :Bf],
                                  costs[:Bf], [a[:Bf] for a in alphas], [t_[:Bf] for t_ in takes], name,
                                  ref_spread=spread, cost=(C, c), detail=detail)
    ref = g[f"{name}_costs"]
    rerr = np.abs(cpu(costs[:Bf]) - ref) / np.maximum(1.0, np.abs(ref))
    print(f"[{name}] forced oracle per class: cost {per_class(classes, detail['cost'])}; u "
          f"{per_class(classes, detail['u'])}; x {per_class(classes, detail['x'])}; near-tie flips "
          f"{detail['flips']}/{detail['total']}\n[{name}] vs the reference's fp64 costs per class: "
          f"{per_class(classes, rerr)}; reference fp32 spread max {spread.max():.1e}")
    assert np.all(rerr < np.maximum(1e-4, 3 * spread)), (np.flatnonzero(rerr >= 1e-4), rerr.max())


# ------------------------------------------------------------------ c. every launch route, the same bits
LANE_CASES = [k for k, v in CC.MPC_CASES.items() if v[0] != "rocket"]
ROCKET_CASES = [k for k, v in CC.MPC_CASES.items() if v[0] == "rocket"]


@pytest.mark.parametrize("name", LANE_CASES)
def test_cost_classes_every_launch_route_same_bits(golden, name):
    """The per-iteration path, dilqr.MPC (the fixed-count whole-solve launch:
    cost speculation, the streamed cost check, carried lane state),
    ops.mpc_solve_unfused and the one-launch small-batch solve give identical
    best trajectories and costs on the mixed-class batch."""
    from dilqr import _native as N
    from dilqr import ops
    mname, T, Bf, it, bounds, decay, mls, _mixed = CC.MPC_CASES[name]
    _g, x0, C, c = fixture(golden, name)
    B = device_batch(name)
    x0d, costd = tiled(x0, C, c, B)
    per_it = P.gpu_solve_with_decisions(x0d, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, cost=costd)[:3]
    routes = {"dilqr.MPC": P.run_gpu_mpc(x0d, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, cost=costd),
              "mpc_solve_unfused": P.run_gpu_mpc(x0d, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, fused=False,
                                                 cost=costd)}
    dx = P.dilqr_models()[mname]()
    Cd, cd = P.device_cost(dx, T, B, costd)
    x0g = gpu(x0d)
    bd, keep = N.make_bounds(*(bounds if bounds else (None, None)))
    sv = ops.MPCSolve(T, B, dx.n_state, dx.n_ctrl, DEV)
    sv.solve_small(dx.model_id, ops.theta_of(dx, x0g), x0g, Cd, cd, bd, decay, mls, it, 1e-4, 0.0, 10 ** 9)
    assert sv.iterations == it
    routes["solve_small"] = sv.gather_best() + (sv.best_cost,)
    del keep
    for route, got in routes.items():
        for ta, tb in zip(per_it, got):
            assert same_bits(ta, tb), (route, P.relerr(cpu(ta), cpu(tb)))


@pytest.mark.parametrize("name", ROCKET_CASES)
def test_cost_classes_rocket_fused_equals_unfused(golden, name):
    """Rocket on the mixed-class batch: the fused iteration (8-lane sweep,
    lane-quad search, register cost or the dense-cost grid per wave) against
    the unfused 16-lane kernels, bit for bit."""
    mname, T, Bf, it, bounds, decay, mls, _mixed = CC.MPC_CASES[name]
    _g, x0, C, c = fixture(golden, name)
    x0d, costd = tiled(x0, C, c, device_batch(name))
    a = P.run_gpu_mpc(x0d, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, fused=True, cost=costd)
    b = P.run_gpu_mpc(x0d, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, fused=False, cost=costd)
    for ta, tb in zip(a, b):
        assert same_bits(ta, tb), P.relerr(cpu(ta), cpu(tb))


# ------------------------------------------------------------------ d. arrangement does not matter
@pytest.mark.parametrize("name", ["cart_mixed_unc", "cart_mixed_box10"])
def test_cost_classes_arrangement_independent(golden, name):
    """The cartpole mixed case arranged two ways: classes interleaved lane by
    lane (one wave holds every path), and 64 tinv_diag problems first, then
    the 40 mixed ones — a first wave that is uniformly flag 7 (the wave-uniform
    register path and its speculation) beside a mixed one.  Each fixture
    problem gives the same bits in both, through the whole-solve launch and
    through the per-iteration path."""
    mname, T, Bf, it, bounds, decay, mls, _mixed = CC.MPC_CASES[name]
    _g, x0, C, c = fixture(golden, name)
    x0a, costa = tiled(x0, C, c, device_batch(name))
    first = np.flatnonzero(np.array(CC.classes_of(Bf)) == "tinv_diag")
    order = np.concatenate([first[np.arange(64) % first.size], np.arange(Bf)])        # fixture problem per lane
    x0b, costb = x0[order], (C[:, order], c[:, order])
    order_t = torch.tensor(order, device=DEV)
    for route in ("whole", "per_iteration"):
        if route == "whole":
            a = P.run_gpu_mpc(x0a, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, cost=costa)
            b = P.run_gpu_mpc(x0b, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, cost=costb)
        else:
            fl = []
            a = P.gpu_solve_with_decisions(x0a, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, cost=costa)[:3]
            b = P.gpu_solve_with_decisions(x0b, mname, T, it, bounds, 0.0, 10 ** 9, decay, mls, cost=costb,
                                           flags_out=fl)[:3]
            assert (fl[0][:64] == 7).all() and np.array_equal(fl[0][64:], CC.flags_of(CC.classes_of(Bf)))
        for ta, tb in zip(a, b):
            axis = 0 if ta.dim() == 1 else 1
            assert same_bits(ta.index_select(axis, order_t), tb), route
