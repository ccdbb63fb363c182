"""The whole-solve launch (k_mpc_solve_fixed) does not wait for begin's pass over
all T cost records: a wave whose problems pass a guard on records 0 and T-1
iterates at once on the guess "diag(q), p at every t" and tests records
1 .. T-2 under the iterations (dilqr_fused.h, CostCheck).  A wave
whose guess holds commits the flags and the one packed record the analysing
begin leaves; a wave whose guess fails runs the solve again from the top on the
ordinary route.  Either way MPCSolve.solve_fixed must leave the state of begin +
iterate_fixed per iteration + finish_fixed, bit for bit: the solution, the cost
flags and the packed cost copy.  Cartpole only; the shapes are the smallest at
which the route can go wrong: T = 1, 2 (no record to test), 3, 4 (one, two),
25; one lane, a whole wave, ragged waves; 1, 2, 3 and 10 iterations (everything
tested inside the first iteration / spread over several).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("slot", "cost", "alpha", "improved", "best_cost", "best_du", "full_du_norm", "best_iter")
D = 6                                                           # cartpole: n + m
PK = D * (D + 1) // 2 + D


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same_bits(a, b):
    """Equal element for element, NaN matching NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, 0.0, a), torch.where(nb, 0.0, b))


def cartpole():
    from dilqr.env_dx.cartpole import CartpoleDx
    return CartpoleDx()


def initial_states(B, seed):
    rng = np.random.RandomState(seed)
    th = rng.uniform(-np.pi, np.pi, B)
    x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                   rng.uniform(-1, 1, B)], 1)
    return torch.tensor(x0, dtype=torch.float32, device=DEV)


def true_cost(dx, T, B):
    """diag(q), p repeated over t and the batch, on the host (the tests poison it there)."""
    q, p = dx.get_true_obj()
    return torch.diag(q).repeat(T, B, 1, 1).contiguous(), p.repeat(T, B, 1).contiguous()


def packed_records(sv):
    """The solve's packed cost copy as [T, B, PK] words (SoaRec<27>: six float4
    planes, one float2 plane, one float plane, each [T, ., B])."""
    T, B = sv.T, sv.B
    w = sv.Cpk.view(torch.int32)
    q4 = w[:T * B * 24].view(T, 6, B, 4).permute(0, 2, 1, 3).reshape(T, B, 24)
    r2 = w[T * B * 24:T * B * 26].view(T, B, 2)
    r1 = w[T * B * 26:T * B * 27].view(T, B, 1)
    return torch.cat([q4, r2, r1], 2)


def check(dx, T, x0, C, c, iters, bounds=(None, None), u0=None):
    """solve_fixed against the per-launch path: the solve's state, the gathered
    best trajectory, the cost flags and the packed copy: both copies start
    filled with one NaN pattern, both paths must write the same records (the
    one at T-1 when a problem's packed records are the same at every t, else
    all T), and every written record must agree.  Returns the flags."""
    from dilqr import _native as N
    from dilqr import ops
    B, n, m = x0.shape[0], dx.n_state, dx.n_ctrl
    C, c = C.to(DEV).contiguous(), c.to(DEV).contiguous()
    theta = ops.theta_of(dx, x0)
    bd, keep = N.make_bounds(*bounds)
    a = ops.MPCSolve(T, B, n, m, x0.device, fixed_iters=iters)
    a.Cpk.fill_(float("nan"))
    a.begin(dx.model_id, theta, x0, u0)
    for i in range(iters):
        a.iterate_fixed(dx.model_id, theta, x0, C, c, bd, 0.5, 2, i, 1e-4)
    a.finish_fixed(iters)
    b = ops.MPCSolve(T, B, n, m, x0.device, fixed_iters=iters)
    b.Cpk.fill_(float("nan"))                                   # nothing left over from an earlier solve
    b.solve_fixed(dx.model_id, theta, x0, C, c, bd, 0.5, 2, 1e-4, u0)
    for key in KEYS:
        assert same_bits(getattr(a, key).float(), getattr(b, key).float()), key
    xa, ua = a.gather_best()
    xb, ub = b.gather_best()
    assert same_bits(xa, xb) and same_bits(ua, ub)
    assert torch.equal(a.cost_sym, b.cost_sym), (a.cost_sym.tolist(), b.cost_sym.tolist())
    pa, pb = packed_records(a), packed_records(b)
    # a record is written unless every word of it still holds the fill (no
    # packed record is all NaN: its off-diagonal words come from the caller's C,
    # and the tests poison one word)
    fill = torch.full((1,), float("nan"), device=DEV).view(torch.int32)
    wa, wb = (pa != fill).any(2), (pb != fill).any(2)           # [T, B]
    assert wa[T - 1].all()
    assert torch.equal(wa, wb), (wa.sum(0).tolist(), wb.sum(0).tolist())
    kept_all = wa.all(0)                                        # every problem keeps record T-1 alone or all T
    assert torch.equal(wa.sum(0), torch.where(kept_all, T, 1))
    assert torch.equal(pa[wa], pb[wa])
    del keep
    return a.cost_sym.cpu()


def warm_start(T, B):
    return (0.3 * torch.randn(T, B, 1, generator=torch.Generator().manual_seed(5))).to(DEV)


@pytest.mark.parametrize("iters", [1, 2, 3, 10])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 25])
def test_clean_cost_commits(T, B, iters):
    """Every problem diag(q), p repeated: every wave of the unconstrained solve
    speculates and commits (the bounded kernels keep the analysing begin and
    must agree all the same)."""
    dx = cartpole()
    x0 = initial_states(B, 1000 * T + 10 * B + iters)
    C, c = true_cost(dx, T, B)
    for bounds in ((None, None), (-10.0, 10.0)):
        for u0 in (None, warm_start(T, B)):
            flags = check(dx, T, x0, C, c, iters, bounds=bounds, u0=u0)
            assert (flags == 7).all(), flags


def poison(C, c, r, b, kind):
    """One word (two for 'asym') of record r of problem b."""
    if kind == "diag_ulp":
        C[r, b, 2, 2] = float(np.nextafter(np.float32(C[r, b, 2, 2].item()), np.float32(np.inf)))
    elif kind == "c_ulp":
        c[r, b, 3] = float(np.nextafter(np.float32(c[r, b, 3].item()), np.float32(np.inf)))
    elif kind == "offdiag_small":
        C[r, b, 4, 1] = 1e-6
    elif kind == "offdiag_negzero":                             # equal as a value, not as bits
        C[r, b, 1, 5] = -0.0
    elif kind == "asym":
        C[r, b, 0, 3] = 1e-3
        C[r, b, 3, 0] = 2e-3
    elif kind == "diag_nan":
        C[r, b, 5, 5] = float("nan")
    else:
        raise ValueError(kind)


# the expected flags of the poisoned problem (kCostSym 1, kCostDiag 2, kCostTinv 4)
POISON_FLAGS = {"diag_ulp": 3, "c_ulp": 3, "offdiag_small": 0, "offdiag_negzero": 0, "asym": 0, "diag_nan": 3}
# T < 3 has no record between 0 and T-1, so there is nothing to poison there:
# those horizons are left out here on purpose (test_clean_cost_commits and the
# guard tests run them).  Middle records of each horizon: 1, T//2, T-2.
POISON_TR = [(3, 1), (4, 1), (4, 2), (25, 1), (25, 12), (25, 23)]
# B = 192: three whole waves; (wave, lane) of the poisoned problem
POISON_WL = [(0, 0), (0, 37), (0, 63), (2, 0), (2, 37), (2, 63)]


@pytest.mark.parametrize("kind", sorted(POISON_FLAGS))
@pytest.mark.parametrize("T,r", POISON_TR)
def test_poisoned_middle_record_restarts(T, r, kind):
    """One problem whose record r differs from record 0 in one word: it passes
    the guard, so its wave speculates, finds the word and solves again.  The
    poisoned problem's flags, copy and solution and its neighbours' bits are the
    per-launch path's, and every other problem keeps flags 7."""
    dx = cartpole()
    B = 192
    x0 = initial_states(B, 100 * T + r)
    for k, (wave, lane) in enumerate(POISON_WL):
        b = 64 * wave + lane
        C, c = true_cost(dx, T, B)
        poison(C, c, r, b, kind)
        assert 0 < r < T - 1
        iters = (1, 2, 3, 10)[(k + r) % 4]
        bounds = (None, None) if k % 2 else (-10.0, 10.0)
        flags = check(dx, T, x0, C, c, iters, bounds=bounds, u0=warm_start(T, B) if k % 3 == 0 else None)
        want = torch.full((B,), 7, dtype=torch.uint8)
        want[b] = POISON_FLAGS[kind]
        assert torch.equal(flags, want), (b, flags.tolist())


@pytest.mark.parametrize("iters", [1, 2, 3, 10])
@pytest.mark.parametrize("T", [3, 25])
def test_poisoned_ragged_last_wave(T, iters):
    """B = 130: the last wave has two live lanes; one of them is poisoned."""
    dx = cartpole()
    B = 130
    x0 = initial_states(B, 7 * T + iters)
    C, c = true_cost(dx, T, B)
    poison(C, c, T // 2, 129, "offdiag_negzero")
    flags = check(dx, T, x0, C, c, iters)
    assert flags[129] == 0 and (flags[:129] == 7).all()


# (T = 1 has one record: no terminal cost apart from record 0)
GUARD_CASES = [(T, kind) for T in (1, 2, 3, 25) for kind in ("terminal", "dense0", "asym0")
               if not (T == 1 and kind == "terminal")]


@pytest.mark.parametrize("T,kind", GUARD_CASES)
def test_guard_failures_take_the_ordinary_route(T, kind):
    """One lane of an otherwise clean wave fails the guard — record T-1 differs
    from record 0 (a terminal cost), record 0 is dense symmetric, record 0 is
    asymmetric — so its wave never speculates."""
    dx = cartpole()
    B = 130
    x0 = initial_states(B, 31 * T)
    C, c = true_cost(dx, T, B)
    b = 70
    if kind == "terminal":
        C[T - 1, b] = 10.0 * C[T - 1, b]
        want = 3
    elif kind == "dense0":
        L = torch.randn(D, D, generator=torch.Generator().manual_seed(2)) * 0.1
        C[0, b] = C[0, b] + L @ L.T
        C[0, b] = 0.5 * (C[0, b] + C[0, b].T)
        want = 1 if T > 1 else 5
    else:
        C[0, b, 0, 1] = 1e-3
        want = 0
    for iters in (1, 3):
        flags = check(dx, T, x0, C, c, iters)
        assert flags[b] == want and (flags[:b] == 7).all() and (flags[b + 1:] == 7).all(), flags.tolist()


def test_non_finite_initial_state_commits():
    """A problem with an infinite initial state component next to clean ones:
    its cost is clean, so its wave commits; its own costs are NaN on both paths."""
    dx = cartpole()
    T, B = 25, 130
    x0 = initial_states(B, 77)
    x0[5, 0] = float("inf")
    x0[129, 4] = float("nan")
    C, c = true_cost(dx, T, B)
    for iters in (1, 10):
        flags = check(dx, T, x0, C, c, iters)
        assert (flags == 7).all()


@pytest.mark.parametrize("both_ends", [False, True])
@pytest.mark.parametrize("T", [3, 25])
def test_wrong_guess_that_diverges(T, both_ends):
    """A negative control weight at record 0 and the true one from record 1 on.
    With record 0 alone the guard sees it (record T-1 differs); with records 0
    and T-1 both negative the wave speculates on a cost that makes its
    iterations diverge, then finds record 1 and solves again.  The result is
    the per-launch path's, and nothing outside that problem changes."""
    dx = cartpole()
    B = 192
    x0 = initial_states(B, 5 * T)
    C, c = true_cost(dx, T, B)
    b = 64 + 37
    for t in ((0, T - 1) if both_ends else (0,)):
        C[t, b, 5, 5] = -50.0
        C[t, b, 0, 0] = -3.0
    for iters, bounds in ((2, (None, None)), (10, (None, None)), (10, (-10.0, 10.0))):
        flags = check(dx, T, x0, C, c, iters, bounds=bounds)
        want = torch.full((B,), 7, dtype=torch.uint8)
        want[b] = 3
        assert torch.equal(flags, want), flags.tolist()
