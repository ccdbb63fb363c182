"""The whole-solve kernels keep a per-lane carry in registers between the
phases of a solve (LaneCarry, dilqr_fused.h: the cost registers, the head
records u_0, x_1, u_1 handed from the sweep to the line search, x_init, the
tail record T-1 handed from the line search to the next sweep), where the
per-iteration launches store and re-read those values.  Every value handed over
is the value the load it replaces returns, so MPCSolve.solve_fixed must leave
exactly the state of begin + iterate_fixed per iteration + finish_fixed — the
per-launch path, which enters every phase with an empty carry — bit for bit,
at the smallest shapes where the carry can go wrong: T = 1..4 (record 1
clamps, nearly all peeled steps), ragged batches, both bounds modes, gains in
HBM, the non-pair line search, warm starts, every cost path, non-finite costs.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("slot", "cost", "alpha", "improved", "best_cost", "best_du", "full_du_norm", "best_iter")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same_bits(a, b):
    """Equal element for element, NaN matching NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, 0.0, a), torch.where(nb, 0.0, b))


def model(mname):
    from dilqr.env_dx.cartpole import CartpoleDx
    from dilqr.env_dx.pendulum import PendulumDx
    return CartpoleDx() if mname == "cartpole" else PendulumDx()


def initial_states(mname, B, seed):
    rng = np.random.RandomState(seed)
    if mname == "pendulum":
        th = rng.uniform(-np.pi / 2, np.pi / 2, B)
        x0 = np.stack([np.cos(th), np.sin(th), rng.uniform(-1, 1, B)], 1)
    else:
        th = rng.uniform(-np.pi, np.pi, B)
        x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), np.cos(th), np.sin(th),
                       rng.uniform(-1, 1, B)], 1)
    return torch.tensor(x0, dtype=torch.float32, device=DEV)


def true_cost(dx, T, B):
    q, p = dx.get_true_obj()
    return (torch.diag(q).repeat(T, B, 1, 1).to(DEV).contiguous(), p.repeat(T, B, 1).to(DEV).contiguous())


def check_solve(dx, T, x0, C, c, iters, bounds=(None, None), decay=0.5, mls=2, u0=None):
    """solve_fixed against the per-launch path; returns the per-launch path's
    step sizes [iters, B] and the whole-solve state."""
    from dilqr import _native as N
    from dilqr import ops
    B, n, m = x0.shape[0], dx.n_state, dx.n_ctrl
    theta = ops.theta_of(dx, x0)
    bd, keep = N.make_bounds(*bounds)
    a = ops.MPCSolve(T, B, n, m, x0.device, fixed_iters=iters)
    a.begin(dx.model_id, theta, x0, u0)
    alphas = []
    for i in range(iters):
        a.iterate_fixed(dx.model_id, theta, x0, C, c, bd, decay, mls, i, 1e-4)
        alphas.append(a.alpha.clone())
    a.finish_fixed(iters)
    b = ops.MPCSolve(T, B, n, m, x0.device, fixed_iters=iters)
    b.solve_fixed(dx.model_id, theta, x0, C, c, bd, decay, mls, 1e-4, u0)
    for key in KEYS:
        assert same_bits(getattr(a, key).float(), getattr(b, key).float()), key
    xa, ua = a.gather_best()
    xb, ub = b.gather_best()
    assert same_bits(xa, xb) and same_bits(ua, ub)
    del keep
    return torch.stack(alphas), b


@pytest.mark.parametrize("iters", [1, 2, 10])
@pytest.mark.parametrize("B", [1, 65, 130])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 25])
def test_carry_short_horizons_and_ragged_batches(T, B, iters):
    """T = 1 has no record 1 (the head clamps to record 0), T = 2 and 3 are
    nearly all peeled steps; B = 1, 65, 130 leave idle lanes in the last wave;
    1 iteration uses only begin's carry, 2 hand one line search's tail over."""
    dx = model("cartpole")
    x0 = initial_states("cartpole", B, 100 * T + B)
    C, c = true_cost(dx, T, B)
    _al, sv = check_solve(dx, T, x0, C, c, iters)
    assert torch.isfinite(sv.best_cost).all()


@pytest.fixture(scope="module")
def headline():
    """The headline's own problems and cost (bench.make_problems), 192 of them."""
    import bench
    x0n, q, p = bench.make_problems(192)
    T, B = bench.T_HORIZON, 192
    x0 = torch.tensor(x0n, device=DEV)
    C = torch.diag(torch.tensor(q)).repeat(T, B, 1, 1).to(DEV).contiguous()
    c = torch.tensor(p).repeat(T, B, 1).to(DEV).contiguous()
    return T, B, x0, C, c


def test_carry_headline_with_b_winners(headline):
    """The headline's settings (decay 0.5, max_ls 2, 10 iterations).  The tail
    record and the copy-out only matter for problems whose candidate B won, so
    the test requires them: B-winners (alpha = decay) in at least three
    iterations, in the last iteration, and one problem taking B in two
    consecutive iterations (its next sweep starts on a tail selected from B)."""
    T, B, x0, C, c = headline
    al, _sv = check_solve(model("cartpole"), T, x0, C, c, 10)
    took_b = al == 0.5                                          # [iters, B]
    per_iter = took_b.sum(1).tolist()
    print("B-winners per iteration:", per_iter)
    assert sum(k > 0 for k in per_iter) >= 3, per_iter
    assert per_iter[-1] > 0, per_iter
    assert bool((took_b[1:] & took_b[:-1]).any()), per_iter


@pytest.mark.parametrize("mode", ["scalar", "tensor"])
def test_carry_headline_bounds(headline, mode):
    """Scalar bounds +-10 and per-(t,b) tensor bounds on the headline case."""
    T, B, x0, C, c = headline
    if mode == "scalar":
        bounds = (-10.0, 10.0)
    else:
        gen = torch.Generator().manual_seed(11)
        bounds = ((-10.0 * (0.3 + 0.7 * torch.rand(T, B, 1, generator=gen))).to(DEV),
                  (10.0 * (0.3 + 0.7 * torch.rand(T, B, 1, generator=gen))).to(DEV))
    check_solve(model("cartpole"), T, x0, C, c, 10, bounds=bounds)


def test_carry_headline_warm_start(headline):
    """A u_init warm start: begin's rollout, and so its tail record, is not the zero-control one."""
    T, B, x0, C, c = headline
    u0 = (0.3 * torch.randn(T, B, 1, generator=torch.Generator().manual_seed(5))).to(DEV)
    check_solve(model("cartpole"), T, x0, C, c, 10, u0=u0)


def test_carry_hbm_gains():
    """T = 48, B = 100: the gain records are in HBM, candidate B rolls out into
    its slot, and there is no LDS copy-out."""
    dx = model("cartpole")
    T, B = 48, 100
    x0 = initial_states("cartpole", B, 48100)
    C, c = true_cost(dx, T, B)
    check_solve(dx, T, x0, C, c, 6)


@pytest.mark.parametrize("mls,decay", [(1, 0.5), (3, 0.2), (3, 0.5)])
def test_carry_non_pair_line_search(headline, mls, decay):
    """max_ls = 1 (candidate A alone) and 3 (two rounds: the tail record is the
    winning round's candidate)."""
    T, B, x0, C, c = headline
    check_solve(model("cartpole"), T, x0, C, c, 6, decay=decay, mls=mls)


def _costs(dx, T, B, kind, seed=3):
    d = dx.n_state + dx.n_ctrl
    g = torch.Generator().manual_seed(seed)
    q, p = dx.get_true_obj()
    C = torch.diag(q).repeat(T, B, 1, 1)
    c = p.repeat(T, B, 1)
    if kind == "diag_tv":                                       # a time-varying diagonal cost
        c = c + 0.01 * torch.randn(T, B, d, generator=g)
        C = C * (1.0 + 0.1 * torch.rand(T, B, 1, 1, generator=g))
    elif kind in ("dense", "asym"):                             # dense, bitwise symmetric (and then not)
        L = torch.randn(T, B, d, d, generator=g) * (0.3 / d ** 0.5)
        C = C + L @ L.transpose(-1, -2)
        C = 0.5 * (C + C.transpose(-1, -2))
        if kind == "asym":
            C[:, :, 0, 1] += 1e-3
    elif kind == "mixed":                                       # as test_packed_cost_paths_bit_identical builds them
        L = torch.randn(T, B // 2, d, d, generator=g) * (0.3 / d ** 0.5)
        C[:, B // 2:] = C[:, B // 2:] + L @ L.transpose(-1, -2)
        C[:, 3 * B // 4:, 0, 1] += 1e-3
        c = c + 0.01 * torch.randn(T, B, d, generator=g)
        c[:, :B // 4] = c[0, :B // 4]
        C[:, B // 2:5 * B // 8] = C[0, B // 2:5 * B // 8]
        c[:, B // 2:5 * B // 8] = c[0, B // 2:5 * B // 8]
    return C.to(DEV).contiguous(), c.to(DEV).contiguous()


@pytest.mark.parametrize("kind", ["diag_tv", "dense", "asym", "mixed"])
def test_carry_other_cost_paths(kind):
    """Costs that leave the time-invariant diagonal path keep reading their
    cost as before but still run on the carried trajectory records."""
    dx = model("cartpole")
    T, B = 12, 128
    x0 = initial_states("cartpole", B, 7)
    C, c = _costs(dx, T, B, kind)
    _al, sv = check_solve(dx, T, x0, C, c, 6, decay=0.5, mls=4 if kind == "mixed" else 2)
    flags = sv.cost_sym.cpu()
    want = {"diag_tv": 3, "dense": 1, "asym": 0}
    if kind == "mixed":
        assert (flags[:B // 4] == 7).all() and (flags[B // 4:B // 2] == 3).all()
        assert (flags[B // 2:5 * B // 8] == 5).all() and (flags[5 * B // 8:3 * B // 4] == 1).all()
        assert (flags[3 * B // 4:] == 0).all()
    else:
        assert (flags == want[kind]).all(), flags


def test_carry_non_finite_problem(headline):
    """One problem with an infinite initial state component: its costs are NaN
    on both paths (a NaN cost takes candidate A), its neighbours untouched."""
    T, B, x0, C, c = headline
    x0 = x0.clone()
    x0[5, 0] = float("inf")
    _al, sv = check_solve(model("cartpole"), T, x0, C, c, 10)
    assert torch.isnan(sv.best_cost[5])
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[5] = False
    assert torch.isfinite(sv.best_cost[keep]).all()


@pytest.mark.parametrize("bounds", [(None, None), (-2.0, 2.0)])
@pytest.mark.parametrize("T", [3, 20])
def test_carry_pendulum(T, bounds):
    dx = model("pendulum")
    B = 65
    x0 = initial_states("pendulum", B, T)
    C, c = true_cost(dx, T, B)
    check_solve(dx, T, x0, C, c, 6, bounds=bounds, decay=0.2, mls=5)
    check_solve(dx, T, x0, C, c, 6, bounds=bounds, decay=0.5, mls=2)
