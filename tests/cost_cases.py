"""One definition of the cost cases the sweep and solve kernels choose a path
from (dilqr_fused.h cost_sym flags), shared by tests/golden/gen_golden.py
(case_costs) and the tests that use its goldens.

TEST INFRASTRUCTURE ONLY.  Nothing is stored as [T,B,d,d] arrays: costs and
sweep inputs are regenerated from numpy.random.RandomState seeds (the seeds are
in the golden files), every value rounded to float32 before use so that the
fp64 reference, the fp64 oracle and the fp32 kernels see identical inputs, and a
float64 checksum in the golden file is asserted before the arrays are used.

Base cost: C = diag(q) + L L^T, c = p + 0.01 N(0,1), L ~ (0.3/sqrt(d)) N(0,1),
q, p the model's true objective (test_solve_carry._costs' scale).  Classes, and
the cost_sym flag the single-lane solve kernels give each:
  tinv_diag   7  diag(q) and the c of t = 0, at every t
  diag_tv     3  diag(q) (1 + 0.1 U) per (t, b), c varying
  tinv_dense  5  the dense record of t = 0 at every t
  dense       1  dense symmetric, varying
  asym        0  dense + 0.05 (N - N^T) at every t
  asym_t0     0  dense, asymmetric at t = 0 only      (SYM form from T-1 down to 1)
  asym_mid    0  dense, asymmetric at t = T//2 only   (the switch mid-sweep)
  asym_last   0  dense, asymmetric at t = T-1 only    (never the SYM form)
The 16-lane rocket kernels know two values only: 7 (tinv_diag) and 0.
"""
import numpy as np

CLASSES = ("tinv_diag", "diag_tv", "tinv_dense", "dense", "asym", "asym_t0", "asym_mid", "asym_last")
FLAGS = (7, 3, 5, 1, 0, 0, 0, 0)
ASYM = ("asym", "asym_t0", "asym_mid", "asym_last")


def classes_of(B):
    """Interleaved: problem b has class b % 8 (every wave holds every path)."""
    return [CLASSES[b % len(CLASSES)] for b in range(B)]


def flags_of(classes, rocket=False):
    f = np.array([FLAGS[CLASSES.index(k)] for k in classes])
    return np.where(f == 7, 7, 0) if rocket else f


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def checksum(*arrays):
    """A float64 position-weighted sum (a transposed or shifted array changes it)."""
    tot = 0.0
    for a in arrays:
        a = np.asarray(a, np.float64).ravel()
        tot += float(np.dot(a, np.cos(0.37 * np.arange(a.size) + 0.1)))
    return np.array(tot)


def check(stored, *arrays):
    got = float(checksum(*arrays))
    assert abs(got - float(stored)) <= 1e-9 * max(1.0, abs(float(stored))), (got, float(stored))


def make_costs(q, p, n, T, classes, seed, sym_uu=False, L_scale=0.3):
    """C [T,B,d,d], c [T,B,d] as float64 arrays of float32 values.  sym_uu: the
    antisymmetric part leaves the C_uu block alone (bounded problems with
    m > 1: pnqp on an asymmetric H is not a descent method)."""
    q, p = f32(q), f32(p)
    d, B = q.shape[0], len(classes)
    rng = np.random.RandomState(seed)            # every draw is made whatever the classes are
    L = rng.normal(size=(T, B, d, d)) * (L_scale / np.sqrt(d))
    cn = p + 0.01 * rng.normal(size=(T, B, d))
    U = rng.uniform(size=(T, B))
    Nn = rng.normal(size=(T, B, d, d))
    A = 0.05 * (Nn - np.swapaxes(Nn, -1, -2))
    if sym_uu:
        A[..., n:, n:] = 0.0
    dense = np.diag(q) + L @ np.swapaxes(L, -1, -2)
    dense = np.triu(dense) + np.swapaxes(np.triu(dense, 1), -1, -2)      # symmetric bit for bit
    C = np.empty((T, B, d, d))
    c = np.empty((T, B, d))
    for b, kind in enumerate(classes):
        if kind == "tinv_diag":
            C[:, b], c[:, b] = np.diag(q), cn[0, b]
        elif kind == "diag_tv":
            C[:, b] = np.diag(q) * (1.0 + 0.1 * U[:, b, None, None])
            c[:, b] = cn[:, b]
        elif kind == "tinv_dense":
            C[:, b], c[:, b] = dense[0, b], cn[0, b]
        else:
            C[:, b], c[:, b] = dense[:, b], cn[:, b]
            ts = {"dense": [], "asym": range(T), "asym_t0": [0], "asym_mid": [T // 2], "asym_last": [T - 1]}[kind]
            for t in ts:
                C[t, b] += A[t, b]
    return f32(C), f32(c)


# the sweep fixtures: name -> (n, m, model whose true objective gives q, p)
SWEEP_SHAPES = {"s31": (3, 1, "pendulum"), "s51": (5, 1, "cartpole"), "s42": (4, 2, None), "s43": (4, 3, None),
                "s133": (13, 3, "rocket")}
SWEEP_T, SWEEP_B, SWEEP_BOX = 9, 16, 0.5
SWEEP_MODES = {name: ("unc", "box") + (("chol",) if m == 3 else ()) for name, (n, m, _) in SWEEP_SHAPES.items()}


def sweep_objective(name, true_obj):
    """q, p of a sweep shape; true_obj(model_name) -> (q, p)."""
    n, m, mname = SWEEP_SHAPES[name]
    if mname is not None:
        return true_obj(mname)
    d = n + m
    return 0.5 + 0.1 * np.arange(d), -0.1 * np.cos(np.arange(d))


def sweep_problem(name, true_obj, seed):
    """The fixture of one sweep shape: F, x, u and the two cost sets (asymmetry
    in C_uu too, for the unconstrained modes; C_uu symmetric, for the box)."""
    n, m, _ = SWEEP_SHAPES[name]
    T, B = SWEEP_T, SWEEP_B
    q, p = sweep_objective(name, true_obj)
    cls = classes_of(B)
    rng = np.random.RandomState(seed + 1000)
    F = np.concatenate([np.eye(n) + 0.05 * rng.normal(size=(T - 1, B, n, n)),
                        0.1 * rng.normal(size=(T - 1, B, n, m))], -1)
    x = 0.5 * rng.normal(size=(T, B, n))
    u = rng.uniform(-0.4, 0.4, (T, B, m))
    C, c = make_costs(q, p, n, T, cls, seed)
    Cb, cb = (C, c) if m == 1 else make_costs(q, p, n, T, cls, seed, sym_uu=True)
    return dict(n=n, m=m, classes=cls, F=f32(F), x=f32(x), u=f32(u), C=C, c=c, C_box=Cb, c_box=cb)


# the MPC fixtures: name -> (model, T, Bf, lqr_iter, bounds, decay, max_ls, mixed classes?)
MPC_CASES = {
    "cart_mixed_unc": ("cartpole", 25, 40, 10, None, 0.5, 2, True),
    "cart_mixed_box10": ("cartpole", 25, 40, 10, (-10.0, 10.0), 0.5, 2, True),
    "pend_mixed_box": ("pendulum", 10, 40, 10, (-2.0, 2.0), 0.2, 5, True),
    "rocket_dense_unc": ("rocket", 30, 16, 10, None, 0.2, 5, True),
    "rocket_dense_box20": ("rocket", 30, 16, 10, (-20.0, 20.0), 0.2, 5, True),
    "rocket_diag_it10": ("rocket", 30, 16, 10, (-20.0, 20.0), 0.2, 5, False),    # bench config 3's settings
}


def mpc_classes(name):
    Bf, mixed = MPC_CASES[name][2], MPC_CASES[name][7]
    return classes_of(Bf) if mixed else None


def mpc_costs(name, true_obj, seed):
    """(C, c) of an MPC fixture; the unmixed case is the true diagonal objective."""
    mname, T, Bf, _it, bounds, _d, _m, mixed = MPC_CASES[name]
    q, p = true_obj(mname)
    n = {"cartpole": 5, "pendulum": 3, "rocket": 13}[mname]
    if not mixed:
        q, p = f32(q), f32(p)
        return (np.ascontiguousarray(np.broadcast_to(np.diag(q), (T, Bf) + (q.size,) * 2)),
                np.ascontiguousarray(np.broadcast_to(p, (T, Bf, p.size))))
    return make_costs(q, p, n, T, classes_of(Bf), seed, sym_uu=bounds is not None and q.size - n > 1)


def tile(a, B, axis=1):
    """Device batch from a fixture: problem b is fixture problem b % Bf."""
    a = np.asarray(a)
    return np.take(a, np.arange(B) % a.shape[axis], axis=axis)


# ---------------------------------------------------------------- the implicit backward's cost paths
# k_implicit_backward (one lane per problem) and the rocket group kernel (one
# lane per row of C) scan C and c bit by bit in their first pass: c_offd (an
# off-diagonal word that is not +0.0), c_dif (a diagonal word unlike step
# T-1's), cv_dif (a word of c unlike step T-1's); the last pass then takes C
# (c) from registers when c_offd = c_dif = 0 (cv_dif = 0).  The eight classes
# above reach three of the four combinations; the backward-only classes below,
# built from the same draws, aim at one branch of that detection each:
#   diag_cvar  diag(q) at every t, c varying per t        C from registers, c re-read
#   diag_t0    diag(q), 1.1 diag(q) at t = 0, c constant   c_dif set by the last step the scan visits
#   c_t0       diag(q), c differs at t = 0 only            cv_dif likewise
#   pair_t0    diag(q) + one symmetric state-control pair C[i,n] = C[n,i] = 0.1
#              at t = 0, c constant                        c_offd from a single word (rocket: rows i, n only)
# No output of the backward depends on C_0, c_0 in the last pass (lam_0 and
# dlam_0 feed only the gradient to x_init, which LQRStep does not return), so
# the kernels' results on the *_t0 classes are the same whether or not the scan
# sees step 0 and whichever path the last pass then takes: on the device they
# detect nothing that tinv_diag does not, and only the numpy path_bits test
# pins what they are.  The *_mid classes make the same kind of change at
# t = T//2, where it reaches every earlier step's costate (c_mid moves c by
# C_MID_GAIN times the difference of two draws, 0.7 sigma, so that the change
# is not lost next to C tau).
BACKWARD_EXTRA = ("diag_cvar", "diag_t0", "c_t0", "pair_t0")
BACKWARD_MID = ("diag_mid", "c_mid", "pair_mid")
BACKWARD_CLASSES = CLASSES + BACKWARD_EXTRA + BACKWARD_MID
PAIR_VALUE, DIAG_SCALE, C_MID_GAIN = 0.1, 1.1, 50.0
# pair_mid's value is PAIR_MID_FRAC sqrt(q_i q_n): 0.1 next to cartpole's control
# weight 0.001 makes the stage cost indefinite, harmless at t = 0 where x_0 is
# fixed, not at a step whose state is free
PAIR_MID_FRAC = 0.5
# the pair is (state PAIR_STATE[n], control 0): a velocity (pendulum, cartpole: the
# angular rate; rocket: v_z), whose costate reaches dtheta within one step; a
# position's costate feeds no Hessian or parameter term of its own step
PAIR_STATE = {3: 2, 5: 4, 13: 5}
# (c_offd, c_dif, cv_dif) a bitwise scan sets, per class
PATH_BITS = {"tinv_diag": (0, 0, 0), "diag_tv": (0, 1, 1), "tinv_dense": (1, 0, 0), "dense": (1, 1, 1),
             "asym": (1, 1, 1), "asym_t0": (1, 1, 1), "asym_mid": (1, 1, 1), "asym_last": (1, 1, 1),
             "diag_cvar": (0, 0, 1), "diag_t0": (0, 1, 0), "c_t0": (0, 0, 1), "pair_t0": (1, 0, 0),
             "diag_mid": (0, 1, 0), "c_mid": (0, 0, 1), "pair_mid": (1, 0, 0)}


def backward_classes_of(B, shift=0):
    """Problem b has class (b + shift) % 15."""
    return [BACKWARD_CLASSES[(b + shift) % len(BACKWARD_CLASSES)] for b in range(B)]


def make_backward_costs(q, p, n, T, classes, seed, sym_uu=False):
    """make_costs for a list drawn from BACKWARD_CLASSES.  The eight classes of
    CLASSES are make_costs' own; a backward-only class is built here from
    make_costs' draw of c (its "diag_tv" c is the rounded draw itself)."""
    assert T >= 2
    base = [k if k in CLASSES else "diag_tv" for k in classes]
    C, c = make_costs(q, p, n, T, base, seed, sym_uu=sym_uu)
    Dq = np.diag(f32(q))
    for b, kind in enumerate(classes):
        if kind in CLASSES:
            continue
        cn = c[:, b].copy()
        ts = T // 2 if kind.endswith("_mid") else 0
        C[:, b] = Dq
        if kind == "diag_cvar":
            c[:, b] = cn
        elif kind in ("diag_t0", "diag_mid"):
            C[ts, b] = f32(DIAG_SCALE * Dq)
            c[:, b] = cn[0]
        elif kind in ("c_t0", "c_mid"):
            if ts == 0:
                c[:, b], c[0, b] = cn[T - 1], cn[0]
            else:
                c[:, b], c[ts, b] = cn[0], f32(cn[0] + C_MID_GAIN * (cn[ts] - cn[0]))
        elif kind in ("pair_t0", "pair_mid"):
            i = PAIR_STATE[n]
            C[ts, b, i, n] = C[ts, b, n, i] = f32(PAIR_VALUE if ts == 0 else PAIR_MID_FRAC * np.sqrt(Dq[i, i] * Dq[n, n]))
            c[:, b] = cn[0]
        else:
            raise KeyError(kind)
    return C, c


def path_bits(C, c):
    """What the kernels' scan sets, in numpy on the float32 bit patterns: per
    problem and per row of C, (c_offd, c_dif, cv_dif) as bool [B, d, 3].  The
    one-lane kernel ORs a problem's rows; the rocket kernel decides per row."""
    Cw = np.ascontiguousarray(C, dtype=np.float32).view(np.uint32)
    cw = np.ascontiguousarray(c, dtype=np.float32).view(np.uint32)
    d = Cw.shape[-1]
    offd = (Cw * (1 - np.eye(d, dtype=np.uint32))).any(axis=(0, 3))
    dg = np.diagonal(Cw, axis1=2, axis2=3)
    return np.stack([offd, (dg != dg[-1]).any(0), (cw != cw[-1]).any(0)], -1)


def per_problem(a, ref, axis):
    """max|a - ref| over each problem's entries / max|ref| over the same entries
    (not the whole array's relerr: a problem with a small gradient does not
    hide behind its neighbours).  axis: the batch axis.  Returns [B]."""
    a, ref = np.moveaxis(np.asarray(a, np.float64), axis, 0), np.moveaxis(np.asarray(ref, np.float64), axis, 0)
    B = ref.shape[0]
    err = np.abs(a - ref).reshape(B, -1).max(1)
    return err / np.maximum(np.abs(ref).reshape(B, -1).max(1), 1e-300)


# the implicit-backward fixtures of tests/golden/implicit_costs_f64.npz (gen_golden.py
# case_implicit_costs): T = 10, one problem of each of BACKWARD_CLASSES, in that order
IMPLICIT_COSTS_T = 10
IMPLICIT_COSTS = {"cart_unc": "cartpole", "cart_box": "cartpole", "pend_box": "pendulum", "rock_unc": "rocket",
                  "rock_box": "rocket"}
STATES = {"cartpole": 5, "pendulum": 3, "rocket": 13}


def implicit_costs_problem(g, tag, true_obj):
    """One fixture as float64 arrays of float32 values: the costs regenerated
    from the stored seed (checksum asserted), the reference's solution, the loss
    weights, the bounds (None, None if unconstrained) and the expected dC, dc,
    per-problem dtheta."""
    mname = IMPLICIT_COSTS[tag]
    q, p = true_obj(mname)
    n = STATES[mname]
    m = q.size - n
    w = float(g[f"{tag}_width"])
    lo, hi = (-w, w) if w > 0 else (None, None)
    cls = [str(k) for k in g["classes"]]
    assert tuple(cls) == BACKWARD_CLASSES
    C, c = make_backward_costs(q, p, n, IMPLICIT_COSTS_T, cls, int(g[f"{tag}_seed"]), sym_uu=w > 0 and m > 1)
    check(g[f"{tag}_sum"], C, c)
    return dict(mname=mname, n=n, m=m, T=IMPLICIT_COSTS_T, classes=cls, C=C, c=c, lo=lo, hi=hi,
                **{k: g[f"{tag}_{k}"] for k in ("x0", "x", "u", "wx", "wu", "dQ", "dP", "dtheta", "pinned")})
