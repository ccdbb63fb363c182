"""A numpy model of the one-hidden-layer NNDynamics for the oracle, and the
DiLQR implicit backward on it (test infrastructure; imported by
test_mlp_implicit_cpu.py and test_mlp_implicit_gpu.py).

MlpOracle has the interface oracle.mpc / oracle.adjoint ask of a model:
forward, get_linear_dyn, n_params and grad_input.  grad_input returns explicit
partials only,
  (dF/dtheta, df/dtheta - dF/dtheta . tau, dF/dx, dF/du, F, -dF/dx . tau, -dF/du . tau),
and ignores the gains: none of the env_dx models' quirks belong to a network.
theta = [W1 (H*d), b1 (H), W2 (n*H), b2 (n)].  Everything computes in the
dtype of the weights, so the same code run in float32 measures what the number
format alone costs (the `ref_spread` convention of tests/test_gpu_parity.py).
"""
import numpy as np

from oracle import adjoint, lqr


class MlpOracle:
    def __init__(self, W1, b1, W2, b2, activation="sigmoid", passthrough=True):
        self.W1, self.b1, self.W2, self.b2 = (np.asarray(a) for a in (W1, b1, W2, b2))
        self.act, self.pt = activation, bool(passthrough)
        self.H, self.d = self.W1.shape
        self.n = self.W2.shape[0]
        self.m = self.d - self.n
        self.n_params = self.H * self.d + self.H + self.n * self.H + self.n

    def astype(self, dt):
        return MlpOracle(*(a.astype(dt) for a in (self.W1, self.b1, self.W2, self.b2)), self.act, self.pt)

    def with_theta(self, th):
        H, d, n = self.H, self.d, self.n
        o = np.cumsum([0, H * d, H, n * H, n])
        return MlpOracle(th[o[0]:o[1]].reshape(H, d), th[o[1]:o[2]], th[o[2]:o[3]].reshape(n, H), th[o[3]:o[4]],
                         self.act, self.pt)

    def theta(self):
        return np.concatenate([a.ravel() for a in (self.W1, self.b1, self.W2, self.b2)])

    def hidden(self, tau):
        """a = act(z), g = act'(z), h = act''(z) at z = W1 tau + b1, rows [R, H]."""
        z = tau @ self.W1.T + self.b1
        if self.act == "relu":
            a = np.maximum(z, 0)
            return a, (a > 0).astype(z.dtype), np.zeros_like(z)     # the relu mask carries no gradient
        a = 1 / (1 + np.exp(-z))
        g = a * (1 - a)
        return a, g, g * (1 - 2 * a)

    def forward(self, x, u, params=None):
        a, _, _ = self.hidden(np.concatenate([x, u], -1))
        o = a @ self.W2.T + self.b2
        return o + x if self.pt else o

    def get_linear_dyn(self, x, u, params=None):
        _, g, _ = self.hidden(np.concatenate([x, u], -1))
        J = np.einsum("ij,rj,jk->rik", self.W2, g, self.W1)
        if self.pt:
            J[:, :, :self.n] += np.eye(self.n, dtype=J.dtype)
        return J

    def lag_hess(self, x, u, lam):
        """M = sum_i lam_i d^2 f_i / d tau^2 = W1^T diag((W2^T lam) act'') W1, rows [R, d, d]."""
        _, _, h = self.hidden(np.concatenate([x, u], -1))
        return np.einsum("rj,jk,jl->rkl", (lam @ self.W2) * h, self.W1, self.W1)

    def grad_input(self, new_x, new_u, K=None, params=None):
        T, B, n = new_x.shape
        d, H, p = self.d, self.H, self.n_params
        tau = np.concatenate([new_x, new_u], -1)[:-1].reshape(-1, d)
        R = tau.shape[0]
        a, g, h = self.hidden(tau)
        W1, W2 = self.W1, self.W2
        dt = W1.dtype
        oW1, ob1, oW2, ob2 = 0, H * d, H * d + H, H * d + H + n * H
        gD = np.zeros((R, n, d, p), dt)               # dF_ik / dtheta
        gf = np.zeros((R, n, p), dt)                  # d f(tau)_i / dtheta (the value)
        t1 = np.zeros((R, n, d, H, d), dt)            # / dW1_jl
        for k in range(d):
            t1[:, :, k, :, k] += W2[None] * g[:, None, :]
        t1 += np.einsum("ij,rj,jk,rl->rikjl", W2, h, W1, tau)
        gD[..., oW1:ob1] = t1.reshape(R, n, d, H * d)
        gD[..., ob1:oW2] = np.einsum("ij,rj,jk->rikj", W2, h, W1)
        t2 = np.zeros((R, n, d, n, H), dt)            # / dW2_qj
        for i in range(n):
            t2[:, i, :, i, :] = np.einsum("rj,jk->rkj", g, W1)
        gD[..., oW2:ob2] = t2.reshape(R, n, d, n * H)
        gf[..., oW1:ob1] = np.einsum("ij,rj,rl->rijl", W2, g, tau).reshape(R, n, H * d)
        gf[..., ob1:oW2] = W2[None] * g[:, None, :]
        t3 = np.zeros((R, n, n, H), dt)
        for i in range(n):
            t3[:, i, i, :] = a
        gf[..., oW2:ob2] = t3.reshape(R, n, n * H)
        gf[..., ob2:] = np.eye(n, dtype=dt)
        gd = gf - np.einsum("rikp,rk->rip", gD, tau)
        Dtau = np.einsum("ij,rj,jk,jl->rikl", W2, h, W1, W1)       # dF_ik / dtau_l
        D = self.get_linear_dyn(tau[:, :n], tau[:, n:])
        dtau = -np.einsum("rikl,rk->ril", Dtau, tau)
        sh = lambda z: z.reshape((T - 1, B) + z.shape[1:])         # noqa: E731
        return (sh(gD), sh(gd), sh(Dtau[..., :n]), sh(Dtau[..., n:]), sh(D), sh(dtau[..., :n]), sh(dtau[..., n:]))

    def param_vjp(self, x, u, gF, gf):
        """The weight gradient of the linearisation (F_t, f_t = f(tau_t) - F_t
        tau_t, t < T-1) for cotangents gF [T-1,B,n,d], gf [T-1,B,n], summed over
        (t, b): (dW1, db1, dW2, db2) — the formulas of csrc/tu_mlp_vjp.hip."""
        d, n = self.d, self.n
        tau = np.concatenate([x, u], -1)[:-1].reshape(-1, d)
        a, g, h = self.hidden(tau)
        o = gf.reshape(-1, n)
        Gb = gF.reshape(-1, n, d) - o[:, :, None] * tau[:, None, :]
        r = np.einsum("rik,jk->rij", Gb, self.W1)
        q = np.einsum("ij,rik->rjk", self.W2, Gb)
        p = o @ self.W2
        s = np.einsum("ij,rij->rj", self.W2, r)
        zh = g * p + h * s
        dW1 = np.einsum("rj,rjk->jk", g, q) + zh.T @ tau
        dW2 = o.T @ a + np.einsum("rj,rij->ij", g, r)
        return dW1, zh.sum(0), dW2, o.sum(0)


def costates(model, C, c, F, x, u):
    """lam_t = Cxx x + Cxu u + c_x + F_x^T lam_{t+1} (lqr_step_explicit.py:305-319), [T,B,n]."""
    T, B, n = x.shape
    lams = [None] * T
    prev = None
    for t in range(T - 1, -1, -1):
        lam = lqr.bmv(C[t, :, :n, :n], x[t]) + lqr.bmv(C[t, :, :n, n:], u[t]) + c[t, :, :n]
        if prev is not None:
            lam = lam + lqr.bmv(np.swapaxes(F[t, :, :, :n], 1, 2), prev)
        lams[t] = prev = lam
    return np.stack(lams)


def implicit_oracle(model, dl_dx, dl_du, C, c, x, u, u_lower=None, u_upper=None):
    """The DiLQR implicit backward at (x, u) by the algebra of
    oracle.adjoint.implicit_backward_fast, with every output the device kernel
    has: (dx_init [B,n], dC, dc, dF [T-1,B,n,d], df [T-1,B,n]).  Runs in the
    dtype of its inputs."""
    T, B, n = x.shape
    m = u.shape[2]
    d = n + m
    dt = C.dtype
    g = np.concatenate([dl_dx, dl_du], 2)
    I = adjoint._active_set(u, u_lower, u_upper)
    F = model.get_linear_dyn(x[:-1].reshape(-1, n), u[:-1].reshape(-1, m)).reshape(T - 1, B, n, d)
    lam = costates(model, C, c, F, x, u)
    M = np.zeros((T, B, d, d), dt)
    for t in range(T - 1):
        M[t] = model.lag_hess(x[t], u[t], lam[t + 1])
    y = adjoint.adjoint_lqr_linear(C + np.swapaxes(M, 2, 3), g, F, n, m, I)
    w = g - np.einsum("tbjk,tbj->tbk", M, y)
    tau = np.concatenate([x, u], 2)
    dC = -0.5 * (y[..., :, None] * tau[..., None, :] + tau[..., :, None] * y[..., None, :])
    dc = -y
    dlam = [None] * T
    prev = None
    for t in range(T - 1, -1, -1):
        dl = lqr.bmv(C[t, :, :n, :n], y[t, :, :n]) + lqr.bmv(C[t, :, :n, n:], y[t, :, n:]) - w[t, :, :n]
        if prev is not None:
            dl = dl + lqr.bmv(np.swapaxes(F[t, :, :, :n], 1, 2), prev)
        dlam[t] = prev = dl
    dlam = np.stack(dlam)
    dF = -(dlam[1:, :, :, None] * tau[:-1, :, None, :] + lam[1:, :, :, None] * y[:-1, :, None, :])
    df = -dlam[1:]
    return -dlam[0], dC, dc, dF.astype(dt), df


def cast(dt, *arrays):
    return tuple(None if a is None else (a if np.ndim(a) == 0 else np.asarray(a, dt)) for a in arrays)


def err32(model, dl_dx, dl_du, C, c, x, u, lo, hi, extra=None):
    """(fp64 outputs, relative error of the same oracle in float32 per output):
    max |o32 - o64| / max |o64|.  extra(model, x, u, outputs) -> tuple of more
    outputs to carry through both precisions (the weight gradients)."""
    out = {}
    for dt in (np.float64, np.float32):
        md = model.astype(dt)
        args = cast(dt, dl_dx, dl_du, C, c, x, u)
        o = implicit_oracle(md, *args, lo, hi)
        if extra is not None:
            o = o + tuple(extra(md, args[4], args[5], o))
        out[dt] = o
    rel = [float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0
           for a, b in zip(out[np.float32], out[np.float64])]
    return out[np.float64], rel
