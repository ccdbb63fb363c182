"""A numpy model of the two-hidden-layer NNDynamics for the oracle of the DiLQR
implicit backward (test infrastructure; imported by test_mlp2_implicit_cpu.py
and test_mlp2_implicit_gpu.py).

Mlp2Oracle has what tests/mlp_oracle.py's implicit_oracle, costates and err32
ask of a model: forward, get_linear_dyn, lag_hess, astype and n, m, d.  With
  z1 = W1 tau + b1, z2 = W2 a(z1) + b2, x' = W3 a(z2) + b3 (+ x),
  g = a'(z), c = a''(z), P = W2 diag(g1) W1, s = W3^T lam, v = W2^T (s o g2):
  F = W3 diag(g2) P (+ I on the state block)
  M = sum_i lam_i d^2 f_i / d tau^2 = P^T diag(s o c2) P + W1^T diag(v o c1) W1
(relu: c = 0, M = 0; the relu mask carries no gradient).  Everything computes
in the dtype of the weights, so the same code run in float32 measures what the
number format alone costs.

weight_vjp is the weight-gradient reference: the oracle's (dF, df) contracted
with torch autograd of a CPU copy of the module's linearisation (F = [R S] from
grad_input, f = f(tau) - F tau) in the model's dtype, the reference of
tests/test_mlp2_vjp_gpu.py for the same six parameters.
"""
import numpy as np


class Mlp2Oracle:
    def __init__(self, W1, b1, W2, b2, W3, b3, activation="sigmoid", passthrough=True):
        self.W1, self.b1, self.W2, self.b2, self.W3, self.b3 = (np.asarray(a) for a in (W1, b1, W2, b2, W3, b3))
        self.act, self.pt = activation, bool(passthrough)
        self.H1, self.d = self.W1.shape
        self.H2 = self.W2.shape[0]
        self.n = self.W3.shape[0]
        self.m = self.d - self.n

    def weights(self):
        return self.W1, self.b1, self.W2, self.b2, self.W3, self.b3

    def astype(self, dt):
        return Mlp2Oracle(*(a.astype(dt) for a in self.weights()), self.act, self.pt)

    def with_weights(self, ws):
        return Mlp2Oracle(*ws, self.act, self.pt)

    def _act(self, z):
        """a = act(z), g = act'(z), c = act''(z)."""
        if self.act == "relu":
            a = np.maximum(z, 0)
            return a, (a > 0).astype(z.dtype), np.zeros_like(z)
        a = 1 / (1 + np.exp(-z))
        g = a * (1 - a)
        return a, g, g * (1 - 2 * a)

    def hidden(self, tau):
        """(z1, a1, g1, c1), (z2, a2, g2, c2) for rows tau [R, d]."""
        z1 = tau @ self.W1.T + self.b1
        l1 = (z1,) + self._act(z1)
        z2 = l1[1] @ self.W2.T + self.b2
        return l1, (z2,) + self._act(z2)

    def forward(self, x, u, params=None):
        _, (_, a2, _, _) = self.hidden(np.concatenate([x, u], -1))
        o = a2 @ self.W3.T + self.b3
        return o + x if self.pt else o

    def tangent(self, g1):
        """P = W2 diag(g1) W1, rows [R, H2, d]."""
        return np.einsum("lj,rj,jk->rlk", self.W2, g1, self.W1)

    def get_linear_dyn(self, x, u, params=None):
        (_, _, g1, _), (_, _, g2, _) = self.hidden(np.concatenate([x, u], -1))
        J = np.einsum("il,rl,rlk->rik", self.W3, g2, self.tangent(g1))
        if self.pt:
            J[:, :, :self.n] += np.eye(self.n, dtype=J.dtype)
        return J

    def lag_hess(self, x, u, lam, first=True, second=True):
        """M [R, d, d]; first / second leave a term out (the tests measure what each is worth)."""
        (_, _, g1, c1), (_, _, g2, c2) = self.hidden(np.concatenate([x, u], -1))
        P = self.tangent(g1)
        s = lam @ self.W3
        v = (s * g2) @ self.W2
        M = np.zeros((P.shape[0], self.d, self.d), P.dtype)
        if first:
            M = M + np.einsum("rl,rlk,rlq->rkq", s * c2, P, P)
        if second:
            M = M + np.einsum("rj,jk,jq->rkq", v * c1, self.W1, self.W1)
        return M


def torch_module(model):
    """The NNDynamics with the oracle's weights, on the CPU in their dtype."""
    import torch
    from dilqr.dynamics import NNDynamics
    dx = NNDynamics(model.n, model.m, hidden_sizes=[model.H1, model.H2], activation=model.act, passthrough=model.pt)
    dx = dx.to(torch.float64 if model.W1.dtype == np.float64 else torch.float32)
    with torch.no_grad():
        for p, w in zip((q for fc in dx.fcs for q in (fc.weight, fc.bias)), model.weights()):
            p.copy_(torch.from_numpy(np.ascontiguousarray(w)))
    return dx


def weight_vjp(model, x, u, dF, df):
    """(dW1, db1, dW2, db2, dW3, db3): the gradient of sum(F . dF) + sum(f . df) over the rows
    t < T-1 by torch autograd through the module's forward and grad_input, in the model's dtype."""
    import torch
    T, B, n = x.shape
    dx = torch_module(model)
    if T < 2:
        return tuple(np.zeros(tuple(p.shape), model.W1.dtype) for fc in dx.fcs for p in (fc.weight, fc.bias))
    dt = next(dx.parameters()).dtype
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)                  # noqa: E731
    xs = t(x[:-1].reshape(-1, n)).requires_grad_(True)           # grad_input's differentiable branch
    us = t(u[:-1].reshape(-1, model.m)).requires_grad_(True)
    new_x = dx(xs, us)
    R, S = dx.grad_input(xs, us)
    F = torch.cat((R, S), 2)
    f = new_x - (F @ torch.cat((xs, us), 1).unsqueeze(-1)).squeeze(-1)
    ((F * t(dF.reshape(-1, n, model.d))).sum() + (f * t(df.reshape(-1, n))).sum()).backward()
    return tuple(p.grad.detach().numpy().copy() for fc in dx.fcs for p in (fc.weight, fc.bias))


def extra_weights(md, x, u, o):
    """err32's `extra`: the six weight gradients from the oracle's (dF, df) = o[3], o[4]."""
    return weight_vjp(md, x, u, o[3], o[4])
