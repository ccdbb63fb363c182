"""LQRStep of DiLQR (lqr_step_explicit.py:24-718) on the HIP path.

`LQRStep(...)` returns a callable with the reference's signature
`apply(x_init, C, c, F, f=None, theta=None)`:

  * regular forward  -> (new_x, new_u, Tensor([n_total_qp_iter]), costs,
                         full_du_norm, mean_alphas)      (lqr_step_explicit.py:625-650)
  * no_op_forward    -> (current_x, current_u) with the Riccati gains of the
                         current trajectory saved for the implicit backward
                         (lqr_step_explicit.py:604-623)

The backward of the no-op step is the DiLQR implicit differentiation
(lqr_step_explicit.py:653-712) and returns (None, dC, dc, None, None,
dtheta [B,p], None); autograd sums dtheta over the batch like the reference.
"""
import torch
from torch.autograd import Function

from . import generic, ops


def _bounds_arg(v):
    if v is None or isinstance(v, (int, float)):
        return v
    return v.detach()


def LQRStep(n_state, n_ctrl, T, u_lower=None, u_upper=None, u_zero_I=None, delta_u=None,
            linesearch_decay=0.2, max_linesearch_iter=10, true_cost=None, true_dynamics=None,
            delta_space=True, current_x=None, current_u=None, verbose=0, back_eps=1e-3,
            no_op_forward=False, theta=None):
    if not delta_space:
        raise NotImplementedError("dilqr: delta_space=False is unimplemented in the reference too (639)")
    if delta_u is not None and u_lower is None:
        raise NotImplementedError("dilqr: delta_u without u_lower is unimplemented in the reference too (197)")
    lo, hi = _bounds_arg(u_lower), _bounds_arg(u_upper)
    zI = None if u_zero_I is None else u_zero_I.detach()

    class LQRStepFn(Function):
        @staticmethod
        def forward(ctx, x_init, C, c, F, f=None, theta=None, if_converge=False):
            assert current_x is not None and current_u is not None
            x, u = current_x.detach(), current_u.detach()
            if no_op_forward:
                K, _, _ = ops.delta_sweep(C, c, F, n_state, n_ctrl, x, u, lo, hi, zI, delta_u)
                ctx.save_for_backward(x_init, C, c, F, f, x, u, theta, K)
                ctx.model = true_dynamics
                return x.clone(), u.clone()
            # lqr_step_explicit.py:166-263: the shared step (sweep, then the line
            # search on device or with the user's Modules in torch)
            nx, nu, costs, full_du_norm, alphas, n_qp = generic.lqr_step_forward(
                T, n_state, n_ctrl, x_init, C, c, F, x, u, true_cost, true_dynamics, lo, hi, delta_u,
                linesearch_decay, max_linesearch_iter, u_zero_I=zI, extras=True, env_models=True)
            ctx.save_for_backward(x_init, C, c, F, f, nx, nu)
            return nx, nu, torch.tensor([float(n_qp)]), costs, full_du_norm, alphas.mean()

        @staticmethod
        def backward(ctx, dl_dx, dl_du, *unused):
            if len(ctx.saved_tensors) != 9:
                # the reference's backward unpacks 9 saved tensors and fails the
                # same way after a regular (non no-op) forward (656)
                raise RuntimeError("LQRStep backward needs a no_op_forward step (lqr_step_explicit.py:656)")
            from .implicit import implicit_backward
            x_init, C, c, F, f, x, u, th, K = ctx.saved_tensors
            dC, dc, dtheta = implicit_backward(ctx.model, dl_dx, dl_du, C, c, F, f, x, u, K, lo, hi, th)
            return None, dC, dc, None, None, dtheta, None

    return LQRStepFn.apply
