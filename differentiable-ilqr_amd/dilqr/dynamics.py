"""Generic dynamics modules of the reference (dynamics.py), for the MPC's
generic loop (dilqr.generic).

They are plain torch Modules — evaluated by torch on the GPU — with the
reference's constructor arguments, parameter layout (so its state dicts load)
and `grad_input` Jacobians.  The fused HIP kernels never see them: the MPC
routes any dynamics other than the env_dx models through dilqr.generic, whose
Riccati sweeps are the HIP kernel.  An NNDynamics with one hidden layer
(sigmoid or relu) also has a device model (`device_model`, csrc/dilqr_mlp.h):
dilqr.generic then runs its rollouts, ANALYTIC linearisation, line search and
whole solves through the HIP MLP kernels, which read the module's weights in
place, and the gradient of a solve reaches the weights through a HIP backward
of the linearisation (ops.mlp_linearize_diff, generic.DEVICE_MLP_VJP); any
other NNDynamics keeps the torch graph through grad_input (final_step).  One
with two hidden layers has a device model too (`device_model(like, deep=True)`,
csrc/dilqr_mlp2.h), used for the solve when generic.DEVICE_MLP_DEEP is on (it
ships off); its gradient goes through the torch graph unless
generic.DEVICE_MLP_DEEP_VJP (off too) is on and the first width is within
N.MLP2_VJP_MAX_HIDDEN1: then it is a HIP backward as well
(ops.mlp2_linearize_diff, csrc/tu_mlp2_vjp.hip).  Through mpc_explicit.MPC a
one-hidden-layer module gets the DiLQR implicit backward on its device model
(ops.mlp_implicit_step, csrc/tu_mlp_implicit.hip, generic.DEVICE_MLP_IMPLICIT);
one with two hidden layers and a first width within N.MLP2_IMPLICIT_MAX_HIDDEN1
does when generic.DEVICE_MLP_DEEP and generic.DEVICE_MLP_DEEP_IMPLICIT (off by
default) are on (csrc/tu_mlp2_implicit.hip).  A solve with a slew-rate penalty
wraps the module in CtrlPassthroughDynamics (below); with
generic.DEVICE_MLP_SLEW (off by default) that wrapper is a HIP model over the
device model (csrc/dilqr_ctrl_through.h, ops.slew_dynamics) and the solve stays
on device, and with generic.DEVICE_MLP_DELTA_U (off too) so does one with
delta_u.
"""
import torch
import torch.nn.functional as Fn
from torch import nn

from .generic import CtrlPassthroughDynamics  # noqa: F401  (dynamics.py:133-156)

ACTS = {"sigmoid": torch.sigmoid, "relu": Fn.relu, "elu": Fn.elu}


class NNDynamics(nn.Module):
    """dynamics.py:15-130: x' = MLP([x; u]) (+ x with passthrough)."""

    def __init__(self, n_state, n_ctrl, hidden_sizes=(100,), activation="sigmoid", passthrough=True):
        super().__init__()
        self.passthrough = passthrough
        sizes = list(hidden_sizes) + [n_state]
        fcs, in_sz = [], n_state + n_ctrl
        for out_sz in sizes:
            fcs.append(nn.Linear(in_sz, out_sz))
            in_sz = out_sz
        self.fcs = nn.ModuleList(fcs)
        if activation not in ACTS:
            raise ValueError(f"activation must be one of {sorted(ACTS)}")
        self.activation = activation
        self.acts = [ACTS[activation]] * (len(self.fcs) - 1) + [lambda z: z]
        self.zs = []

    @property
    def Ws(self):
        return [fc.weight for fc in self.fcs]

    def forward(self, x, u):
        x_dim, u_dim = x.ndimension(), u.ndimension()
        if x_dim == 1:
            x = x.unsqueeze(0)
        if u_dim == 1:
            u = u.unsqueeze(0)
        self.zs = []
        z = torch.cat((x, u), 1)
        for act, fc in zip(self.acts, self.fcs):
            z = act(fc(z))
            self.zs.append(z)
        self.zs = self.zs[:-1]            # the hidden activations (dynamics.py:82-83)
        if self.passthrough:
            z = z + x
        return z.squeeze(0) if x_dim == 1 else z

    def device_model(self, like, deep=False):
        """The network as the HIP MLP kernels take it (ops.MlpModel: sizes, flags
        and pointers to this module's own parameter storage — no copy, so an
        optimiser step is seen by the next solve), or None when the module is
        outside their envelope: more than one hidden layer, elu, a hidden width
        above N.MLP_MAX_HIDDEN, an (n, m) the one-lane kernels are not compiled
        for, parameters that are not fp32 / contiguous / 16-byte aligned, or
        parameters on another device than `like`.  With deep, a module with two
        hidden layers inside the same envelope (both widths) gives its
        ops.Mlp2Model (csrc/dilqr_mlp2.h); three or more still give None."""
        from . import _native as N
        from . import ops
        layers = len(self.fcs) - 1
        if layers not in ((1, 2) if deep else (1,)) or self.activation not in ("sigmoid", "relu"):
            return None
        params = [p for fc in self.fcs for p in (fc.weight, fc.bias)]
        d = params[0].shape[1]
        n = params[-2].shape[0]
        widths = [fc.weight.shape[0] for fc in self.fcs[:-1]]
        if (n, d - n) not in N.LANE_SHAPES or not all(1 <= H <= N.MLP_MAX_HIDDEN for H in widths):
            return None
        for p in params:
            if p is None or p.dtype != torch.float32 or not p.is_contiguous() or p.device != like.device \
                    or p.data_ptr() % 16:
                return None
        act = N.MLP_SIGMOID if self.activation == "sigmoid" else N.MLP_RELU
        make = ops.MlpModel if layers == 1 else ops.Mlp2Model
        return make(n, d - n, act, self.passthrough, *(p.detach() for p in params))

    def grad_input(self, x, u):
        """dynamics.py:92-130: R = d x'/d x, S = d x'/d u from the weights and the
        last forward's activations."""
        n_batch, n_state = x.size()
        diff = x.requires_grad or u.requires_grad
        Ws = self.Ws if diff else [W.detach() for W in self.Ws]
        zs = self.zs if diff else [z.detach() for z in self.zs]
        grad = Ws[-1].unsqueeze(0).repeat(n_batch, 1, 1)
        for i in range(len(zs) - 1, -1, -1):
            n_out, n_in = Ws[i].size()
            if self.activation == "relu":
                Wi = Ws[i].unsqueeze(0).repeat(n_batch, 1, 1)
                Wi = Wi * (zs[i] > 0.).to(Wi.dtype).unsqueeze(2)
            elif self.activation == "sigmoid":
                d = (zs[i] * (1. - zs[i])).unsqueeze(2).expand(n_batch, n_out, n_in)
                Wi = Ws[i].unsqueeze(0).repeat(n_batch, 1, 1) * d
            else:
                raise NotImplementedError("grad_input: relu and sigmoid only (as the reference)")
            grad = grad.bmm(Wi)
        R, S = grad[:, :, :n_state], grad[:, :, n_state:]
        if self.passthrough:
            R = R + torch.eye(n_state, dtype=R.dtype, device=R.device).unsqueeze(0)
        return R, S


class AffineDynamics(nn.Module):
    """dynamics.py:159-202: x' = A x + B u + c."""

    def __init__(self, A, B, c=None):
        super().__init__()
        assert A.ndimension() == 2 and B.ndimension() == 2
        self.A, self.B, self.c = A, B, c

    def forward(self, x, u):
        x_dim = x.ndimension()
        if x_dim == 1:
            x = x.unsqueeze(0)
        if u.ndimension() == 1:
            u = u.unsqueeze(0)
        z = x.mm(self.A.t()) + u.mm(self.B.t()) + (self.c if self.c is not None else 0.)
        return z.squeeze(0) if x_dim == 1 else z

    def grad_input(self, x, u):
        n_batch = x.size(0)
        return self.A.unsqueeze(0).repeat(n_batch, 1, 1), self.B.unsqueeze(0).repeat(n_batch, 1, 1)
