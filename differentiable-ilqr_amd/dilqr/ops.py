"""Functional layer over the C-ABI: allocate outputs, launch on the current
stream.  Every function here is one (or a few) libdilqr.so calls; nothing
computes on the host.

What the kernels take for a dynamics is resolved in one place: a Dynamics
handle (model id, (n, m), and theta / F, f / the MLP descriptor), made by
device_dynamics from a dynamics object or by Dynamics.of from the public
functions' (model_id, theta, F, f).  Its three launches (rollout, linearise,
line search) are the only call sites of those entry points; rollout,
linearize, mlp_*, lqr_forward and mpc_solve_unfused all go through them.  A
network under MPC's slew-rate penalty is one more handle (slew_dynamics: the
control-passthrough model over the network, its own family of entry points),
with slew_problem building the augmented problem it solves.

A network is an MlpModel (one hidden layer) or an Mlp2Model (two).  Both take
their validation from _NetModel and differ in what a kind declares: the prefix
of its entry points, its descriptor, its widths.  The public mlp_* / mlp2_*
pairs (linearize_vjp, linearize_diff) keep their own refusals over one
implementation (_linearize_vjp, _LinearizeDiff, Dynamics.linearize_vjp).
"""
import collections
import os

import torch

from . import _native as N


def _f32(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"dilqr computes in fp32; got {t.dtype}")
    return t.detach().contiguous()


class _NetModel:
    """What every kind of network model shares: the validation of (n, m), the
    widths and the weights (W, b per layer in torch's nn.Linear layouts, the
    expected shapes derived from the widths), the descriptor over the module's
    own parameter storage (nothing is copied) and the tensors that keep its
    pointers alive.  A kind gives entry (the prefix of its entry points:
    entry + "rollout_f32", ...), Desc (its descriptor: the widths, the flags,
    the pointers) and the two texts its errors quote."""
    model_id = N.MODEL_MLP

    def __init__(self, n, m, activation, passthrough, *tensors):
        widths = tuple(W.shape[0] for W in tensors[:-2:2])
        if (n, m) not in N.LANE_SHAPES or not all(1 <= H <= N.MLP_MAX_HIDDEN for H in widths):
            raise ValueError(f"dilqr: no MLP kernels for (n, m) = {(n, m)}, {self.width_names} = "
                             f"{widths[0] if len(widths) == 1 else widths}")
        sizes = (n + m,) + widths + (n,)
        shapes = tuple(s for fan_in, fan_out in zip(sizes, sizes[1:]) for s in ((fan_out, fan_in), (fan_out,)))
        if tuple(tuple(t.shape) for t in tensors) != shapes:
            raise ValueError(f"dilqr: MLP weights must be {self.layout}")
        for t in tensors:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != tensors[0].device or t.data_ptr() % 16:
                raise ValueError("dilqr: MLP weights must be fp32, contiguous, 16-byte aligned, on one device")
        self.n, self.m, self.widths, self.device, self.tensors = n, m, widths, tensors[0].device, tensors
        self.desc = self.Desc(*widths, int(activation), int(bool(passthrough)), *(t.data_ptr() for t in tensors))

    def check(self, x, u):
        """x [..., n], u [..., m] on the weights' device (the kernels index rows by n and m)."""
        if x.shape[-1] != self.n or u.shape[-1] != self.m or x.shape[:-1] != u.shape[:-1]:
            raise ValueError(f"dilqr: MLP model is (n, m) = {(self.n, self.m)}; got x {tuple(x.shape)}, "
                             f"u {tuple(u.shape)}")
        if x.device != self.device or u.device != self.device:
            raise RuntimeError("dilqr: MLP weights and inputs are on different devices")


class MlpModel(_NetModel):
    """A one-hidden-layer network as the dilqr_mlp_* entry points take it: the
    dilqr_mlp descriptor plus (n, m), H and the tensors.  Built by
    NNDynamics.device_model; passed to lqr_forward / mpc_solve_unfused in place
    of (model_id, theta)."""
    entry, Desc = "dilqr_mlp_", N.Mlp
    width_names, layout = "H", "W1 [H,n+m], b1 [H], W2 [n,H], b2 [n]"

    def __init__(self, n, m, activation, passthrough, W1, b1, W2, b2):
        super().__init__(n, m, activation, passthrough, W1, b1, W2, b2)
        self.H, = self.widths


class Mlp2Model(_NetModel):
    """A two-hidden-layer network as the dilqr_mlp2_* entry points take it
    (csrc/dilqr_mlp2.h): the dilqr_mlp2 descriptor plus (n, m), H1, H2 and the
    tensors.  Built by NNDynamics.device_model(like, deep=True); stands wherever
    an MlpModel does (isinstance(., MlpModel) means one hidden layer: this is
    not a subclass of it).  Its weight gradient has its own call
    (mlp2_linearize_vjp, csrc/tu_mlp2_vjp.hip; mlp_linearize_vjp stays the
    one-hidden-layer one) and exists when vjp_ok: a first width of at most
    N.MLP2_VJP_MAX_HIDDEN1.  The DiLQR implicit backward
    (mlp_implicit_backward, csrc/tu_mlp2_implicit.hip) takes it when
    implicit_ok: a first width of at most N.MLP2_IMPLICIT_MAX_HIDDEN1."""
    entry, Desc = "dilqr_mlp2_", N.Mlp2
    width_names, layout = "(H1, H2)", "W1 [H1,n+m], b1 [H1], W2 [H2,H1], b2 [H2], W3 [n,H2], b3 [n]"

    def __init__(self, n, m, activation, passthrough, W1, b1, W2, b2, W3, b3):
        super().__init__(n, m, activation, passthrough, W1, b1, W2, b2, W3, b3)
        self.H1, self.H2 = self.widths
        self.vjp_ok = self.H1 <= N.MLP2_VJP_MAX_HIDDEN1  # inside the envelope of dilqr_mlp2_linearize_vjp_f32
        self.implicit_ok = self.H1 <= N.MLP2_IMPLICIT_MAX_HIDDEN1  # ... of dilqr_mlp2_implicit_backward_f32


MLP_MODELS = (MlpModel, Mlp2Model)


class Dynamics:
    """What the kernels take for one dynamics, resolved once per solve: the
    model id, (n, m), and theta (an env_dx model), F / f (LinDx) or the
    MlpModel / Mlp2Model (model_id MODEL_MLP, or the model in its place, with
    the descriptor as theta or ignored).  The three launches write into buffers
    of the caller, who has validated their shapes; T and B come from the
    buffers."""

    def __init__(self, model_id, n, m, theta=None, F=None, f=None, slew=False):
        """slew: the network under the slew-rate augmentation (slew_dynamics):
        n is the augmented state's, the network's n + m."""
        self.mlp = None
        if isinstance(model_id, MLP_MODELS):
            model_id, theta = N.MODEL_MLP, model_id
        if model_id == N.MODEL_MLP:
            if not isinstance(theta, MLP_MODELS):
                raise TypeError("dilqr: MODEL_MLP needs an MlpModel or Mlp2Model (NNDynamics.device_model) as theta")
            if (theta.n + (theta.m if slew else 0), theta.m) != (n, m):   # the kernels index the weights by n and m
                raise ValueError(f"dilqr: MLP model is (n, m) = {(theta.n, theta.m)}; got (n, m) = {(n, m)}")
            self.mlp, theta, F, f = theta, None, None, None
        self.slew = bool(slew) and self.mlp is not None
        self.model_id, self.n, self.m = model_id, n, m
        self.theta, self.F, self.f = theta, _f32(F), _f32(f)
        # the family of entry points the three launches call
        self._entry = "dilqr_" if self.mlp is None else self.mlp.entry + ("slew_" if self.slew else "")
        # these line searches take the previous one's cost of the accepted
        # candidate as the old cost (as the fused MPC kernel does); the others
        # recompute it
        self.carries_cost = model_id in (N.MODEL_PENDULUM, N.MODEL_CARTPOLE, N.MODEL_MLP)

    @classmethod
    def of(cls, model_id, theta, n, m, F=None, f=None):
        """The handle for the public functions' (model_id, theta, F, f), (n, m)
        being their buffers'; a handle in place of model_id is returned as it is
        once its (n, m) are seen to be the same."""
        if not isinstance(model_id, cls):
            return cls(model_id, n, m, theta, F, f)
        if (model_id.n, model_id.m) != (n, m):
            raise ValueError(f"dilqr: dynamics is (n, m) = {(model_id.n, model_id.m)}; the operands have {(n, m)}")
        return model_id

    def _head(self, T, B):
        if self.mlp is not None:
            return self.mlp.n, self.mlp.m, T, B, self.mlp.desc     # the network's own (n, m), under slew too
        return self.model_id, self.n, self.m, T, B, N.ptr(self.theta), N.ptr(self.F), N.ptr(self.f)

    def check(self, x, u):
        """x [..., n], u [..., m] of a network's handle on the weights' device
        (the kernels index rows by n and m): the model's own check, under the
        slew-rate augmentation at the augmented width."""
        if not self.slew:
            return self.mlp.check(x, u)
        if x.shape[-1] != self.n or u.shape[-1] != self.m or x.shape[:-1] != u.shape[:-1]:
            raise ValueError(f"dilqr: MLP model under the slew-rate augmentation is (n, m) = {(self.n, self.m)}; "
                             f"got x {tuple(x.shape)}, u {tuple(u.shape)}")
        if x.device != self.mlp.device or u.device != self.mlp.device:
            raise RuntimeError("dilqr: MLP weights and inputs are on different devices")

    def rollout(self, x_init, u, x_out):
        """util.get_traj (util.py:104-127): x_out [T,B,n] from x_init and u [T,B,m]."""
        T, B = u.shape[:2]
        N.call(self._entry + "rollout_f32", *self._head(T, B),
               N.ptr(x_init), N.ptr(u), N.ptr(x_out), N.stream(u.device))

    def linearize(self, x, u):
        """F [T-1,B,n,n+m], f [T-1,B,n] at (x, u); a LinDx returns its own."""
        if self.model_id == N.MODEL_LINDX:
            return self.F, self.f
        T, B = x.shape[:2]
        F = torch.empty(max(T - 1, 0), B, self.n, self.n + self.m, device=x.device)
        f = torch.empty(max(T - 1, 0), B, self.n, device=x.device)
        if self.mlp is None:
            N.call("dilqr_linearize_f32", self.model_id, T, B, N.ptr(self.theta), N.ptr(x), N.ptr(u), N.ptr(F),
                   N.ptr(f), N.stream(x.device))
        elif T > 1 and B > 0:                       # the MLP entry point is not handed empty outputs
            N.call(self._entry + "linearize_f32", *self._head(T, B), N.ptr(x), N.ptr(u), N.ptr(F), N.ptr(f),
                   N.stream(x.device))
        return F, f

    def linearize_vjp(self, x, u, gF, gf, *grads, max_waves=0):
        """The gradient of linearize's F, f into the network's weights (the MLP
        only; a two-hidden-layer model must be vjp_ok) for incoming gF, gf
        (None = zeros), written into grads, one tensor per weight in the order
        and shapes of the model's tensors (dW1, db1, dW2, db2[, dW3, db3]); the
        workspace is allocated here."""
        T, B = x.shape[:2]
        entry = self.mlp.entry + "linearize_vjp_"
        nbytes = getattr(N.lib(), entry + "ws_bytes")(self.n, self.m, T, B, *self.mlp.widths, int(max_waves))
        ws = torch.empty(max(nbytes // 4, 1), device=x.device)
        N.call(entry + "f32", self.n, self.m, T, B, self.mlp.desc, N.ptr(x), N.ptr(u), N.ptr(gF), N.ptr(gf),
               *(N.ptr(g) for g in grads), int(max_waves), N.ptr(ws), nbytes, N.stream(x.device))

    def line_search(self, x_init, C, c, x, u, K, k, bounds, zI, decay, max_ls, x_out, u_out, cost, du_sq, alpha,
                    old_cost=None):
        """lqr_forward (lqr_step_explicit.py:166-263) from (x, u) with gains K, k
        into x_out, u_out, cost [B], du_sq [T,m,B] (first pass), alpha [B]
        (final pass); old_cost [B]: the cost of (x, u) when the caller has it."""
        T, B = x.shape[:2]
        N.call(self._entry + "lqr_forward_f32", *self._head(T, B),
               N.ptr(x_init), N.ptr(C), N.ptr(c), N.ptr(x), N.ptr(u), N.ptr(K), N.ptr(k), bounds, N.ptr(zI),
               float(decay), int(max_ls), N.ptr(x_out), N.ptr(u_out), N.ptr(cost), N.ptr(du_sq), N.ptr(alpha),
               N.ptr(old_cost), N.stream(x.device))

    def fused_iterate(self, x_init, C, c, x, u, bounds, decay, max_ls, ws, x_out, u_out, cost, du_sq, alpha,
                      old_cost=None, ctrl=None):
        """linearize + lqr_backward + line_search in one launch (a one-hidden-
        layer MlpModel only: dilqr_mlp_ilqr_iterate_f32), the same bits in
        x_out, u_out, cost, du_sq, alpha.  ws: T * B * ilqr_ws_floats(n, m)
        floats; ctrl: the loop's control word (a no-op once it says stopped)."""
        T, B = x.shape[:2]
        N.call("dilqr_mlp_ilqr_iterate_f32", self.n, self.m, T, B, self.mlp.desc, N.ptr(x_init), N.ptr(C), N.ptr(c),
               N.ptr(x), N.ptr(u), bounds, float(decay), int(max_ls), N.ptr(ws), N.ptr(x_out), N.ptr(u_out),
               N.ptr(cost), N.ptr(du_sq), N.ptr(alpha), N.ptr(old_cost), N.ptr(ctrl), N.stream(x.device))


def device_dynamics(dx, like, env=True, mlp=True, deep=False):
    """The Dynamics handle of a dynamics object for tensors like `like`: a LinDx
    or an env_dx model (with env; theta is left out when like is None), or a
    Module with a device model for GPU fp32 tensors (with mlp:
    NNDynamics.device_model; with deep its two-hidden-layer model too).  None
    for a Module the kernels do not model, or of a kind the caller did not ask
    for (it then runs in torch)."""
    from .definitions import LinDx
    if isinstance(dx, LinDx):
        if not env:
            return None
        n = dx.F.shape[-2]
        return Dynamics(N.MODEL_LINDX, n, dx.F.shape[-1] - n, F=dx.F,
                        f=None if dx.f is None or dx.f.nelement() == 0 else dx.f)
    mid = getattr(dx, "model_id", None)
    if mid is not None:
        if not env:
            return None
        return Dynamics(mid, dx.n_state, dx.n_ctrl, theta=None if like is None else dx._theta(like))
    make = getattr(dx, "device_model", None)
    if not mlp or make is None or not like.is_cuda or like.dtype != torch.float32:
        return None
    md = make(like, deep=True) if deep else make(like)
    return None if md is None else Dynamics(md, md.n, md.m)


def slew_dynamics(mlp):
    """The Dynamics handle of the network mlp (an MlpModel or an Mlp2Model)
    under the slew-rate augmentation (mpc_explicit.py:383-466): the reference's
    CtrlPassthroughDynamics (dynamics.py:133-156) on device, state
    [u_{t-1}; x_t] of n = mlp.n + mlp.m entries, m = mlp.m; .mlp is the network.
    Its rollout, linearisation and line search are the dilqr_mlp_slew_* /
    dilqr_mlp2_slew_* entry points (csrc/dilqr_ctrl_through.h); it stands
    wherever a handle does (lqr_forward, mpc_solve_unfused: the four launches
    per iteration).  None when the augmented (n, m) is not a shape the kernels
    are compiled for."""
    if not isinstance(mlp, MLP_MODELS):
        raise TypeError("dilqr: slew_dynamics takes an MlpModel or an Mlp2Model (NNDynamics.device_model)")
    if (mlp.n + mlp.m, mlp.m) not in N.LANE_SHAPES:
        return None
    return Dynamics(mlp, mlp.n + mlp.m, mlp.m, slew=True)


def slew_cost_block(T, B, n, m, slew_rate_penalty, device, dtype):
    """The slew-rate penalty's own cost matrix [T,B,n+2m,n+2m] on
    [u_{t-1}; x_t; u_t] (mpc_explicit.py:383-466): gamma [[I, -I], [-I, I]] on
    the two controls, zero elsewhere."""
    d = n + 2 * m
    sC = torch.zeros(T, B, d, d, device=device, dtype=dtype)
    half_gamI = slew_rate_penalty * torch.eye(m, device=device, dtype=dtype).expand(T, B, m, m)
    sC[:, :, :m, :m] = half_gamI
    sC[:, :, -m:, :m] = -half_gamI
    sC[:, :, :m, -m:] = -half_gamI
    sC[:, :, -m:, -m:] = half_gamI
    return sC


def slew_prev_ctrl(prev_ctrl, B, m, device, dtype):
    """MPC's prev_ctrl (None = zeros, [m], [B,m] or [1,B,m]) as [1,B,m] or a
    view that expands to it (mpc_explicit.py:383-466)."""
    if prev_ctrl is None:
        return torch.zeros(1, B, m, device=device, dtype=dtype)
    prev_u = prev_ctrl.detach()
    if prev_u.ndimension() == 1:
        prev_u = prev_u.unsqueeze(0)
    if prev_u.ndimension() == 2:
        prev_u = prev_u.unsqueeze(0)
    return prev_u


def slew_problem(x_init, C, c, slew_rate_penalty, prev_ctrl, m):
    """The plain MPC problem the slew-rate augmentation solves
    (mpc_explicit.py:383-466): (x~_init [B,n+m] = [prev_ctrl; x_init],
    C~ [T,B,n+2m,n+2m] = C padded on the left and top + slew_cost_block,
    c~ [T,B,n+2m] = [0; c]) for x_init [B,n], C [T,B,n+m,n+m], c [T,B,n+m].
    Plain torch ops (they carry C's, c's and x_init's gradient);
    generic.slew_augment builds its own from these."""
    T, B = C.shape[:2]
    n = x_init.shape[1]
    dev, dt = C.device, C.dtype
    _C = slew_cost_block(T, B, n, m, slew_rate_penalty, dev, dt) + torch.nn.functional.pad(C, (m, 0, m, 0))
    _c = torch.cat((torch.zeros(T, B, m, device=dev, dtype=dt), c), 2)
    prev_u = slew_prev_ctrl(prev_ctrl, B, m, dev, dt)
    _x_init = torch.cat((prev_u[0].expand(B, m), x_init), 1)
    return _x_init, _C, _c


def generic_model_id(dx):
    """The model id of a LinDx or an env_dx model, or None for a dynamics Module
    that is neither (the caller then runs it in torch, or on its device model)."""
    dyn = device_dynamics(dx, None, mlp=False)
    return None if dyn is None else dyn.model_id


def model_id_of(dx):
    mid = generic_model_id(dx)
    if mid is None:
        raise NotImplementedError(
            "dilqr: dynamics must be a dilqr.env_dx model or a LinDx "
            "(generic autograd/finite-difference dynamics are not on the HIP path)")
    return mid


def theta_of(dx, like):
    return dx._theta(like)


def _al16(t):
    """t, or a copy when t is a view that does not start on a 16-byte boundary
    (a row block of a larger tensor: the C-ABI takes aligned pointers only)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def mlp_dynamics(mlp, x, u):
    """NNDynamics.forward (dynamics.py:66-90) for rows x [N,n], u [N,m]; mlp an
    MlpModel or an Mlp2Model, here and in mlp_linear_dyn, mlp_rollout and
    mlp_linearize."""
    x, u = _al16(_f32(x)), _al16(_f32(u))
    mlp.check(x, u)
    rows = x.shape[0]
    out = torch.empty(rows, mlp.n, device=x.device)
    N.call(mlp.entry + "dynamics_f32", mlp.n, mlp.m, rows, mlp.desc, N.ptr(x), N.ptr(u), N.ptr(out),
           N.stream(x.device))
    return out


def mlp_linear_dyn(mlp, x, u):
    """NNDynamics.grad_input (dynamics.py:92-130) as D = [R S], [N,n,n+m]."""
    x, u = _al16(_f32(x)), _al16(_f32(u))
    mlp.check(x, u)
    rows = x.shape[0]
    D = torch.empty(rows, mlp.n, mlp.n + mlp.m, device=x.device)
    N.call(mlp.entry + "linear_dyn_f32", mlp.n, mlp.m, rows, mlp.desc, N.ptr(x), N.ptr(u), N.ptr(D),
           N.stream(x.device))
    return D


def mlp_rollout(mlp, x_init, u):
    """util.get_traj (util.py:104-127) with the network: x [T,B,n]."""
    T, B, _ = u.shape
    x_init, u = _al16(_f32(x_init)), _al16(_f32(u))
    mlp.check(x_init, u[0])
    x = torch.empty(T, B, mlp.n, device=u.device)
    Dynamics(mlp, mlp.n, mlp.m).rollout(x_init, u, x)
    return x


def mlp_linearize(mlp, x, u):
    """MPC.linearize_dynamics ANALYTIC with grad_input (mpc.py:494-519):
    F [T-1,B,n,n+m], f [T-1,B,n] (empty, and nothing launched, at T = 1)."""
    x, u = _al16(_f32(x)), _al16(_f32(u))
    mlp.check(x, u)
    return Dynamics(mlp, mlp.n, mlp.m).linearize(x, u)


def _linearize_vjp(name, mlp, x, u, gF, gf, max_waves):
    """mlp_linearize_vjp and mlp2_linearize_vjp (name: the caller's, for the
    messages) once the kind of model is settled: the argument checks, one
    gradient per tensor of the model, the launches."""
    x, u = _al16(_f32(x)), _al16(_f32(u))
    if x.ndimension() != 3 or u.ndimension() != 3:
        raise ValueError(f"dilqr: {name} takes x [T,B,n], u [T,B,m]; got {tuple(x.shape)}, {tuple(u.shape)}")
    mlp.check(x, u)
    if max_waves < 0:
        raise ValueError("dilqr: max_waves must be >= 0")
    T, B = x.shape[:2]
    n, d = mlp.n, mlp.n + mlp.m
    gF, gf = (None if g is None else _al16(_f32(g)) for g in (gF, gf))
    for g, shape, gname in ((gF, (max(T - 1, 0), B, n, d), "gF"), (gf, (max(T - 1, 0), B, n), "gf")):
        if g is None:
            continue
        if tuple(g.shape) != shape:
            raise ValueError(f"dilqr: {gname} must be {shape}; got {tuple(g.shape)}")
        if g.device != mlp.device:
            raise RuntimeError("dilqr: MLP weights and inputs are on different devices")
    rows = max(T - 1, 0) * B
    new = torch.zeros if rows == 0 else torch.empty
    out = tuple(new(*t.shape, device=x.device) for t in mlp.tensors)
    if rows:
        Dynamics(mlp, mlp.n, mlp.m).linearize_vjp(x, u, gF, gf, *out, max_waves=max_waves)
    return out


def mlp_linearize_vjp(mlp, x, u, gF, gf, max_waves=0):
    """The backward of mlp_linearize into the weights: (dW1 [H,n+m], db1 [H],
    dW2 [n,H], db2 [n]) for gradients gF [T-1,B,n,n+m] on F and gf [T-1,B,n]
    on f (None = zeros) at x [T,B,n], u [T,B,m]; two launches, no atomics, the
    same bits on every run (csrc/tu_mlp_vjp.hip).  max_waves caps the groups of
    waves the rows are dealt to (0: the library's default); zeros, and nothing
    launched, at T = 1 or B = 0."""
    if not isinstance(mlp, MlpModel):
        raise TypeError("dilqr: mlp_linearize_vjp is built for the one-hidden-layer MlpModel only")
    return _linearize_vjp("mlp_linearize_vjp", mlp, x, u, gF, gf, max_waves)


def mlp2_linearize_vjp(mlp2, x, u, gF, gf, max_waves=0):
    """mlp_linearize_vjp for the two-hidden-layer Mlp2Model: (dW1 [H1,n+m],
    db1 [H1], dW2 [H2,H1], db2 [H2], dW3 [n,H2], db3 [n]) for gradients
    gF [T-1,B,n,n+m] on F and gf [T-1,B,n] on f (None = zeros) at x [T,B,n],
    u [T,B,m]; three launches, no atomics, the same bits on every run
    (csrc/tu_mlp2_vjp.hip).  max_waves caps the groups of waves the rows are
    dealt to (0: the library's defaults); zeros, and nothing launched, at T = 1
    or B = 0.  The model must be vjp_ok (H1 <= N.MLP2_VJP_MAX_HIDDEN1)."""
    if not isinstance(mlp2, Mlp2Model):
        raise TypeError("dilqr: mlp2_linearize_vjp is built for the two-hidden-layer Mlp2Model only")
    if not mlp2.vjp_ok:
        raise ValueError(f"dilqr: mlp2_linearize_vjp takes H1 <= {N.MLP2_VJP_MAX_HIDDEN1}; got {mlp2.H1}")
    return _linearize_vjp("mlp2_linearize_vjp", mlp2, x, u, gF, gf, max_waves)


class _LinearizeDiff(torch.autograd.Function):
    """mlp_linearize with the gradient into the model's parameters (W, b per
    layer: the storage the model points at): the linearisation kernel forward,
    the weight gradient backward — vjp names it, mlp_linearize_vjp or
    mlp2_linearize_vjp, and it is looked up in this module when the backward
    runs.  x and u get no gradient."""

    @staticmethod
    def forward(ctx, mlp, vjp, x, u, *params):
        ctx.mlp, ctx.vjp = mlp, vjp
        ctx.set_materialize_grads(False)
        # saved so that an in-place update of a parameter between forward and
        # backward is refused by autograd (the kernels read the live storage)
        ctx.save_for_backward(x, u, *params)
        F, f = mlp_linearize(mlp, x, u)
        return F, f

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gF, gf):
        x, u = ctx.saved_tensors[:2]
        grads = globals()[ctx.vjp](ctx.mlp, x, u, gF, gf)
        return (None,) * 4 + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:]))


def _linearize_diff(vjp, mlp, params, count, refusal, x, u):
    params = tuple(params)
    if len(params) != count or any(p.data_ptr() != t.data_ptr() or p.shape != t.shape
                                   for p, t in zip(params, mlp.tensors)):
        raise ValueError(refusal)
    return _LinearizeDiff.apply(mlp, vjp, x.detach(), u.detach(), *params)


def mlp_linearize_diff(mlp, params, x, u):
    """mlp_linearize(mlp, x, u) whose F, f carry the gradient into params =
    (W1, b1, W2, b2), the Parameters mlp was made from (NNDynamics.fcs); the
    same bits as mlp_linearize.  Not differentiable twice, and not with respect
    to x and u."""
    return _linearize_diff("mlp_linearize_vjp", mlp, params, 4, "dilqr: mlp_linearize_diff takes the four "
                           "parameters (W1, b1, W2, b2) the MlpModel reads", x, u)


def mlp2_linearize_diff(mlp2, params, x, u):
    """mlp_linearize(mlp2, x, u) whose F, f carry the gradient into params =
    (W1, b1, W2, b2, W3, b3), the Parameters the Mlp2Model was made from
    (NNDynamics.fcs); the same bits as mlp_linearize.  Not differentiable
    twice, and not with respect to x and u."""
    if not isinstance(mlp2, Mlp2Model) or not mlp2.vjp_ok:
        raise ValueError("dilqr: mlp2_linearize_diff takes an Mlp2Model inside the weight gradient's envelope (vjp_ok)")
    return _linearize_diff("mlp2_linearize_vjp", mlp2, params, 6, "dilqr: mlp2_linearize_diff takes the six "
                           "parameters (W1, b1, W2, b2, W3, b3) the Mlp2Model reads", x, u)


def mlp_implicit_backward(mlp, dl_dx, dl_du, C, c, x, u, u_lower, u_upper, want_dF=True):
    """The DiLQR implicit backward at a solution (x [T,B,n], u [T,B,m]) of a
    solve on an MlpModel or an Mlp2Model with cost C [T,B,d,d], c [T,B,d] and
    box u_lower / u_upper (None, floats or [T,B,m] tensors), for the loss
    gradients dl_dx, dl_du: the derivative of the iLQR fixed point, curvature of
    the network included (csrc/tu_mlp_implicit.hip, csrc/tu_mlp2_implicit.hip;
    one launch).  Returns (dx_init [B,n], dC, dc, dF [T-1,B,n,d],
    df [T-1,B,n]); the gradient into the weights is
    mlp_linearize_vjp(mlp, x, u, dF, df), for a two-hidden-layer model
    mlp2_linearize_vjp(mlp2, x, u, dF, df).  Without want_dF, dF and df are
    None: not computed, not allocated.  An Mlp2Model must be implicit_ok
    (H1 <= N.MLP2_IMPLICIT_MAX_HIDDEN1)."""
    if not isinstance(mlp, MLP_MODELS):
        raise TypeError("dilqr: mlp_implicit_backward takes an MlpModel or an Mlp2Model (NNDynamics.device_model)")
    if not getattr(mlp, "implicit_ok", True):
        raise ValueError(f"dilqr: mlp_implicit_backward takes H1 <= {N.MLP2_IMPLICIT_MAX_HIDDEN1} for a "
                         f"two-hidden-layer model; got {mlp.H1}")
    dl_dx, dl_du, C, c, x, u = (_al16(_f32(t)) for t in (dl_dx, dl_du, C, c, x, u))
    if x.ndimension() != 3 or u.ndimension() != 3:
        raise ValueError(f"dilqr: mlp_implicit_backward takes x [T,B,n], u [T,B,m]; got {tuple(x.shape)}, "
                         f"{tuple(u.shape)}")
    T, B = x.shape[:2]
    n, m = mlp.n, mlp.m
    d = n + m
    if T < 1 or x.shape[2] != n or tuple(u.shape) != (T, B, m):
        raise ValueError(f"dilqr: MLP model is (n, m) = {(n, m)}; got x {tuple(x.shape)}, u {tuple(u.shape)}")
    for t, shape, name in ((dl_dx, (T, B, n), "dl_dx"), (dl_du, (T, B, m), "dl_du"), (C, (T, B, d, d), "C"),
                           (c, (T, B, d), "c")):
        if tuple(t.shape) != shape:
            raise ValueError(f"dilqr: {name} must be {shape}; got {tuple(t.shape)}")
    if (u_lower is None) != (u_upper is None):
        raise ValueError("dilqr: u_lower and u_upper go together")
    for b, name in ((u_lower, "u_lower"), (u_upper, "u_upper")):
        if isinstance(b, torch.Tensor) and tuple(b.shape) != (T, B, m):
            raise ValueError(f"dilqr: {name} must be a float or {(T, B, m)}; got {tuple(b.shape)}")
    for t in (dl_dx, dl_du, C, c, x, u, u_lower, u_upper):
        if isinstance(t, torch.Tensor) and t.device != mlp.device:
            raise RuntimeError("dilqr: MLP weights and inputs are on different devices")
    dev = x.device
    rec = N.lib().dilqr_mlp_implicit_ws_floats(n, m)
    if rec < 0:
        raise ValueError(f"dilqr: no implicit backward kernel for (n, m) = {(n, m)}")
    bounds, keep = N.make_bounds(u_lower, u_upper)
    ws = torch.empty(max(T * B * rec, 4), device=dev)
    dx0 = torch.empty(B, n, device=dev)
    dC = torch.empty(T, B, d, d, device=dev)
    dc = torch.empty(T, B, d, device=dev)
    # at T = 1 there is no F: the kernel is handed no empty outputs
    want = bool(want_dF) and T > 1
    dF = torch.empty(T - 1, B, n, d, device=dev) if want else None
    df = torch.empty(T - 1, B, n, device=dev) if want else None
    if B > 0:                                       # an empty batch: empty outputs, nothing launched
        N.call(mlp.entry + "implicit_backward_f32", n, m, T, B, mlp.desc, N.ptr(C), N.ptr(c), N.ptr(x), N.ptr(u),
               N.ptr(dl_dx), N.ptr(dl_du), bounds, N.ptr(ws), N.ptr(dx0), N.ptr(dC), N.ptr(dc), N.ptr(dF),
               N.ptr(df), N.stream(dev))
    del keep
    if want_dF and not want:
        dF, df = torch.zeros(0, B, n, d, device=dev), torch.zeros(0, B, n, device=dev)
    return dx0, dC, dc, dF, df


class _MlpImplicitStep(torch.autograd.Function):
    """The closing no-op LQR step of a solve on the MlpModel (generic.final_step,
    classic=False): forward returns the solution, backward is
    mlp_implicit_backward.  F and f are graph edges only — the kernel
    linearises at (x, u) itself; their gradients dF, df go on to the
    linearisation's backward (mlp_linearize_vjp, or the torch graph through
    grad_input)."""

    @staticmethod
    def forward(ctx, mlp, lo, hi, x, u, x_init, C, c, F, f):
        ctx.mlp, ctx.lo, ctx.hi = mlp, lo, hi
        # the weights are saved so that an in-place update between forward and
        # backward is refused by autograd (the kernel reads the live storage)
        ctx.save_for_backward(C, c, x, u, *mlp.tensors)
        return x.clone(), u.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dl_dx, dl_du):
        C, c, x, u = ctx.saved_tensors[:4]
        need = ctx.needs_input_grad
        dx0, dC, dc, dF, df = mlp_implicit_backward(ctx.mlp, dl_dx, dl_du, C, c, x, u, ctx.lo, ctx.hi,
                                                    want_dF=need[8] or need[9])
        grads = (dx0, dC, dc, dF, df)
        return (None,) * 5 + tuple(g if nd else None for g, nd in zip(grads, need[5:]))


def mlp_implicit_step(mlp, x_init, C, c, F, f, x, u, u_lower=None, u_upper=None):
    """(x, u) carrying the DiLQR implicit gradient into x_init, C, c and,
    through F and f (the differentiable linearisation at (x, u)), into the
    network's weights."""
    lo = u_lower if (u_lower is None or isinstance(u_lower, (int, float))) else u_lower.detach()
    hi = u_upper if (u_upper is None or isinstance(u_upper, (int, float))) else u_upper.detach()
    return _MlpImplicitStep.apply(mlp, lo, hi, x.detach(), u.detach(), x_init, C, c, F, f)


def rollout(model_id, theta, x_init, u, F=None, f=None):
    """util.get_traj (util.py:104-127)."""
    T, B, m = u.shape
    n = x_init.shape[1]
    x_init, u = _f32(x_init), _f32(u)
    x = torch.empty(T, B, n, device=u.device)
    Dynamics.of(model_id, theta, n, m, F, f).rollout(x_init, u, x)
    return x


def linearize(model_id, theta, x, u):
    """MPC.linearize_dynamics ANALYTIC (mpc_explicit.py:516-546)."""
    return Dynamics.of(model_id, theta, x.shape[2], u.shape[2]).linearize(_f32(x), _f32(u))


def zero_mask(u_zero_I, T, B, m, device):
    """u_zero_I as the kernels read it: uint8 [T,B,m] on `device` (the kernels
    index it (t*B + b)*m + a for every t and b, so any other shape is refused
    here rather than read out of bounds on the device)."""
    if u_zero_I is None:
        return None
    if tuple(u_zero_I.shape) != (T, B, m):
        raise ValueError(f"u_zero_I: expected [T, B, m] = {(T, B, m)}, got {tuple(u_zero_I.shape)}")
    return u_zero_I.to(device=device, dtype=torch.uint8).contiguous()


def lqr_backward(C, c, F, n, m, x=None, u=None, u_lower=None, u_upper=None, u_zero_I=None,
                 m_solver=N.SOLVE_INV, want_nqp=False, qp_total=False):
    """lqr_backward (lqr_step_explicit.py:54-162) with the fused delta-space c_back.
    Returns K [T,B,m,n], k [T,B,m] (natural time order), and n_qp [B] (the
    per-problem sums of 1 + pnqp iterations) with want_nqp, or with qp_total
    the reference's n_total_qp_iter (lqr_step_explicit.py:148-150: its batched
    pnqp runs each step until the slowest problem converges, so the count is
    sum_t (1 + max over problems of that step's iterations); 0 unbounded)."""
    T, B = C.shape[:2]
    C, c, F, x, u = _f32(C), _f32(c), _f32(F), _f32(x), _f32(u)
    bounds, keep = N.make_bounds(u_lower, u_upper)
    zI = zero_mask(u_zero_I, T, B, m, C.device)
    K = torch.empty(T, B, m, n, device=C.device)
    k = torch.empty(T, B, m, device=C.device)
    nqp = torch.zeros(B, dtype=torch.int32, device=C.device) if want_nqp else None
    step = torch.zeros(T, dtype=torch.int32, device=C.device) if qp_total else None
    N.call("dilqr_lqr_backward_f32", n, m, T, B, N.ptr(C), N.ptr(c), N.ptr(x), N.ptr(u), N.ptr(F), bounds,
           N.ptr(zI), m_solver, N.ptr(K), N.ptr(k), N.ptr(nqp), N.ptr(step), N.stream(C.device))
    del keep
    if qp_total:
        return K, k, (int(step.sum().item()) + T if bounds.mode != N.BOUNDS_NONE else 0)
    return K, k, nqp


def c_back(C, c, x, u):
    """Delta-space linear term C_t tau_t + c_t (lqr_step_explicit.py:630-636),
    for the callers that hand the sweep relative bounds (delta_u)."""
    tau = torch.cat((x, u), -1)
    return (C @ tau.unsqueeze(-1)).squeeze(-1) + c


def _full(v, like):
    return v if isinstance(v, torch.Tensor) else torch.full_like(like, float(v))


def delta_u_sweep_bounds(u_lower, u_upper, u, delta_u):
    """The sweep's box in delta space with the delta_u trust region,
    lqr_step_explicit.py:132-135: lb = lower - u_t, ub = upper - u_t, then
    lb[lb < -delta_u] = -delta_u, ub[ub > delta_u] = delta_u (exact values)."""
    lb = _full(u_lower, u) - u
    ub = _full(u_upper, u) - u
    lb = torch.where(lb < -delta_u, torch.full_like(lb, -delta_u), lb)
    ub = torch.where(ub > delta_u, torch.full_like(ub, delta_u), ub)
    return lb.contiguous(), ub.contiguous()


def delta_u_rollout_bounds(u_lower, u_upper, u, delta_u):
    """The rollout's clamp with the delta_u trust region, lqr_step_explicit.py:
    205-213: lb = u_t - delta_u raised to lower, ub = u_t + delta_u cut to upper."""
    lb = u - delta_u
    ub = u + delta_u
    lo, hi = _full(u_lower, u), _full(u_upper, u)
    lb = torch.where(lb < lo, lo, lb)
    ub = torch.where(ub > hi, hi, ub)
    return lb.contiguous(), ub.contiguous()


def delta_sweep(C, c, F, n, m, x, u, u_lower, u_upper, u_zero_I=None, delta_u=None, qp_total=False):
    """The LQR step's Riccati sweep in delta space around (x, u): lqr_backward
    with c_back fused into the kernel; with delta_u the box is relative to u
    and clipped to +-delta_u (lqr_step_explicit.py:132-135) and c_back is formed
    here; the u_zero_I mask applies only without bounds (the reference's pnqp
    branch ignores it)."""
    if delta_u is not None:
        rlo, rhi = delta_u_sweep_bounds(u_lower, u_upper, u, delta_u)
        return lqr_backward(C, c_back(C.detach(), c.detach(), x, u), F, n, m, u_lower=rlo, u_upper=rhi,
                            qp_total=qp_total)
    return lqr_backward(C, c, F, n, m, x=x, u=u, u_lower=u_lower, u_upper=u_upper,
                        u_zero_I=u_zero_I if u_lower is None else None, qp_total=qp_total)


def lqr_forward(model_id, theta, x_init, C, c, x, u, K, k, F=None, f=None, u_lower=None, u_upper=None,
                u_zero_I=None, linesearch_decay=0.2, max_linesearch_iter=10):
    """lqr_forward (lqr_step_explicit.py:166-263): returns new_x, new_u, costs [B],
    du_sq [T,m,B] (first pass), alphas [B] (final pass).  An MlpModel or
    Mlp2Model in place of model_id (theta then ignored), or MODEL_MLP with it as
    theta, rolls out the network (its own entry point); a Dynamics handle in
    place of model_id is taken as it is."""
    T, B, n = x.shape
    m = u.shape[2]
    x_init, C, c, x, u, K, k = map(_f32, (x_init, C, c, x, u, K, k))
    bounds, keep = N.make_bounds(u_lower, u_upper)
    zI = zero_mask(u_zero_I, T, B, m, x.device)
    dev = x.device
    nx, nu = torch.empty_like(x), torch.empty_like(u)
    cost, alpha = torch.empty(B, device=dev), torch.empty(B, device=dev)
    du_sq = torch.empty(T, m, B, device=dev)
    dyn = Dynamics.of(model_id, theta, n, m, F, f)
    if dyn.mlp is not None:
        dyn.check(x, u)
        d = n + m
        if (tuple(x_init.shape), tuple(C.shape), tuple(c.shape), tuple(K.shape), tuple(k.shape)) != (
                (B, n), (T, B, d, d), (T, B, d), (T, B, m, n), (T, B, m)):
            raise ValueError("dilqr: lqr_forward operands must be x_init [B,n], C [T,B,d,d], c [T,B,d], "
                             "K [T,B,m,n], k [T,B,m]")
    dyn.line_search(x_init, C, c, x, u, K, k, bounds, zI, linesearch_decay, max_linesearch_iter, nx, nu, cost,
                    du_sq, alpha)
    del keep
    return nx, nu, cost, du_sq, alpha


def pnqp(H, q, lower, upper, x_init=None):
    """pnqp.py:5-82 per problem -> (x [B,m], H_ [B,m,m], If [B,m], n_iter [B]).
    lower/upper: floats or [B,m] tensors.  The reference's batched call couples
    the Armijo loop across the batch; this is the reference at batch size 1."""
    B, m = q.shape
    H, q, x_init = _f32(H), _f32(q), _f32(x_init)
    bounds, keep = N.make_bounds(lower, upper)
    x = torch.empty(B, m, device=q.device)
    If = torch.empty(B, m, device=q.device)
    Hf = torch.empty(B, m, m, device=q.device)
    it = torch.empty(B, dtype=torch.int32, device=q.device)
    N.call("dilqr_pnqp_f32", m, B, N.ptr(H), N.ptr(q), bounds, N.ptr(x_init), N.ptr(x), N.ptr(If), N.ptr(Hf),
           N.ptr(it), N.stream(q.device))
    del keep
    return x, Hf, If, it


def quirk_norm(du_sq):
    """lqr_step_explicit.py:245-247 norm over the re-viewed [T,m,B] buffer."""
    T, m, B = du_sq.shape
    out = torch.empty(B, device=du_sq.device)
    N.call("dilqr_quirk_norm_f32", T, m, B, N.ptr(du_sq), N.ptr(out), N.stream(du_sq.device))
    return out


def _lim(not_improved_lim):
    """not_improved_lim as the C-ABI's int (callers pass 10 ** 9 and more for "never")."""
    return int(min(not_improved_lim, 2 ** 31 - 1))


def expand_u_init(u_init, T, B, m, device, dtype=torch.float32):
    """u_init on `device`, a [T,m] plan repeated over the batch as an expanded
    view [T,B,m] (m = -1 keeps its last size).  What else the callers accept
    differs and stays theirs: MPCSolve makes it contiguous and refuses any other
    shape than [T,B,m] (ValueError); mpc_solve_unfused lets copy_ broadcast it
    into its buffer; generic.solve keeps x_init's dtype, clones the expanded
    view and takes a [T,B,m] tensor as it is."""
    u0 = u_init.to(device=device, dtype=dtype)
    if u0.ndimension() == 2:
        u0 = u0.unsqueeze(1).expand(T, B, m)
    return u0


def grec_floats(n, m):
    return ((m * n + m + 1) + 3) // 4 * 4


def ilqr_ws_floats(n, m):
    """Per-(t,b) workspace of dilqr_ilqr_iterate_f32: gain record + the line
    search's second candidate (x, u)."""
    return grec_floats(n, m) + n + m


class MPCWorkspace:
    """Device buffers of one MPC solve (reused across iterations)."""

    def __init__(self, T, B, n, m, device, packed_cost=True, fused=False):
        """fused: ws also holds the fused iteration's second line-search candidate."""
        dev = device
        self.dims = (n, m, T, B)
        self.xa = torch.empty(T, B, n, device=dev)
        self.ua = torch.empty(T, B, m, device=dev)
        self.xb = torch.empty(T, B, n, device=dev)
        self.ub = torch.empty(T, B, m, device=dev)
        self.ws = torch.empty(T * B * (ilqr_ws_floats(n, m) if fused else grec_floats(n, m)), device=dev)
        self.cost = torch.empty(B, device=dev)
        self.alpha = torch.empty(B, device=dev)
        self.du_sq = torch.empty(T, m, B, device=dev)
        self.fdn = torch.empty(B, device=dev)
        self.best_x = torch.empty(T, B, n, device=dev)
        self.best_u = torch.empty(T, B, m, device=dev)
        self.best_cost = torch.empty(B, device=dev)
        self.best_du = torch.empty(B, device=dev)
        self.ctrl = torch.zeros(N.CTRL_INTS, dtype=torch.int32, device=dev)

    def update_best(self, first, best_cost_eps, eps, lim):
        """Best-iterate bookkeeping and the stop rule for the new iterate (xb, ub)."""
        N.call("dilqr_mpc_update_best_f32", *self.dims, int(first), float(best_cost_eps), float(eps), lim,
               *map(N.ptr, (self.xb, self.ub, self.cost, self.du_sq, self.fdn, self.best_x, self.best_u,
                            self.best_cost, self.best_du, self.ctrl)), N.stream(self.ctrl.device))

    def swap(self):
        self.xa, self.xb, self.ua, self.ub = self.xb, self.xa, self.ub, self.ua

    def stop_seen(self, i, check_every, lqr_iter):
        """After iteration i: a poll point at which the rule has fired."""
        return bool(check_every and (i + 1) % check_every == 0 and i + 1 < lqr_iter and int(self.ctrl[1].item()))


class MPCSolve:
    """Device state of one fused MPC solve (dilqr_mpc_state): three trajectory
    slots per problem (current, best, two line-search candidates), per-problem
    best bookkeeping, the loop control block."""

    def __init__(self, T, B, n, m, device, packed_cost=True, fixed_iters=None):
        """fixed_iters: a fixed-count solve of that many iterations (the stop rule
        cannot fire: eps <= 0, not_improved_lim >= iterations) — one launch per
        iteration (iterate_fixed) and finish_fixed at the end; du_sq keeps one
        [T,m,B] plane per iteration."""
        dev = device
        self.T, self.B, self.n, self.m = T, B, n, m
        self.fixed_iters = fixed_iters
        # slots: [4,T,B,n+m] records [x_t; u_t] for the thread-per-problem models
        # (Us aliases Xs, unused by the kernels), the caller's [4,T,B,n] and
        # [4,T,B,m] for rocket
        self.rec = n + m <= 8
        if self.rec:
            self.Xs = torch.zeros((4, T, B, n + m), device=dev)
            self.Us = self.Xs
        else:
            self.Xs = torch.empty((4, T, B, n), device=dev)
            self.Us = torch.zeros((4, T, B, m), device=dev)
        self.slot = torch.zeros(2, B, dtype=torch.uint8, device=dev)
        self.best_cost = torch.empty(B, device=dev)
        self.best_du = torch.empty(B, device=dev)
        self.improved = torch.zeros(B, dtype=torch.int32, device=dev)
        self.cost = torch.empty(B, device=dev)
        self.alpha = torch.empty(B, device=dev)
        self.du_sq = torch.empty((fixed_iters or 1) * T, m, B, device=dev)
        self.best_iter = torch.zeros(B, dtype=torch.int32, device=dev) if fixed_iters else None
        self.full_du_norm = torch.empty(B, device=dev)
        self.ws = torch.empty(T * B * ilqr_ws_floats(n, m), device=dev)
        self.ctrl = torch.zeros(2 * N.CTRL_INTS, dtype=torch.int32, device=dev)   # ping-pong control state
        self.last_iteration = -1
        # stop-rule sync area: 16 words + two planes of per-workgroup partials (<= ceil(B/64))
        self.counter = torch.zeros(16 + 4 * ((B + 63) // 64), dtype=torch.int32, device=dev)
        # the solve's copy of its cost: packed symmetric records for the thread-per-
        # problem fused kernels (d <= 8), one [2d] row record per problem (a
        # time-invariant diagonal cost) for the 16-lane ones
        pk = N.lib().dilqr_mpc_packed_cost_floats(n, m)
        if not packed_cost:
            self.Cpk = None
        elif n + m <= 8:
            self.Cpk = torch.empty(T * B * pk, device=dev)
        else:
            self.Cpk = torch.empty(B * 2 * (n + m), device=dev)
        self.cost_sym = torch.zeros(B, dtype=torch.uint8, device=dev) if self.Cpk is not None else None
        self.state = N.MpcState(*[t.data_ptr() if t is not None else None for t in (
            self.Xs, self.Us, self.slot, self.best_cost, self.best_du, self.improved, self.cost, self.alpha,
            self.du_sq, self.full_du_norm, self.ws, self.ctrl, self.counter, self.Cpk, self.cost_sym,
            self.best_iter)])

    def _u_init(self, u_init):
        if u_init is None:
            return None
        u0 = expand_u_init(u_init, self.T, self.B, self.m, self.Xs.device).contiguous()
        if tuple(u0.shape) != (self.T, self.B, self.m):
            raise ValueError(f"u_init: expected [T, B, m] = {(self.T, self.B, self.m)} or [T, m], got "
                             f"{tuple(u_init.shape)}")
        return u0

    def begin(self, model_id, theta, x_init, u_init=None):
        """x = get_traj(u_init or 0) into slot 0; reset slots and the control block."""
        u0 = self._u_init(u_init)
        N.call("dilqr_mpc_begin_f32", model_id, self.T, self.B, N.ptr(theta), N.ptr(x_init),
               None if u0 is None else N.ptr(u0), self.state, N.stream(x_init.device))
        self._u0 = u0                       # alive until the launch has read it

    def solve_fixed(self, model_id, theta, x_init, C, c, bounds, decay, max_ls, best_cost_eps, u_init=None):
        """A whole fixed-count solve of fixed_iters iterations in one call
        (dilqr_mpc_solve_fixed_f32: begin + every iteration in one launch for
        the single-lane models, then finish); the same bits as begin +
        iterate_fixed per iteration + finish_fixed."""
        if not self.fixed_iters:
            raise ValueError("solve_fixed: solve not built for a fixed count")
        u0 = self._u_init(u_init)
        N.call("dilqr_mpc_solve_fixed_f32", model_id, self.T, self.B, N.ptr(theta), N.ptr(x_init),
               None if u0 is None else N.ptr(u0), N.ptr(C), N.ptr(c), bounds, float(decay), int(max_ls),
               int(self.fixed_iters), float(best_cost_eps), self.state, N.stream(x_init.device))
        self._u0 = u0
        self.last_iteration = self.fixed_iters - 1

    def solve_small(self, model_id, theta, x_init, C, c, bounds, decay, max_ls, iterations, best_cost_eps, eps,
                    not_improved_lim, u_init=None):
        """A whole stop-rule solve in one launch (dilqr_mpc_solve_small_f32: B <=
        SMALL_BATCH_MAX, one workgroup, the rule applied in-kernel after each
        iteration); the same bits as begin + iterate per iteration."""
        u0 = self._u_init(u_init)
        N.call("dilqr_mpc_solve_small_f32", model_id, self.T, self.B, N.ptr(theta), N.ptr(x_init),
               None if u0 is None else N.ptr(u0), N.ptr(C), N.ptr(c), bounds, float(decay), int(max_ls),
               int(iterations), float(best_cost_eps), float(eps), _lim(not_improved_lim),
               self.state, N.stream(x_init.device))
        self._u0 = u0
        self.small = True
        self.last_iteration = iterations - 1

    def iterate(self, model_id, theta, x_init, C, c, bounds, decay, max_ls, iteration, best_cost_eps, eps,
                not_improved_lim):
        """Iteration `iteration` (0, 1, ...) of the solve started by begin()."""
        if isinstance(iteration, bool):
            raise TypeError("iteration is the 0-based iteration index")
        N.call("dilqr_mpc_iterate_f32", model_id, self.T, self.B, N.ptr(theta), N.ptr(x_init), N.ptr(C),
               N.ptr(c), bounds, float(decay), int(max_ls), int(iteration), float(best_cost_eps), float(eps),
               _lim(not_improved_lim), self.state, N.stream(x_init.device))
        self.last_iteration = int(iteration)

    def iterate_range(self, model_id, theta, x_init, C, c, bounds, decay, max_ls, first, count, best_cost_eps, eps,
                      not_improved_lim):
        """Iterations first .. first+count-1 in one library call (the same
        launches as iterate() for each)."""
        N.call("dilqr_mpc_iterate_range_f32", model_id, self.T, self.B, N.ptr(theta), N.ptr(x_init), N.ptr(C),
               N.ptr(c), bounds, float(decay), int(max_ls), int(first), int(count), float(best_cost_eps), float(eps),
               _lim(not_improved_lim), self.state, N.stream(x_init.device))
        if count > 0:
            self.last_iteration = int(first + count - 1)

    def iterate_fixed(self, model_id, theta, x_init, C, c, bounds, decay, max_ls, iteration, best_cost_eps):
        """Iteration `iteration` of a fixed-count solve (one launch, no stop rule)."""
        if not self.fixed_iters or not 0 <= iteration < self.fixed_iters:
            raise ValueError("iterate_fixed: solve not built for a fixed count, or iteration out of range")
        N.call("dilqr_mpc_iterate_fixed_f32", model_id, self.T, self.B, N.ptr(theta), N.ptr(x_init), N.ptr(C),
               N.ptr(c), bounds, float(decay), int(max_ls), int(iteration), float(best_cost_eps), self.state,
               N.stream(x_init.device))
        self.last_iteration = int(iteration)

    def finish_fixed(self, iterations):
        """best_du of a fixed-count solve after `iterations` iterations."""
        N.call("dilqr_mpc_finish_fixed_f32", self.T, self.m, self.B, int(iterations), self.state,
               N.stream(self.Xs.device))

    def poll_buffer(self, i):
        """Pinned host buffer i (a small ring) for mpc_solve's non-blocking stop
        polls; a buffer is reused only after its poll was read."""
        if not hasattr(self, "_polls"):
            self._polls = [torch.empty(N.CTRL_INTS, dtype=torch.int32, pin_memory=True)
                           for _ in range(POLL_AHEAD + 2)]
        return self._polls[i % len(self._polls)]

    def _ctrl_now(self):
        k = max(self.last_iteration, 0)
        return self.ctrl.view(2, N.CTRL_INTS)[k & 1]        # solve_small writes both words

    def gather_best(self):
        x = torch.empty(self.T, self.B, self.n, device=self.Xs.device)
        u = torch.empty(self.T, self.B, self.m, device=self.Xs.device)
        N.call("dilqr_mpc_gather_best_f32", self.n, self.m, self.T, self.B, self.state, N.ptr(x), N.ptr(u),
               N.stream(x.device))
        return x, u

    @property
    def stopped(self):
        """True once the stop rule fired (the device skips later iterations); the
        rule for the last launched iteration is applied by the next one."""
        return bool(int(self._ctrl_now()[1].item()))

    @property
    def iterations(self):
        """The iterations that ran: the device's count when the stop rule fired
        (published by the prologue after the iteration that met it), else every
        launched iteration (the rule of the last one is never applied, so the
        device word then reads one less; every solve path leaves the same word)."""
        ctrl = self._ctrl_now()
        if int(ctrl[1].item()):
            return int(ctrl[0].item())
        return self.last_iteration + 1


# runs of the stop-rule loop queued behind the oldest unread stop-flag copy
# (mpc_solve): the host waits for a poll only this far behind the device
# (DILQR_POLL_AHEAD=0: a blocking poll after every run, the round-5 loop)
POLL_AHEAD = int(os.environ.get("DILQR_POLL_AHEAD", "2"))

# dilqr_mpc_solve_small_f32: batches one workgroup holds, thread-per-problem models
SMALL_BATCH_MAX = 256
SMALL_BATCH_MODELS = (N.MODEL_PENDULUM, N.MODEL_CARTPOLE, N.MODEL_PENDULUM_COMPLEX)

# mpc_solve_unfused on a one-hidden-layer MlpModel runs the fused iteration
# (dilqr_mlp_ilqr_iterate_f32 / dilqr_mlp_mpc_solve_small_f32: the same bits as
# the four launches per iteration).  False: always the four launches (tests and
# tools/bench_nn_mpc.py run both routes on the same inputs).
MLP_FUSED = True
# the largest batch the per-iteration fused kernel is taken at (None: any):
# the measured rule of DESIGN.md §6b
MLP_FUSED_MAX_BATCH = None
# the largest batch the one-launch solve (dilqr_mlp_mpc_solve_small_f32, up to
# SMALL_BATCH_MAX problems) is taken at.  0: never.  Measured,
# it does not beat the four launches at B = 32..128 and loses at 256, one
# workgroup's waves sharing a CU, while the fused iteration per launch wins at
# every batch; so the route does not take it (tests and tools set this to
# SMALL_BATCH_MAX to run it)
MLP_SMALL_MAX_BATCH = 0


def mlp_solve_route(dyn, B, lqr_iter, u_zero_I, verbose):
    """Which launches mpc_solve_unfused runs for a dynamics (a Dynamics handle
    or a model): "small", the whole stop-rule solve in one launch (B <=
    min(SMALL_BATCH_MAX, MLP_SMALL_MAX_BATCH), a shape in N.MLP_SMALL_SHAPES); "fused", the fused iteration +
    dilqr_mpc_update_best_f32 per iteration; "unfused", the four launches per
    iteration: everything but a one-hidden-layer MlpModel, a control mask,
    verbose, MLP_FUSED off, a batch above MLP_FUSED_MAX_BATCH; and a handle
    under the slew-rate augmentation (slew_dynamics), whose fused iteration is
    not built."""
    mlp = dyn.mlp if isinstance(dyn, Dynamics) else dyn
    if getattr(dyn, "slew", False):
        return "unfused"
    if not MLP_FUSED or not isinstance(mlp, MlpModel) or u_zero_I is not None or verbose > 0:
        return "unfused"
    if B < 1 or lqr_iter < 1:
        return "unfused"
    if B <= min(SMALL_BATCH_MAX, MLP_SMALL_MAX_BATCH) and (mlp.n, mlp.m) in N.MLP_SMALL_SHAPES:
        return "small"
    if MLP_FUSED_MAX_BATCH is not None and B > MLP_FUSED_MAX_BATCH:
        return "unfused"
    return "fused"


def mpc_solve(model_id, theta, x_init, C, c, T, u_init=None, u_lower=None, u_upper=None, lqr_iter=10,
              eps=1e-7, linesearch_decay=0.2, max_linesearch_iter=10, not_improved_lim=5, best_cost_eps=1e-4,
              check_every=8, verbose=0):
    """The iLQR outer loop of mpc_explicit.MPC.forward (mpc_explicit.py:228-299)
    entirely on device (fused iterate kernel + norm/stop kernel per iteration);
    the host only polls the stop flag every `check_every` iterations.
    Returns (best_x, best_u, best_cost, best_du, solve).

    verbose > 0: the same launches one iteration per library call, each
    followed by reductions queued on the stream (mean best cost, max
    full_du_norm, mean step size: the reference's table row, mpc_explicit.py:
    285-295) into a device array; `solve.log` holds them for util.print_solve_log
    (no host sync inside the loop)."""
    B, n = x_init.shape
    m = C.shape[-1] - n
    x_init, C, c = _f32(x_init), _f32(C), _f32(c)
    # the stop rule (max full_du_norm < eps or n_not_improved > lim) cannot fire:
    # one launch per iteration, best_du formed at the end (same values).  The
    # per-iteration du planes are kept, so this mode is taken only while they
    # stay small: at most 1/16 of the free device memory and 2 GiB
    plane_bytes = 4 * lqr_iter * T * m * B
    fixed = (lqr_iter >= 1 and eps <= 0 and not_improved_lim >= lqr_iter
             and plane_bytes <= min(2 ** 31, torch.cuda.mem_get_info(x_init.device)[0] // 16))
    sv = MPCSolve(T, B, n, m, x_init.device, fixed_iters=lqr_iter if fixed else None)
    bounds, keep = N.make_bounds(u_lower, u_upper)
    if verbose > 0:
        _mpc_solve_logged(sv, model_id, theta, x_init, C, c, u_init, bounds, u_lower is None, lqr_iter, eps,
                          linesearch_decay, max_linesearch_iter, not_improved_lim, best_cost_eps)
    elif fixed:
        sv.solve_fixed(model_id, theta, x_init, C, c, bounds, linesearch_decay, max_linesearch_iter, best_cost_eps,
                       u_init)
    elif B <= SMALL_BATCH_MAX and model_id in SMALL_BATCH_MODELS and lqr_iter >= 1:
        # the whole stop-rule loop in one launch (one workgroup holds the batch)
        sv.solve_small(model_id, theta, x_init, C, c, bounds, linesearch_decay, max_linesearch_iter, lqr_iter,
                       best_cost_eps, eps, not_improved_lim, u_init)
    else:
        _mpc_solve_polled(sv, model_id, theta, x_init, C, c, u_init, bounds, lqr_iter, eps, linesearch_decay,
                          max_linesearch_iter, not_improved_lim, best_cost_eps, check_every)
    del keep
    x, u = sv.gather_best()
    return x, u, sv.best_cost, sv.best_du, sv


def _mpc_solve_polled(sv, model_id, theta, x_init, C, c, u_init, bounds, lqr_iter, eps, decay, max_ls,
                      not_improved_lim, best_cost_eps, check_every):
    """mpc_solve's stop-rule loop for a batch above one workgroup: runs of
    check_every iterations per library call (iterations after a stop are
    device no-ops).  The stop flag is polled without stalling the device:
    after each run the control word is copied to pinned host memory behind an
    event, and the host only waits for the copy of a run once POLL_AHEAD runs
    are queued behind it — so the GPU never drains while the host looks (a
    blocking poll every 8 iterations idled it once per poll), and at most
    POLL_AHEAD runs of no-op launches follow a stop."""
    sv.begin(model_id, theta, x_init, u_init)
    step = check_every if check_every else max(lqr_iter, 1)
    polls = collections.deque()
    n_polls = 0
    stream = torch.cuda.current_stream(x_init.device)
    for i0 in range(0, lqr_iter, step):
        sv.iterate_range(model_id, theta, x_init, C, c, bounds, decay, max_ls, i0, min(step, lqr_iter - i0),
                         best_cost_eps, eps, not_improved_lim)
        if i0 + step >= lqr_iter:
            return
        host = sv.poll_buffer(n_polls)            # a ring longer than the polls in flight
        n_polls += 1
        host.copy_(sv._ctrl_now(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        polls.append((ev, host))
        while polls and (len(polls) > POLL_AHEAD or polls[0][0].query()):
            ev0, host0 = polls.popleft()
            ev0.synchronize()
            if int(host0[1]):
                return


# (n, m) of the env_dx models (include/dilqr.h DILQR_MODEL_*)
MODEL_SHAPES = {N.MODEL_PENDULUM: (3, 1), N.MODEL_CARTPOLE: (5, 1), N.MODEL_ROCKET: (13, 3),
                N.MODEL_PENDULUM_COMPLEX: (3, 1)}
WARM_MODES = {"reference": N.WARM_REFERENCE, "shift": N.WARM_SHIFT, "cold": N.WARM_COLD}


def mpc_advance(model_id, theta_plant, u_plan, x_cur, u_warm, warm_mode, x_next_log, u_log, C=None, c=None,
                cost_log=None):
    """The step between two solves of a closed loop (dilqr_mpc_advance_f32,
    il_env.py:134-140), one launch, everything in place: x_cur [B,n] becomes the
    plant's f(x_cur, u_plan[0]) and is copied to x_next_log [B,n]; u_log [B,m]
    takes u_plan[0] as the solver gave it; u_warm [T,B,m] takes the plan
    shifted by warm_mode (a key of WARM_MODES or a DILQR_WARM_* value);
    cost_log [B] (optional, with the solve's C, c) takes the t = 0 stage cost
    at (x_cur, u_plan[0]).  x_next_log, u_log and cost_log may be rows of
    larger arrays."""
    T, B, m = u_plan.shape
    n = x_cur.shape[-1]
    # the kernel indexes every operand by the model's own (n, m)
    if (n, m) != MODEL_SHAPES.get(model_id, (n, m)):
        raise ValueError(f"dilqr: model {model_id} is (n, m) = {MODEL_SHAPES[model_id]}; got {(n, m)}")
    want = {"x_cur": (x_cur, (B, n)), "u_warm": (u_warm, (T, B, m)), "x_next_log": (x_next_log, (B, n)),
            "u_log": (u_log, (B, m)), "cost_log": (cost_log, (B,)), "C": (C, (T, B, n + m, n + m)),
            "c": (c, (T, B, n + m))}
    for name, (t, shape) in want.items():
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"dilqr: mpc_advance: {name} must be {shape}, got {tuple(t.shape)}")
    N.call("dilqr_mpc_advance_f32", int(model_id), T, B, N.ptr(theta_plant), N.ptr(u_plan), N.ptr(x_cur),
           N.ptr(u_warm), int(WARM_MODES.get(warm_mode, warm_mode)), N.ptr(C), N.ptr(c), N.ptr(x_next_log),
           N.ptr(u_log), N.ptr(cost_log), N.stream(u_plan.device))


def quad_traj_cost(x, u, C, c):
    """util.get_cost for a quadratic cost (util.py:130-153): per problem,
    sum_t 0.5 tau_t^T C_t tau_t + c_t^T tau_t, in torch on the device (the
    verbose report's initial cost only)."""
    tau = torch.cat((x, u), -1)
    return (0.5 * torch.einsum("tbi,tbij,tbj->tb", tau, C, tau) + (tau * c).sum(-1)).sum(0)


def _mpc_solve_logged(sv, model_id, theta, x_init, C, c, u_init, bounds, unbounded, lqr_iter, eps, decay, max_ls,
                      not_improved_lim, best_cost_eps):
    """mpc_solve with verbose > 0: the same kernels, one iteration per call,
    the table row's reductions queued after each on the launch stream."""
    dev = x_init.device
    stats = torch.zeros(max(lqr_iter, 1), 3, device=dev)
    sv.begin(model_id, theta, x_init, u_init)
    x0, u0 = sv.gather_best()                               # slot 0: get_traj(u_init)
    initial = quad_traj_cost(x0, u0, C, c).mean()
    T, m, B = sv.T, sv.m, sv.B
    for i in range(lqr_iter):
        if sv.fixed_iters:
            sv.iterate_fixed(model_id, theta, x_init, C, c, bounds, decay, max_ls, i, best_cost_eps)
            fdn = quirk_norm(sv.du_sq[i * T:(i + 1) * T])
        else:
            sv.iterate(model_id, theta, x_init, C, c, bounds, decay, max_ls, i, best_cost_eps, eps, not_improved_lim)
            fdn = sv.full_du_norm
        stats[i, 0] = sv.best_cost.mean()
        stats[i, 1] = fdn.max()
        stats[i, 2] = sv.alpha.mean()
    if sv.fixed_iters:
        sv.finish_fixed(lqr_iter)
    # the iterations that ran: the rule after iteration k is applied by
    # iteration k+1's prologue, which then publishes iter = k+1 with the stop
    # flag (dilqr_fused.h mpc_decide); a solve that never stopped ran them all
    ran = sv.iterations
    # total_qp_iters: 0 without bounds, as the reference (pnqp runs only with
    # bounds, lqr_step_explicit.py:137-150); the fused kernels do not count the
    # batch-coupled pnqp iterations the reference reports with bounds
    sv.log = {"initial_mean_cost": initial, "stats": stats, "iterations": ran, "qp_iters": 0 if unbounded else None}


def lqr_adjoint(C, c, F, x, u, dl_dx, dl_du, u_lower=None, u_upper=None, m_solver=N.SOLVE_INV, want_df=True):
    """Classic adjoint (lqr_step.py:312-407) -> dx_init, dC, dc, dF, df."""
    T, B, n = x.shape
    m = u.shape[2]
    d = n + m
    C, c, F, x, u, dl_dx, dl_du = map(_f32, (C, c, F, x, u, dl_dx, dl_du))
    bounds, keep = N.make_bounds(u_lower, u_upper)
    dev = C.device
    ws = torch.empty(T * B * (m * n + m), device=dev)
    dx0 = torch.empty(B, n, device=dev)
    dC = torch.empty(T, B, d, d, device=dev)
    dc = torch.empty(T, B, d, device=dev)
    dF = torch.empty(max(T - 1, 0), B, n, d, device=dev)
    df = torch.empty(max(T - 1, 0), B, n, device=dev) if want_df else None
    N.call("dilqr_lqr_adjoint_f32", n, m, T, B, N.ptr(C), N.ptr(c), N.ptr(F), N.ptr(x), N.ptr(u), N.ptr(dl_dx),
           N.ptr(dl_du), bounds, m_solver, N.ptr(ws), N.ptr(dx0), N.ptr(dC), N.ptr(dc), N.ptr(dF), N.ptr(df),
           N.stream(dev))
    del keep
    return dx0, dC, dc, dF, df


def mpc_solve_unfused(model_id, theta, x_init, C, c, T, F=None, f=None, u_init=None, u_lower=None,
                      u_upper=None, lqr_iter=10, eps=1e-7, linesearch_decay=0.2, max_linesearch_iter=10,
                      not_improved_lim=5, best_cost_eps=1e-4, check_every=8, u_zero_I=None, verbose=0,
                      delta_u=None):
    """The same outer loop with the unfused kernels (linearise -> F in HBM ->
    Riccati -> rollout/line search).  Used for LinDx dynamics (classic mpc.MPC,
    the adjoint engines), MPC(u_zero_I=...) and to cross-check the fused
    iteration.  u_zero_I [T,B,m] (bool): controls held at zero — the sweep's
    masked solve when unconstrained (lqr_step_explicit.py:98-129; with bounds
    the reference's pnqp branch ignores the mask) and zeroed in every rollout
    before the clamp (199-200).  An MlpModel or Mlp2Model (NNDynamics.
    device_model) in place of model_id, or MODEL_MLP with it as theta, runs the
    loop on the network; which of the two it is only the handle knows.  A
    one-hidden-layer MlpModel without a mask and with verbose <= 0 takes the
    route mlp_solve_route names instead of the four launches: the fused
    iteration (Dynamics.fused_iterate) + the best/stop rule per iteration, or
    the whole solve in one launch; both fill the same MPCWorkspace fields with
    the four launches' bits (best_x, best_u, best_cost, best_du, fdn, ctrl).
    A handle of slew_dynamics (with slew_problem's x_init, C, c) solves
    MPC(slew_rate_penalty=...) on a network: the four launches, the rollout,
    linearisation and line search being the dilqr_mlp*_slew_* entry points.

    delta_u: the trust region of MPC(delta_u=...) (bounds required, as in the
    reference, lqr_step_explicit.py:197), for any dynamics, always the four
    launches: every iteration's sweep takes the box relative to the current u
    clipped to +-delta_u (132-135; delta_sweep) and its line search clamps to
    u_t +- delta_u cut to the bounds (205-213), both formed from the current
    controls by torch ops on the stream and passed as tensor bounds; no host
    synchronisation besides the stop poll.

    The host polls the stop flag every `check_every` iterations: up to
    check_every - 1 iterations after the stop rule fired still run their
    linearise, sweep and line-search launches (these kernels carry no stop
    guard); their results are discarded by k_mpc_best, which leaves the best
    iterate, best_du and the control word as they were at the stop."""
    B, n = x_init.shape
    m = C.shape[-1] - n
    dev = x_init.device
    x_init, C, c = _f32(x_init), _f32(C), _f32(c)
    dyn = Dynamics.of(model_id, theta, n, m, F, f)
    if dyn.mlp is not None:
        # the network: the same four launches per iteration through the
        # dilqr_mlp_* / dilqr_mlp2_* entry points (rollout, linearise, line search)
        if tuple(C.shape) != (T, B, n + m, n + m) or tuple(c.shape) != (T, B, n + m):
            raise ValueError(f"dilqr: MLP model is (n, m) = {(n, m)}; got x_init {tuple(x_init.shape)}, "
                             f"C {tuple(C.shape)}, c {tuple(c.shape)} at T = {T}")
        if x_init.device != dyn.mlp.device:
            raise RuntimeError("dilqr: MLP weights and inputs are on different devices")
    if delta_u is not None and u_lower is None:
        raise NotImplementedError("dilqr: delta_u without u_lower is unimplemented in the reference too "
                                  "(lqr_step_explicit.py:197)")
    route = mlp_solve_route(dyn, B, lqr_iter, u_zero_I, verbose) if delta_u is None else "unfused"
    ws = MPCWorkspace(T, B, n, m, dev, fused=route != "unfused")
    s = N.stream(dev)
    bounds, keep = N.make_bounds(u_lower, u_upper)          # (keep: alive until every launch is queued)
    lim = _lim(not_improved_lim)
    if route == "small":
        # the whole stop-rule loop in one launch (one workgroup holds the batch)
        u0 = None if u_init is None else _al16(expand_u_init(u_init, T, B, m, dev).expand(T, B, m).contiguous())
        N.call("dilqr_mlp_mpc_solve_small_f32", n, m, T, B, dyn.mlp.desc, N.ptr(x_init), N.ptr(u0), N.ptr(C),
               N.ptr(c), bounds, float(linesearch_decay), int(max_linesearch_iter), int(lqr_iter),
               float(best_cost_eps), float(eps), lim, N.ptr(ws.xa), N.ptr(ws.ua), N.ptr(ws.xb),
               N.ptr(ws.ub), N.ptr(ws.ws), N.ptr(ws.cost), N.ptr(ws.alpha), N.ptr(ws.du_sq), N.ptr(ws.fdn),
               N.ptr(ws.best_x), N.ptr(ws.best_u), N.ptr(ws.best_cost), N.ptr(ws.best_du), N.ptr(ws.ctrl), s)
        return ws
    if u_init is None:
        ws.ua.zero_()
    else:
        ws.ua.copy_(expand_u_init(u_init, T, B, m, dev))
    zI = zero_mask(u_zero_I, T, B, m, dev)
    dyn.rollout(x_init, ws.ua, ws.xa)
    if route == "fused":
        # per iteration two library calls on the workspace's own buffers: the
        # fused iteration and the best-iterate / stop rule (both no-ops once the
        # rule fired); the flag is polled as below
        for i in range(lqr_iter):
            dyn.fused_iterate(x_init, C, c, ws.xa, ws.ua, bounds, linesearch_decay, max_linesearch_iter, ws.ws,
                              ws.xb, ws.ub, ws.cost, ws.du_sq, ws.alpha, old_cost=ws.cost if i > 0 else None,
                              ctrl=ws.ctrl)
            ws.update_best(i == 0, best_cost_eps, eps, lim)
            ws.swap()
            if ws.stop_seen(i, check_every, lqr_iter):
                break
        return ws
    stats = None
    if verbose > 0:                        # the table rows, reduced on the stream (util.print_solve_log)
        stats = torch.zeros(max(lqr_iter, 1), 3, device=dev)
        initial = quad_traj_cost(ws.xa, ws.ua, C, c).mean()
    ran = 0
    for i in range(lqr_iter):
        Fi, _ = dyn.linearize(ws.xa, ws.ua)
        if delta_u is None:
            K, k, _ = lqr_backward(C, c, Fi, n, m, x=ws.xa, u=ws.ua, u_lower=u_lower, u_upper=u_upper,
                                   u_zero_I=zI if u_lower is None else None)
        else:
            # the trust region around this iteration's controls, for the sweep and for the rollout
            K, k, _ = delta_sweep(C, c, Fi, n, m, ws.xa, ws.ua, u_lower, u_upper, delta_u=delta_u)
            bounds, keep = N.make_bounds(*delta_u_rollout_bounds(u_lower, u_upper, ws.ua, delta_u))
        # from iteration 1 the old cost is the previous line search's value for
        # the accepted candidate (ws.cost), as the fused MPC kernel takes it
        dyn.line_search(x_init, C, c, ws.xa, ws.ua, K, k, bounds, zI, linesearch_decay, max_linesearch_iter,
                        ws.xb, ws.ub, ws.cost, ws.du_sq, ws.alpha,
                        old_cost=ws.cost if i > 0 and dyn.carries_cost else None)
        ws.update_best(i == 0, best_cost_eps, eps, lim)
        if stats is not None:
            stats[i, 0] = ws.best_cost.mean()
            stats[i, 1] = ws.fdn.max()
            stats[i, 2] = ws.alpha.mean()
        ran = i + 1
        ws.swap()
        if ws.stop_seen(i, check_every, lqr_iter):
            break
    if stats is not None:
        # k_mpc_control counts the iterations that ran (ctrl[0]) and stops counting
        # once the rule fired (ctrl[1])
        if int(ws.ctrl[1].item()):
            ran = min(ran, int(ws.ctrl[0].item()))
        ws.log = {"initial_mean_cost": initial, "stats": stats, "iterations": ran,
                  "qp_iters": 0 if u_lower is None else None}
    return ws
