"""The iLQR loop for generic dynamics and costs.

What the fused HIP iteration cannot take — dynamics that are an arbitrary
torch Module (e.g. the reference's NNDynamics, dynamics.py:15-130), the
GradMethods.AUTO_DIFF / FINITE_DIFF linearisations (mpc_explicit.py:547-627),
non-quadratic costs expanded by autograd (approximate_cost, 468-508), the
slew-rate augmentation with CtrlPassthroughDynamics (383-466, dynamics.py:
133-156) and the delta_u trust region (lqr_step_explicit.py:202-215; for a
network with a device model these two have a device route behind
DEVICE_MLP_SLEW / DEVICE_MLP_DELTA_U, off by default) — runs
here: the user's Module is evaluated by torch on the GPU, batched over the
whole horizon wherever the reference loops over t, and every Riccati sweep
(+pnqp) is the HIP kernel (ops.lqr_backward, c_back fused).  The line search
follows lqr_step_explicit.py:166-263 with per-problem step sizes (the
reference's `torch.diag(alphas).mm(kt)` is O(B^2); here it is a broadcast),
the best-iterate bookkeeping and stop rule follow mpc_explicit.py:262-299.
One Module is not run by torch: an NNDynamics with a device model (one hidden
layer, sigmoid or relu; NNDynamics.device_model) goes through the HIP MLP
kernels, the gradient into its weights included — see DEVICE_MLP and
DEVICE_MLP_VJP below; with DEVICE_MLP_DEEP (off by default) one with two
hidden layers does too, and with DEVICE_MLP_DEEP_VJP (off by default) so does
that gradient (a first width of at most 128; wider ones keep the torch graph);
with DEVICE_MLP_DEEP_IMPLICIT (off by default) it trains through
mpc_explicit.MPC, the DiLQR implicit backward on its device model.  With
DEVICE_MLP_SLEW / DEVICE_MLP_DELTA_U (off by default) a solve of such a network
with a slew-rate penalty or with delta_u stays on device too.

lqr_step_forward is the one regular forward of an LQR step: the LQRStep
factories (lqr_step.py, lqr_step_explicit.py) call it too.  Whether its line
search runs in the kernels (on an ops.Dynamics handle) or in torch is decided
in one place, line_search_dynamics.

Nothing here is on the HIP hot path of the headline: those solves go through
ops.mpc_solve.  This module exists so that a user of the reference with any
dynamics or cost finds the same MPC API working on the GPU.
"""
import torch

from . import _native as N
from . import ops
from .definitions import LinDx, QuadCost


# ---------------------------------------------------------------- batched helpers (util.py:42-56)
def bmv(X, y):
    return torch.matmul(X, y.unsqueeze(-1)).squeeze(-1)


def bquad(x, Q):
    return (x.unsqueeze(-2) @ Q @ x.unsqueeze(-1)).squeeze(-1).squeeze(-1)


def bdot(x, y):
    return (x * y).sum(-1)


def eclamp(x, lo, hi):
    """util.eclamp (util.py:58-72): the bound values are written exactly."""
    lo_t = lo if isinstance(lo, torch.Tensor) else torch.full_like(x, float(lo))
    hi_t = hi if isinstance(hi, torch.Tensor) else torch.full_like(x, float(hi))
    x = torch.where(x < lo_t, lo_t, x)
    return torch.where(x > hi_t, hi_t, x)


def quad_stage_cost(tau, C, c):
    return 0.5 * bquad(tau, C) + bdot(tau, c)


# ---------------------------------------------------------------- the device MLP route
# A dynamics Module with a device model (NNDynamics.device_model: one hidden
# layer, sigmoid/relu, within the kernels' shapes) runs its rollouts, its
# ANALYTIC linearisation, its line search and, for a quadratic cost without
# slew-rate penalty or delta_u, the whole solve through the HIP MLP kernels
# (csrc/tu_mlp.hip).  False restores the torch loop everywhere (tests and
# tools/bench_nn_mpc.py run both on the same inputs).
DEVICE_MLP = True
# With DEVICE_MLP, the differentiable ANALYTIC linearisation of final_step (the
# one place a solve's gradient reaches the network's weights) is the same
# kernel with a HIP backward (ops.mlp_linearize_diff, csrc/tu_mlp_vjp.hip).
# False keeps the torch graph through NNDynamics.grad_input for it.
DEVICE_MLP_VJP = True
# With DEVICE_MLP, a module with two hidden layers takes the same routes on its
# own device model (ops.Mlp2Model, csrc/tu_mlp2.hip): rollout, the ANALYTIC
# linearisation without gradient, the line search and the whole solve.  Its
# gradient stays on the torch graph through grad_input unless
# DEVICE_MLP_DEEP_VJP says otherwise.  Off: such a module runs in torch, as it
# always has.
DEVICE_MLP_DEEP = False
# With DEVICE_MLP, DEVICE_MLP_DEEP and DEVICE_MLP_VJP, the differentiable
# ANALYTIC linearisation of final_step for a two-hidden-layer module inside the
# device VJP's envelope (ops.Mlp2Model.vjp_ok: a first width of at most
# N.MLP2_VJP_MAX_HIDDEN1) is the Mlp2 kernel with a HIP backward into the six
# parameters (ops.mlp2_linearize_diff, csrc/tu_mlp2_vjp.hip).  Off, or outside
# the envelope: the torch graph through NNDynamics.grad_input.
DEVICE_MLP_DEEP_VJP = False
# With DEVICE_MLP, the DiLQR implicit backward of final_step (mpc_explicit.MPC)
# for a one-hidden-layer module, a quadratic cost, the ANALYTIC linearisation,
# no slew-rate penalty, delta_u or u_zero_I is a HIP kernel on the device model
# (ops.mlp_implicit_step, csrc/tu_mlp_implicit.hip): the derivative of the iLQR
# fixed point with the network's curvature; its dF, df reach the weights through
# the linearisation's backward (DEVICE_MLP_VJP, or the torch graph).  Off, or
# outside that envelope: the refusal final_step has always given.
DEVICE_MLP_IMPLICIT = True
# With DEVICE_MLP, DEVICE_MLP_DEEP and DEVICE_MLP_IMPLICIT, the same for a
# two-hidden-layer module inside the kernel's envelope
# (ops.Mlp2Model.implicit_ok: a first width of at most
# N.MLP2_IMPLICIT_MAX_HIDDEN1; csrc/tu_mlp2_implicit.hip): its dF, df reach the
# six parameters through the linearisation's backward (DEVICE_MLP_DEEP_VJP, or
# the torch graph).  Off, or outside the envelope: the refusal, as it always has
# been for such a module.
DEVICE_MLP_DEEP_IMPLICIT = False
# With DEVICE_MLP (and DEVICE_MLP_DEEP for two hidden layers), a solve with a
# slew-rate penalty that is otherwise inside device_solve_ok's envelope (a
# quadratic cost, ANALYTIC, no delta_u, not verbose) runs on device as the plain
# solve of the augmented system (ops.slew_problem, ops.mpc_solve_unfused on
# ops.slew_dynamics: the reference's CtrlPassthroughDynamics as a HIP model,
# csrc/dilqr_ctrl_through.h), when the augmented (n + m, m) is a shape the
# kernels are compiled for.  The gradient is unchanged: final_step's
# differentiable linearisation of the network, slew_augment, the classic
# adjoint.  Off: the torch loop, as it always has been.
DEVICE_MLP_SLEW = False
# With DEVICE_MLP (and DEVICE_MLP_DEEP), a solve with delta_u and no slew-rate
# penalty, otherwise inside device_solve_ok's envelope, runs on device
# (ops.mpc_solve_unfused(delta_u=...): the trust region as per-iteration tensor
# bounds of the sweep and the line search), and one LQR step with delta_u takes
# the device line search on the network as it does on an env_dx model
# (line_search_dynamics).  Off: the torch loop / torch line search.  Both
# options at once stay in torch whatever the switches say.
DEVICE_MLP_DELTA_U = False


def device_mlp(dynamics, like):
    """dynamics' ops.MlpModel (with DEVICE_MLP_DEEP possibly an ops.Mlp2Model)
    for tensors like `like` (a GPU fp32 tensor), or None."""
    dyn = ops.device_dynamics(dynamics, like, env=False, mlp=DEVICE_MLP, deep=DEVICE_MLP_DEEP)
    return None if dyn is None else dyn.mlp


def device_solve_ok(mpc, cost, dx, x_init):
    """The MlpModel when the whole solve can run on device (ops.mpc_solve_unfused
    on the MLP model): a device model, a quadratic cost, the ANALYTIC
    linearisation, no slew-rate penalty, no delta_u, not verbose (the torch
    loop's table prints the pnqp count, which the device loop does not form)."""
    from .mpc_explicit import GradMethods
    if not (isinstance(cost, QuadCost) and mpc.grad_method == GradMethods.ANALYTIC
            and mpc.slew_rate_penalty is None and mpc.delta_u is None and getattr(mpc, "verbose", 0) <= 0):
        return None
    return device_mlp(dx, x_init)


def device_option_solve_ok(mpc, cost, dx, x_init):
    """("slew", handle) or ("delta_u", handle) when the whole solve of an MPC
    with exactly one of the two options can run on device — device_solve_ok's
    envelope otherwise, the option's switch on (DEVICE_MLP_SLEW,
    DEVICE_MLP_DELTA_U), a device model of the solve's (n, m) and, for the
    slew-rate penalty, an augmented shape the kernels are compiled for; the
    handle is the ops.Dynamics the solve runs on.  None otherwise."""
    from .mpc_explicit import GradMethods
    slew, trust = mpc.slew_rate_penalty is not None, mpc.delta_u is not None
    if slew == trust or not (DEVICE_MLP_SLEW if slew else DEVICE_MLP_DELTA_U):
        return None
    if not (isinstance(cost, QuadCost) and mpc.grad_method == GradMethods.ANALYTIC
            and getattr(mpc, "verbose", 0) <= 0):
        return None
    mlp = device_mlp(dx, x_init)
    if mlp is None or (mlp.n, mlp.m) != (mpc.n_state, mpc.n_ctrl):
        return None
    dyn = ops.slew_dynamics(mlp) if slew else ops.Dynamics(mlp, mlp.n, mlp.m)
    return None if dyn is None else ("slew" if slew else "delta_u", dyn)


def implicit_mlp_ok(mpc, cost, dx, x_init):
    """The device model when final_step's DiLQR implicit backward can run on
    device (ops.mlp_implicit_step): DEVICE_MLP_IMPLICIT, a one-hidden-layer
    device model of the solve's (n, m) — or, with DEVICE_MLP_DEEP and
    DEVICE_MLP_DEEP_IMPLICIT, a two-hidden-layer one that is implicit_ok —, a
    quadratic cost, the ANALYTIC linearisation, no slew-rate penalty, no
    delta_u, no u_zero_I mask."""
    from .mpc_explicit import GradMethods
    if not (DEVICE_MLP_IMPLICIT and isinstance(cost, QuadCost) and mpc.grad_method == GradMethods.ANALYTIC
            and mpc.slew_rate_penalty is None and mpc.delta_u is None and getattr(mpc, "u_zero_I", None) is None):
        return None
    if getattr(dx, "model_id", None) is not None or not hasattr(dx, "grad_input"):
        return None
    mlp = device_mlp(dx, x_init)
    deep = DEVICE_MLP_DEEP_IMPLICIT and isinstance(mlp, ops.Mlp2Model) and mlp.implicit_ok
    if not (isinstance(mlp, ops.MlpModel) or deep) or (mlp.n, mlp.m) != (mpc.n_state, mpc.n_ctrl):
        return None
    return mlp


# ---------------------------------------------------------------- dynamics / cost wrappers
class CtrlPassthroughDynamics(torch.nn.Module):
    """dynamics.py:133-156: state [u_{t-1}; x_t] -> [u_t; f(x_t, u_t)]."""

    def __init__(self, dynamics):
        super().__init__()
        self.dynamics = dynamics

    def forward(self, tilde_x, u):
        squeeze = tilde_x.ndimension() == 1
        if squeeze:
            tilde_x = tilde_x.unsqueeze(0)
        if u.ndimension() == 1:
            u = u.unsqueeze(0)
        n_ctrl = u.size(1)
        out = torch.cat((u, self.dynamics(tilde_x[:, n_ctrl:], u)), dim=1)
        return out.squeeze(0) if squeeze else out


class SlewRateCost(torch.nn.Module):
    """mpc_explicit.py:35-55: cost(true tau) + 1/2 tau^T slew_C tau."""

    def __init__(self, cost, slew_C, n_state, n_ctrl):
        super().__init__()
        self.cost, self.slew_C, self.n_state, self.n_ctrl = cost, slew_C, n_state, n_ctrl

    def forward(self, tau):
        return self.cost(tau[:, self.n_ctrl:]) + 0.5 * bquad(tau, self.slew_C[0])


def next_state(dynamics, t, x, u):
    """x_{t+1}: a LinDx's F_t [x; u] (+ f_t), any other dynamics called as a Module."""
    if not isinstance(dynamics, LinDx):
        return dynamics(x, u)
    nx = bmv(dynamics.F[t], torch.cat((x, u), 1))
    return nx if dynamics.f is None or dynamics.f.nelement() == 0 else nx + dynamics.f[t]


def rollout(T, u, x_init, dynamics):
    """util.get_traj (util.py:104-127)."""
    mlp = device_mlp(dynamics, x_init)
    if mlp is not None:
        return ops.mlp_rollout(mlp, x_init.detach(), u.detach())
    x = [x_init.detach()]
    with torch.no_grad():
        for t in range(T - 1):
            x.append(next_state(dynamics, t, x[t], u[t].detach()).detach())
    return torch.stack(x, 0)


def traj_cost(T, x, u, cost):
    """util.get_cost (util.py:130-153) on a given trajectory; returns [B]."""
    with torch.no_grad():
        tau = torch.cat((x, u), 2)
        if isinstance(cost, QuadCost):
            return quad_stage_cost(tau, cost.C, cost.c).sum(0)
        return torch.stack([cost(tau[t]) for t in range(T)], 0).sum(0)


# ---------------------------------------------------------------- linearisation
def linearize(mpc, x, u, dynamics, diff):
    """MPC.linearize_dynamics (mpc_explicit.py:511-627, mpc.py:490-601) for
    every grad method, batched over the horizon: the (T-1)*B rows go through
    the dynamics as one batch (the reference loops over t; per-row dynamics give
    the same rows).  Returns F [T-1,B,n,n+m], f [T-1,B,n]."""
    from .mpc_explicit import GradMethods
    T, B, n = x.shape
    m = u.shape[2]
    dev = x.device
    if T < 2:
        return torch.zeros(0, B, n, n + m, device=dev), torch.zeros(0, B, n, device=dev)
    mid = getattr(dynamics, "model_id", None)
    gm = mpc.grad_method
    if gm == GradMethods.ANALYTIC and mid is not None and not diff:
        # the env_dx models: the HIP linearisation (get_linear_dyn, unclamped u)
        return ops.linearize(mid, ops.theta_of(dynamics, x), x.detach(), u.detach())
    if gm == GradMethods.ANALYTIC and not diff and mid is None and hasattr(dynamics, "grad_input"):
        mlp = device_mlp(dynamics, x)
        if mlp is not None:
            # the network: value and grad_input's [R S] of every row in one kernel
            return ops.mlp_linearize(mlp, x.detach(), u.detach())
    if gm == GradMethods.ANALYTIC and diff and mid is None and hasattr(dynamics, "grad_input") and DEVICE_MLP_VJP:
        mlp = device_mlp(dynamics, x)
        one = isinstance(mlp, ops.MlpModel)
        if one or (DEVICE_MLP_DEEP_VJP and isinstance(mlp, ops.Mlp2Model) and mlp.vjp_ok):
            # the same kernel, with the device VJP of its kind of network into the module's own
            # parameters as its backward (any other two-layer model differentiates through
            # grad_input below)
            params = tuple(p for fc in dynamics.fcs for p in (fc.weight, fc.bias))
            diff_of = ops.mlp_linearize_diff if one else ops.mlp2_linearize_diff
            return diff_of(mlp, params, x.detach(), u.detach())
    xs = x[:-1].detach().reshape(-1, n)
    us = u[:-1].detach().reshape(-1, m)
    if gm == GradMethods.ANALYTIC:
        if mid is not None:
            # env_dx model, differentiable linearisation: get_linear_dyn
            # (mpc_explicit.py:516-546) on the autograd path of the model
            with torch.enable_grad():
                new_x = dynamics(xs, us)
                D = dynamics.get_linear_dyn(xs, us)
            f = new_x - bmv(D, torch.cat((xs, us), 1))
            return D.view(T - 1, B, n, n + m), f.view(T - 1, B, n)
        if not hasattr(dynamics, "grad_input"):
            raise ValueError("GradMethods.ANALYTIC needs dynamics.grad_input(x, u) -> (R, S)")
        # mpc.py:494-519: R, S from the model's grad_input (NNDynamics: the
        # chain of its weights, differentiable when diff)
        xs = xs.clone().requires_grad_(True)
        us = us.clone().requires_grad_(True)
        with torch.enable_grad():
            new_x = dynamics(xs, us)
            if not diff:
                new_x, xs, us = new_x.detach(), xs.detach(), us.detach()
            R, S = dynamics.grad_input(xs, us)
            f = new_x - bmv(R, xs) - bmv(S, us)
        F = torch.cat((R, S), 2)
        if not diff:
            F, f = F.detach(), f.detach()
        return F.view(T - 1, B, n, n + m), f.view(T - 1, B, n)
    if gm == GradMethods.AUTO_DIFF:
        # mpc_explicit.py:566-576: one backward per state component, without
        # create_graph (so F carries no graph; f does, through new_x)
        xs = xs.clone().requires_grad_(True)
        us = us.clone().requires_grad_(True)
        with torch.enable_grad():
            new_x = dynamics(xs, us)
            Rs, Ss = [], []
            for j in range(n):
                Rj, Sj = torch.autograd.grad(new_x[:, j].sum(), [xs, us], retain_graph=True)
                Rs.append(Rj)
                Ss.append(Sj)
            R, S = torch.stack(Rs, 1), torch.stack(Ss, 1)
            if not diff:
                new_x, xs, us = new_x.detach(), xs.detach(), us.detach()
            f = new_x - bmv(R, xs) - bmv(S, us)
        F = torch.cat((R, S), 2)
        if not diff:
            f = f.detach()
        return F.view(T - 1, B, n, n + m), f.view(T - 1, B, n)
    if gm == GradMethods.FINITE_DIFF:
        # mpc_explicit.py:598-611 with util.jacobian (util.py:10-20): central
        # differences, eps = 1e-4, every row at once.  With diff the quotients
        # keep their graph (the reference differentiates F through them too)
        eps = 1e-4
        with torch.set_grad_enabled(diff):
            new_x = dynamics(xs, us)
            Rc, Sc = [], []
            for i in range(n):
                e = torch.zeros_like(xs)
                e[:, i] = eps
                Rc.append((dynamics(xs + e, us) - dynamics(xs - e, us)) / (2. * eps))
            for i in range(m):
                e = torch.zeros_like(us)
                e[:, i] = eps
                Sc.append((dynamics(xs, us + e) - dynamics(xs, us - e)) / (2. * eps))
            R, S = torch.stack(Rc, 2), torch.stack(Sc, 2)
            f = new_x - bmv(R, xs) - bmv(S, us)
        F = torch.cat((R, S), 2)
        if not diff:
            f = f.detach()
        return F.view(T - 1, B, n, n + m), f.view(T - 1, B, n)
    raise NotImplementedError(f"dilqr: grad_method {gm} is not implemented")


def approximate_cost(x, u, cost, diff):
    """MPC.approximate_cost (mpc_explicit.py:468-508): the cost's Hessian and
    gradient at tau by autograd, all T*B rows at once.  Returns C [T,B,d,d],
    c [T,B,d] (= grad - H tau), stage costs [T,B]."""
    T, B, n = x.shape
    d = n + u.shape[2]
    with torch.enable_grad():
        tau = torch.cat((x, u), 2).detach().reshape(T * B, d).requires_grad_(True)
        val = cost(tau)
        grad = torch.autograd.grad(val.sum(), tau, create_graph=True)[0]
        H = torch.stack([torch.autograd.grad(grad[:, i].sum(), tau, create_graph=True)[0] for i in range(d)], -1)
        c = grad - bmv(H, tau)
    H, c, val = H.view(T, B, d, d), c.view(T, B, d), val.view(T, B)
    if not diff:
        return H.detach(), c.detach(), val.detach()
    return H, c, val


# ---------------------------------------------------------------- one LQR step (forward)
def line_search_dynamics(true_cost, true_dynamics, x, delta_u, env_models):
    """The ops.Dynamics handle the step's line search runs on in the kernels, or
    None for the torch loop.  This is the whole routing rule of an LQR step:
      * not a QuadCost -> torch;
      * an env_dx model or a LinDx (env_models: asked for by the LQRStep
        factories only; the generic MPC loop has always run them in torch, its
        own use of them being delta_u, the slew-rate penalty and the autograd /
        finite-difference linearisations) -> device, with any delta_u;
      * a dynamics Module with a device model (DEVICE_MLP) -> device with the
        full [T,B,d,d] / [T,B,d] QuadCost, and with delta_u only when
        DEVICE_MLP_DELTA_U says so (the caller then clamps the rollout to
        ops.delta_u_rollout_bounds, as for the env_dx models);
      * any other Module -> torch."""
    if not isinstance(true_cost, QuadCost):
        return None
    dyn = ops.device_dynamics(true_dynamics, x, env=env_models, mlp=DEVICE_MLP, deep=DEVICE_MLP_DEEP)
    if dyn is None or dyn.mlp is None:
        return dyn
    T, B, d = x.shape[0], x.shape[1], dyn.n + dyn.m
    full = tuple(true_cost.C.shape) == (T, B, d, d) and tuple(true_cost.c.shape) == (T, B, d)
    return dyn if (delta_u is None or DEVICE_MLP_DELTA_U) and full else None


def lqr_step_forward(T, n, m, x_init, C, c, F, x, u, true_cost, true_dynamics, u_lower, u_upper, delta_u,
                     decay, max_ls, u_zero_I=None, extras=False, env_models=False):
    """LQRStepFn.forward of the DiLQR step (lqr_step_explicit.py:625-650), the
    one regular forward of both LQRStep factories and of the generic loop: the
    HIP Riccati sweep in delta space (ops.delta_sweep), then the line search of
    lqr_forward (166-263) with the true dynamics/cost, in the kernels or in
    torch as line_search_dynamics rules.  Returns (new_x, new_u, costs [B],
    full_du_norm [B]); with extras also the final step sizes [B] (in torch one
    decay undone where the last pass still failed, 254-255) and the sweep's
    pnqp iteration count (formed only then, and only with bounds)."""
    B = x.shape[1]
    lo, hi = (v if v is None or isinstance(v, (int, float)) else v.detach().contiguous() for v in (u_lower, u_upper))
    if delta_u is not None and lo is None:
        raise NotImplementedError("dilqr: delta_u without u_lower is unimplemented in the reference too "
                                  "(lqr_step_explicit.py:197)")
    zI = None if u_zero_I is None else u_zero_I.detach()
    xd, ud = x.detach().contiguous(), u.detach().contiguous()
    K, k, nqp = ops.delta_sweep(C.detach().contiguous(), c.detach().contiguous(), F.detach().contiguous(), n, m,
                                xd, ud, lo, hi, zI, delta_u, qp_total=extras and lo is not None)
    n_qp = nqp if isinstance(nqp, int) else 0
    # with delta_u the rollout's clamp is u_t +- delta_u cut to the bounds (205-213)
    flo, fhi = (lo, hi) if delta_u is None else ops.delta_u_rollout_bounds(lo, hi, ud, delta_u)
    dyn = line_search_dynamics(true_cost, true_dynamics, xd, delta_u, env_models)
    if dyn is not None:
        # the same per-problem rule on device; du_sq is the first pass's, alphas the last pass's
        new_x, new_u, cur_cost, du_sq, alphas = ops.lqr_forward(
            dyn, None, x_init.detach(), true_cost.C.detach(), true_cost.c.detach(), xd, ud, K, k, u_lower=flo,
            u_upper=fhi, u_zero_I=zI, linesearch_decay=decay, max_linesearch_iter=max_ls)
        full_du_norm = ops.quirk_norm(du_sq)
        return (new_x, new_u, cur_cost, full_du_norm) + ((alphas, n_qp) if extras else ())
    if zI is not None:
        zI = zI.bool()
    old_cost = traj_cost(T, x, u, true_cost)
    alphas = torch.ones(B, device=x.device)
    cur_cost, full_du_norm = None, None
    i = 0
    with torch.no_grad():
        while (cur_cost is None or bool((cur_cost > old_cost).any())) and i < max_ls:
            new_u, new_x, dxs, objs = [], [x_init.detach()], torch.zeros_like(x_init), []
            for t in range(T):
                nu = bmv(K[t], dxs) + u[t] + alphas.unsqueeze(1) * k[t]
                if zI is not None:                              # lqr_step_explicit.py:199-200
                    nu = torch.where(zI[t], torch.zeros_like(nu), nu)
                if flo is not None:
                    nu = eclamp(nu, *(v if isinstance(v, (int, float)) else v[t] for v in (flo, fhi)))
                new_u.append(nu)
                tau = torch.cat((new_x[t], nu), 1)
                if t < T - 1:
                    nx = next_state(true_dynamics, t, new_x[t], nu)
                    new_x.append(nx)
                    dxs = nx - x[t + 1]
                if isinstance(true_cost, QuadCost):
                    objs.append(quad_stage_cost(tau, true_cost.C[t], true_cost.c[t]))
                else:
                    objs.append(true_cost(tau))
            cur_cost = torch.stack(objs).sum(0)
            new_u = torch.stack(new_u)
            new_x = torch.stack(new_x)
            if full_du_norm is None:                        # 245-247: the batch-mixing view
                full_du_norm = (u - new_u).transpose(1, 2).contiguous().view(B, -1).norm(2, 1)
            alphas = torch.where(cur_cost > old_cost, alphas * decay, alphas)
            i += 1
        if extras:
            alphas = torch.where(cur_cost > old_cost, alphas / decay, alphas)
    return (new_x, new_u, cur_cost, full_du_norm) + ((alphas, n_qp) if extras else ())


# ---------------------------------------------------------------- the slew-rate augmentation
def slew_augment(mpc, x_init, C, c, F, f, cost, dynamics, x, u):
    """solve_lqr_subproblem's slew-rate branch (mpc_explicit.py:383-466): the
    state becomes [u_{t-1}; x_t] with cost gamma/2 |u_t - u_{t-1}|^2 added."""
    T, n, m = mpc.T, mpc.n_state, mpc.n_ctrl
    B = C.size(1)
    nsc = n + m
    dev, dt = C.device, C.dtype
    _x_init, _C, _c = ops.slew_problem(x_init, C, c, mpc.slew_rate_penalty, mpc.prev_ctrl, m)
    _F0 = torch.cat((torch.zeros(m, n + m, device=dev, dtype=dt), torch.eye(m, device=dev, dtype=dt)), 1)
    _F0 = _F0.expand(T - 1, B, m, nsc + m)
    _F1 = torch.cat((torch.zeros(T - 1, B, n, m, device=dev, dtype=dt), F), 3)
    _F = torch.cat((_F0, _F1), 2)
    _f = None if f is None else torch.cat((torch.zeros(T - 1, B, m, device=dev, dtype=dt), f), 2)
    prev_u = ops.slew_prev_ctrl(mpc.prev_ctrl, B, m, dev, dt)
    utm1s = torch.cat((prev_u.expand(1, B, m), u.detach()[:-1]))
    _x = torch.cat((utm1s, x), 2)
    _dyn = None if isinstance(dynamics, LinDx) else CtrlPassthroughDynamics(dynamics)
    _cost = QuadCost(_C, _c) if isinstance(cost, QuadCost) else SlewRateCost(
        cost, ops.slew_cost_block(T, B, n, m, mpc.slew_rate_penalty, dev, dt), n, m)
    return _x_init, _C, _c, _F, _f, _dyn, _cost, _x


def solve_subproblem(mpc, x_init, C, c, F, f, cost, dynamics, x, u, extras=False):
    """One LQR step of the outer loop (solve_lqr_subproblem, mpc_explicit.py:360-466).
    extras: also the step sizes and the pnqp count (the verbose table)."""
    T, n, m = mpc.T, mpc.n_state, mpc.n_ctrl
    if mpc.slew_rate_penalty is None or isinstance(cost, torch.nn.Module):
        return lqr_step_forward(T, n, m, x_init, C, c, F, x, u, cost, dynamics, mpc.u_lower, mpc.u_upper,
                                mpc.delta_u, mpc.linesearch_decay, mpc.max_linesearch_iter,
                                getattr(mpc, "u_zero_I", None), extras=extras)
    _x_init, _C, _c, _F, _f, _dyn, _cost, _x = slew_augment(mpc, x_init, C, c, F, f, cost, dynamics, x, u)
    true_dyn = _dyn if _dyn is not None else LinDx(_F, _f)
    out = lqr_step_forward(T, n + m, m, _x_init, _C, _c, _F, _x, u, _cost, true_dyn, mpc.u_lower,
                           mpc.u_upper, mpc.delta_u, mpc.linesearch_decay, mpc.max_linesearch_iter,
                           getattr(mpc, "u_zero_I", None), extras=extras)
    return (out[0][:, :, m:],) + tuple(out[1:])


# ---------------------------------------------------------------- the outer loop
def solve(mpc, x_init, cost, dx, n_batch):
    """mpc_explicit.MPC.forward / mpc.MPC.forward loop (mpc_explicit.py:226-299)
    for generic dynamics/costs.  Returns (best x, best u, best costs, best
    full_du_norm), all detached."""
    T, n, m = mpc.T, mpc.n_state, mpc.n_ctrl
    dev = x_init.device
    mlp = device_solve_ok(mpc, cost, dx, x_init)
    if mlp is not None and (mlp.n, mlp.m) == (n, m):
        # the whole loop on device: rollout, linearise, sweep, line search and the
        # best-iterate / stop rule, four launches per iteration, no host poll
        # between them (ops.mpc_solve_unfused on the MLP model)
        from .mpc_explicit import MPC
        with torch.no_grad():
            ws = ops.mpc_solve_unfused(
                mlp, None, x_init.detach(), cost.C.detach().contiguous(), cost.c.detach().contiguous(), T,
                u_zero_I=getattr(mpc, "u_zero_I", None), **MPC.solver_args(mpc))
        return ws.best_x, ws.best_u, ws.best_cost, ws.best_du
    option = device_option_solve_ok(mpc, cost, dx, x_init)
    if option is not None:
        # one of the two options on device: the slew-rate penalty as the plain
        # solve of the augmented system on the control-passthrough model, or
        # delta_u as per-iteration tensor bounds; four launches per iteration
        from .mpc_explicit import MPC
        which, dyn = option
        x0, C, c = x_init.detach(), cost.C.detach().contiguous(), cost.c.detach().contiguous()
        with torch.no_grad():
            if which == "slew":
                x0, C, c = ops.slew_problem(x0, C, c, mpc.slew_rate_penalty, mpc.prev_ctrl, m)
            ws = ops.mpc_solve_unfused(dyn, None, x0.contiguous(), C, c, T, u_zero_I=getattr(mpc, "u_zero_I", None),
                                       delta_u=mpc.delta_u, **MPC.solver_args(mpc))
        best_x = ws.best_x[:, :, m:] if which == "slew" else ws.best_x
        return best_x, ws.best_u, ws.best_cost, ws.best_du
    if mpc.u_init is None:
        u = torch.zeros(T, n_batch, m, device=dev, dtype=x_init.dtype)
    else:
        u = ops.expand_u_init(mpc.u_init, T, n_batch, -1, dev, x_init.dtype)
        if mpc.u_init.ndimension() == 2:
            u = u.clone()
    x_init = x_init.detach()
    best = None
    n_not_improved = 0
    verbose = getattr(mpc, "verbose", 0) > 0
    if verbose:                                                          # mpc_explicit.py:236-241
        x0 = rollout(T, u, x_init, dx)
        print("Initial mean(cost): {:.4e}".format(float(traj_cost(T, x0, u, cost).mean())))
    for it in range(mpc.lqr_iter):
        u = u.detach()
        x = rollout(T, u, x_init, dx)
        if isinstance(dx, LinDx):
            F, f = dx.F.detach(), (None if dx.f is None or dx.f.nelement() == 0 else dx.f.detach())
        else:
            F, f = linearize(mpc, x, u, dx, diff=False)
        if isinstance(cost, QuadCost):
            C, c = cost.C.detach(), cost.c.detach()
        else:
            C, c, _ = approximate_cost(x, u, cost, diff=False)
        out = solve_subproblem(mpc, x_init, C, c, F, f, cost, dx, x, u, extras=verbose)
        x, u, costs, full_du_norm = out[:4]
        n_not_improved += 1
        if best is None:
            best = {"x": x.clone(), "u": u.clone(), "costs": costs.clone(), "fdn": full_du_norm.clone()}
        else:
            take = costs <= best["costs"] + mpc.best_cost_eps           # mpc_explicit.py:277-283
            if bool(take.any()):
                n_not_improved = 0
            best["x"][:, take] = x[:, take]
            best["u"][:, take] = u[:, take]
            best["costs"][take] = costs[take]
            best["fdn"][take] = full_du_norm[take]
        if verbose:                                                      # mpc_explicit.py:285-295
            from .util import table_log
            table_log("lqr", (("iter", it), ("mean(cost)", float(best["costs"].mean()), "{:.4e}"),
                              ("||full_du||_max", float(full_du_norm.max()), "{:.2e}"),
                              ("mean(alphas)", float(out[4].mean()), "{:.2e}"), ("total_qp_iters", out[5])))
        if float(full_du_norm.max()) < mpc.eps or n_not_improved > mpc.not_improved_lim:   # 297-299
            break
    return best["x"], best["u"], best["costs"], best["fdn"]


def final_step(mpc, x_init, cost, dx, x, u, classic):
    """The reference's closing no-op LQR step (mpc_explicit.py:302-325,
    mpc.py:299-318): linearise at the best iterate WITH gradients (the
    autograd linearisation / cost expansion graphs carry them to the dynamics'
    and cost's parameters; for a network with a device model the linearisation
    and its backward are HIP kernels, DEVICE_MLP_VJP), then the no-op step whose
    backward is the classic adjoint kernel (classic=True) or the DiLQR implicit
    backward: an env_dx model's, or for a network inside implicit_mlp_ok's
    envelope the kernel on its device model (DEVICE_MLP_IMPLICIT; for two hidden
    layers DEVICE_MLP_DEEP_IMPLICIT as well)."""
    from .lqr_step import LQRStep as ClassicStep
    from .lqr_step_explicit import LQRStep as ExplicitStep
    T, n, m = mpc.T, mpc.n_state, mpc.n_ctrl
    if isinstance(dx, LinDx):
        F, f = dx.F, dx.f
    else:
        F, f = linearize(mpc, x, u, dx, diff=True)
    if isinstance(cost, QuadCost):
        C, c = cost.C, cost.c
    else:
        C, c, _ = approximate_cost(x, u, cost, diff=True)
    if f is None:
        f = torch.empty(0, device=x.device)
    if mpc.slew_rate_penalty is not None and not isinstance(cost, torch.nn.Module):
        _x_init, _C, _c, _F, _f, _dyn, _cost, _x = slew_augment(mpc, x_init, C, c, F, f if f.nelement() else None,
                                                                cost, dx, x, u)
        if not classic:
            raise NotImplementedError("dilqr: the DiLQR implicit backward with a slew-rate penalty")
        step = ClassicStep(n + m, m, T, u_lower=mpc.u_lower, u_upper=mpc.u_upper, true_cost=_cost,
                           true_dynamics=_dyn if _dyn is not None else LinDx(_F, _f), current_x=_x.detach(),
                           current_u=u.detach(), back_eps=mpc.back_eps, no_op_forward=True)
        xa, ua = step(_x_init, _C, _c, _F, _f if _f is not None else torch.empty(0, device=x.device))
        return xa[:, :, m:], ua
    if classic:
        step = ClassicStep(n, m, T, u_lower=mpc.u_lower, u_upper=mpc.u_upper, true_cost=QuadCost(C, c),
                           true_dynamics=dx, current_x=x.detach(), current_u=u.detach(), back_eps=mpc.back_eps,
                           no_op_forward=True)
        return step(x_init, C, c, F, f)
    mlp = implicit_mlp_ok(mpc, cost, dx, x_init)
    if mlp is not None:
        # the network: the implicit backward kernel on its device model; dF, df
        # go on through F, f into the linearisation's backward above
        return ops.mlp_implicit_step(mlp, x_init, C, c, F, f, x, u, u_lower=mpc.u_lower, u_upper=mpc.u_upper)
    if getattr(dx, "model_id", None) not in (N.MODEL_CARTPOLE, N.MODEL_PENDULUM, N.MODEL_ROCKET):
        # the DiLQR implicit backward needs an env_dx model's second derivatives
        # (the reference reads dx.params and dx.grad_input and raises without
        # them, mpc_explicit.py:325, lqr_step_explicit.py:703): a caller whose
        # inputs carry gradients gets the same refusal, never a silently
        # detached solution; without gradients there is nothing to attach
        wants = [t for t in (x_init, C, c, F, f) if isinstance(t, torch.Tensor) and t.requires_grad]
        if wants:
            raise NotImplementedError(
                "dilqr: mpc_explicit.MPC differentiates through the DiLQR implicit backward, which needs an "
                "env_dx model (cartpole, pendulum, rocket); use mpc.MPC (classic adjoint) for LinDx or "
                "generic dynamics, or solve under torch.no_grad()")
        return x.detach(), u.detach()
    th = dx.params if isinstance(dx.params, torch.Tensor) else torch.tensor(dx.params)
    # the no-op step's sweep (its gains feed the implicit backward) sees the
    # same mask / trust region as the loop's (mpc_explicit.py:369, 452)
    step = ExplicitStep(n, m, T, u_lower=mpc.u_lower, u_upper=mpc.u_upper, u_zero_I=getattr(mpc, "u_zero_I", None),
                        delta_u=mpc.delta_u, true_cost=QuadCost(C, c), true_dynamics=dx, current_x=x.detach(),
                        current_u=u.detach(), back_eps=mpc.back_eps, no_op_forward=True)
    return step(x_init, C, c, F, f, th)
