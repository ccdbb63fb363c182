"""CPU checks of the fused MPC path on the one-hidden-layer network: the two
entry points (dilqr_mlp_ilqr_iterate_f32, dilqr_mlp_mpc_solve_small_f32) are
declared, exported and bound; their argument validation returns codes before
any launch (so this runs without a GPU); ops.mlp_solve_route picks the route."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")
NEW = ("dilqr_mlp_ilqr_iterate_f32", "dilqr_mlp_mpc_solve_small_f32")
P = ctypes.c_void_p(16)          # a non-null, 16-byte aligned address (never dereferenced: no launch)


def test_symbols_declared_exported_bound():
    from dilqr import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in N.SIGNATURES
    assert lib.dilqr_version() == 11


def mlp(H=8, act=0, ptr=P):
    from dilqr import _native as N
    return N.Mlp(H, act, 1, ptr.value, ptr.value, ptr.value, ptr.value)


def iterate(n=5, m=1, T=4, B=8, desc=None, x_init=P, C=P, ws=P, x_out=P, old_cost=None, ctrl=None, max_ls=2):
    from dilqr import _native as N
    nb = N.Bounds(N.BOUNDS_NONE, 0.0, 0.0, None, None)
    return N.lib().dilqr_mlp_ilqr_iterate_f32(n, m, T, B, desc or mlp(), x_init, C, P, P, P, nb, 0.5, max_ls, ws,
                                              x_out, P, P, P, P, old_cost, ctrl, None)


def small(n=5, m=1, T=4, B=8, desc=None, x_init=P, u_init=None, C=P, xa=P, best_x=P, ctrl=P, iters=3, max_ls=2):
    from dilqr import _native as N
    nb = N.Bounds(N.BOUNDS_NONE, 0.0, 0.0, None, None)
    return N.lib().dilqr_mlp_mpc_solve_small_f32(n, m, T, B, desc or mlp(), x_init, u_init, C, P, nb, 0.5, max_ls,
                                                 iters, 1e-4, 1e-7, 5, xa, P, P, P, P, P, P, P, P, best_x, P, P, P,
                                                 ctrl, None)


@pytest.mark.parametrize("call", [iterate, small], ids=["iterate", "small"])
def test_argument_validation_without_launch(call):
    assert call(x_init=None) == 2 and call(C=None) == 2                  # null pointers
    assert call(x_init=ctypes.c_void_p(20)) == 2                         # a misaligned pointer
    assert call(desc=mlp(ptr=ctypes.c_void_p(0))) == 2                   # null weights
    assert call(desc=mlp(ptr=ctypes.c_void_p(8))) == 2                   # misaligned weights
    assert call(T=0) == 2 and call(B=-1) == 2 and call(max_ls=0) == 2    # bad sizes
    assert call(n=7, m=1) == 1                                           # no kernels for (7, 1)
    assert call(desc=mlp(H=0)) == 1 and call(desc=mlp(H=257)) == 1       # H outside [1, 256]
    assert call(desc=mlp(act=2)) == 3                                    # unknown activation
    assert call(B=0) == 0                                                # nothing to do, nothing launched


def test_argument_validation_of_each_call():
    assert iterate(ws=None) == 2 and iterate(x_out=ctypes.c_void_p(4)) == 2
    assert small(B=257) == 1                                             # above one workgroup
    assert small(B=257, n=7) == 1
    assert small(n=6, m=2) == 1 and small(n=6, m=2, B=0) == 1            # (6, 2): the per-iteration kernel only
    assert iterate(n=6, m=2, B=0) == 0
    assert small(ctrl=None) == 2 and small(xa=None) == 2 and small(best_x=ctypes.c_void_p(24)) == 2
    assert small(u_init=ctypes.c_void_p(4)) == 2                         # u_init is nullable, not misalignable
    assert small(iters=0) == 2
    assert small(B=0, u_init=None) == 0


def models():
    from dilqr import ops
    n, m, H = 5, 1, 8
    one = ops.MlpModel(n, m, 0, True, torch.zeros(H, n + m), torch.zeros(H), torch.zeros(n, H), torch.zeros(n))
    two = ops.Mlp2Model(n, m, 0, True, torch.zeros(H, n + m), torch.zeros(H), torch.zeros(H, H), torch.zeros(H),
                        torch.zeros(n, H), torch.zeros(n))
    return one, two


def test_route(monkeypatch):
    from dilqr import _native as N
    from dilqr import ops
    one, two = models()
    dyn = ops.Dynamics(one, 5, 1)
    assert ops.MLP_FUSED is True and ops.SMALL_BATCH_MAX == 256
    # as shipped: the one-launch solve did not win its measurement, so the fused
    # iteration per launch is taken at every batch, with no upper threshold (it won at 65 536 too)
    assert ops.MLP_SMALL_MAX_BATCH == 0 and ops.MLP_FUSED_MAX_BATCH is None
    for d in (dyn, one):
        for B in (1, 256, 257, 65536):
            assert ops.mlp_solve_route(d, B, 10, None, 0) == "fused"
    # with the one-launch solve switched on: up to one workgroup's batch
    monkeypatch.setattr(ops, "MLP_SMALL_MAX_BATCH", ops.SMALL_BATCH_MAX)
    for d in (dyn, one):
        assert ops.mlp_solve_route(d, 1, 10, None, 0) == "small"
        assert ops.mlp_solve_route(d, 256, 10, None, 0) == "small"
        assert ops.mlp_solve_route(d, 256, 1, None, -1) == "small"
        assert ops.mlp_solve_route(d, 257, 10, None, 0) == "fused"
    monkeypatch.setattr(ops, "MLP_FUSED_MAX_BATCH", 4096)                # a threshold, had one been needed
    assert ops.mlp_solve_route(dyn, 4096, 10, None, 0) == "fused"
    assert ops.mlp_solve_route(dyn, 4097, 10, None, 0) == "unfused"
    monkeypatch.setattr(ops, "MLP_FUSED_MAX_BATCH", None)
    for B in (8, 257):
        assert ops.mlp_solve_route(ops.Dynamics(two, 5, 1), B, 10, None, 0) == "unfused"
        assert ops.mlp_solve_route(dyn, B, 10, torch.zeros(4, B, 1, dtype=torch.bool), 0) == "unfused"
        assert ops.mlp_solve_route(dyn, B, 10, None, 1) == "unfused"
        assert ops.mlp_solve_route(ops.Dynamics(N.MODEL_CARTPOLE, 5, 1), B, 10, None, 0) == "unfused"
    assert ops.mlp_solve_route(dyn, 8, 0, None, 0) == "unfused"
    # (6, 2) has no one-launch solve (its iteration leaves the loop no registers): per iteration at every B
    wide = ops.MlpModel(6, 2, 0, True, torch.zeros(8, 8), torch.zeros(8), torch.zeros(6, 8), torch.zeros(6))
    assert (6, 2) not in N.MLP_SMALL_SHAPES and (5, 1) in N.MLP_SMALL_SHAPES
    assert ops.mlp_solve_route(wide, 8, 10, None, 0) == "fused"
    monkeypatch.setattr(ops, "MLP_FUSED", False)
    for B in (1, 256, 257):
        assert ops.mlp_solve_route(dyn, B, 10, None, 0) == "unfused"
