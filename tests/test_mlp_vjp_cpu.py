"""CPU checks around the device VJP of the MLP linearisation
(csrc/tu_mlp_vjp.hip): the ABI-11 symbols, dilqr_mlp_linearize_vjp_f32's
argument validation (errors return before any launch, so no GPU is needed),
the workspace size, and which linearisation generic.linearize(diff=True)
takes."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")
E_SHAPE, E_ARG, E_MODE = 1, 2, 3


def test_abi_11_symbols():
    from dilqr import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+dilqr_mlp_linearize_vjp_ws_bytes\s*\(", src)
    assert re.search(r"\bint\s+dilqr_mlp_linearize_vjp_f32\s*\(", src)
    lib = N.lib()
    assert hasattr(lib, "dilqr_mlp_linearize_vjp_ws_bytes") and hasattr(lib, "dilqr_mlp_linearize_vjp_f32")
    assert lib.dilqr_version() == 11 == N.ABI_VERSION
    assert "dilqr_mlp_linearize_vjp_f32" in N.SIGNATURES


def slab(n, m, H):
    return H * (n + m + 1) + n * H + n


def vjp(N, n=5, m=1, T=4, B=65, H=32, act=0, W1=16, x=16, gF=16, gf=16, dW1=16, db1=16, dW2=16, db2=16, max_waves=0,
        ws=16, short=0):
    """The call with fake (never dereferenced) pointers and an exactly sized workspace, less `short` bytes."""
    P = ctypes.c_void_p
    G = max(1, min((max(T - 1, 0) * B + 63) // 64, max_waves if max_waves > 0 else 512))
    nbytes = 4 * G * slab(n, m, max(H, 1))
    return N.lib().dilqr_mlp_linearize_vjp_f32(n, m, T, B, N.Mlp(H, act, 1, W1, 16, 16, 16), P(x), P(16), P(gF), P(gf),
                                               P(dW1), P(db1), P(dW2), P(db2), max_waves, P(ws), nbytes - short, None)


def test_vjp_rejects_bad_arguments_without_launch():
    from dilqr import _native as N
    for kw in ({"dW1": None}, {"db1": None}, {"dW2": None}, {"db2": None}, {"dW1": 4}, {"db1": 8}, {"dW2": 20},
               {"db2": 12}, {"x": None}, {"x": 4}, {"gF": 4}, {"gf": 8}, {"W1": None}, {"W1": 4}, {"ws": None},
               {"ws": 8}, {"short": 1}, {"max_waves": -1}, {"T": 0}, {"B": -1}):
        assert vjp(N, **kw) == E_ARG, kw
    for kw in ({"n": 7, "m": 3}, {"n": 13, "m": 3}, {"H": 0}, {"H": N.MLP_MAX_HIDDEN + 1}):
        assert vjp(N, **kw) == E_SHAPE, kw
    for kw in ({"act": 2}, {"act": -1}):
        assert vjp(N, **kw) == E_MODE, kw
    # no rows: valid, nothing launched
    assert vjp(N, T=1) == 0
    assert vjp(N, B=0) == 0
    assert vjp(N, T=1, gF=None, gf=None) == 0


def test_ws_bytes():
    """4 G P bytes, G = min(ceil(rows / 64), cap) (at least 1), cap = max_waves
    or 512, P = H (n + m + 1) + n H + n; never smaller for more rows."""
    from dilqr import _native as N
    size = N.lib().dilqr_mlp_linearize_vjp_ws_bytes
    for n, m, T, B, H, mw, G in ((5, 1, 3, 65, 33, 0, 3), (5, 1, 5, 50, 33, 1, 1), (5, 1, 5, 50, 33, 2, 2),
                                 (5, 1, 5, 50, 33, 9, 4), (4, 2, 25, 65536, 100, 0, 512), (6, 2, 2, 65, 256, 0, 2),
                                 (2, 1, 2, 1, 1, 0, 1), (5, 1, 1, 8, 32, 0, 1), (5, 1, 4, 0, 32, 0, 1)):
        assert size(n, m, T, B, H, mw) == 4 * G * slab(n, m, H), (n, m, T, B, H, mw)
    assert size(5, 1, 4, 8, 32, -1) == 0 and size(5, 1, 0, 8, 32, 0) == 0 and size(5, 1, 4, 8, 0, 0) == 0
    for mw in (0, 1, 7):
        sizes = [size(5, 1, 2, B, 100, mw) for B in (0, 1, 63, 64, 65, 200, 448, 449, 10 ** 5, 10 ** 7)]
        assert sizes == sorted(sizes) and sizes[0] > 0, mw


class _Taken(Exception):
    pass


def test_linearize_diff_routing(monkeypatch):
    """generic.linearize(diff=True) reaches ops.mlp_linearize_diff, with the
    module's own parameters, for a one-hidden-layer sigmoid or relu module on
    GPU fp32 tensors (`is_cuda` faked: the routing reads nothing else of the
    device), and the torch graph through the module for everything else."""
    from dilqr import generic, ops
    from dilqr.dynamics import NNDynamics
    from dilqr.mpc_explicit import GradMethods

    class FakeCuda(torch.Tensor):
        is_cuda = True

    def device(mlp, params, x, u):
        assert isinstance(mlp, ops.MlpModel) and len(params) == 4
        device.params = params
        raise _Taken("device")

    def torch_graph(self, x, u):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "mlp_linearize_diff", device)
    # the torch graph evaluates the module (forward, then grad_input with
    # ANALYTIC; forward alone with AUTO_DIFF / FINITE_DIFF): both are the marker
    monkeypatch.setattr(NNDynamics, "grad_input", torch_graph)
    monkeypatch.setattr(NNDynamics, "forward", torch_graph)

    def route(dx, gm=GradMethods.ANALYTIC, diff=True):
        dt = next(dx.parameters()).dtype
        x = torch.zeros(4, 3, 5, dtype=dt).as_subclass(FakeCuda)
        u = torch.zeros(4, 3, 1, dtype=dt).as_subclass(FakeCuda)
        with pytest.raises(_Taken) as e:
            generic.linearize(types.SimpleNamespace(grad_method=gm), x, u, dx, diff)
        return str(e.value)

    assert generic.DEVICE_MLP is True and generic.DEVICE_MLP_VJP is True
    for dx in (NNDynamics(5, 1, hidden_sizes=[32]),
               NNDynamics(5, 1, hidden_sizes=[100], activation="relu", passthrough=False)):
        assert route(dx) == "device"
        assert all(a is b for a, b in zip(device.params, (dx.fcs[0].weight, dx.fcs[0].bias, dx.fcs[1].weight,
                                                          dx.fcs[1].bias)))
    dx = NNDynamics(5, 1, hidden_sizes=[32])
    assert route(NNDynamics(5, 1, hidden_sizes=[8, 8])) == "torch"
    assert route(NNDynamics(5, 1, hidden_sizes=[32], activation="elu")) == "torch"
    assert route(NNDynamics(5, 1, hidden_sizes=[32]).double()) == "torch"
    assert route(dx, GradMethods.AUTO_DIFF) == "torch"
    assert route(dx, GradMethods.FINITE_DIFF) == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP_VJP", False)
    assert route(dx) == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP_VJP", True)
    monkeypatch.setattr(generic, "DEVICE_MLP", False)
    assert route(dx) == "torch"
    monkeypatch.setattr(generic, "DEVICE_MLP", True)
    # CPU tensors keep the torch graph
    with pytest.raises(_Taken, match="torch"):
        generic.linearize(types.SimpleNamespace(grad_method=GradMethods.ANALYTIC), torch.zeros(4, 3, 5),
                          torch.zeros(4, 3, 1), dx, True)
