"""CPU checks around the device VJP of the two-hidden-layer MLP linearisation
(csrc/tu_mlp2_vjp.hip): the additive symbols, dilqr_mlp2_linearize_vjp_f32's
argument validation (errors return before any launch, so no GPU is needed),
the workspace size, and which linearisation generic.linearize(diff=True) takes
under DEVICE_MLP_DEEP_VJP, which ships off."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")
E_SHAPE, E_ARG, E_MODE = 1, 2, 3


def test_abi_symbols():
    from dilqr import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+dilqr_mlp2_linearize_vjp_ws_bytes\s*\(", src)
    assert re.search(r"\bint\s+dilqr_mlp2_linearize_vjp_f32\s*\(", src)
    cap = int(re.search(r"#define\s+DILQR_MLP2_VJP_MAX_HIDDEN1\s+(\d+)", src).group(1))
    assert cap == N.MLP2_VJP_MAX_HIDDEN1 and 64 <= cap <= N.MLP_MAX_HIDDEN
    lib = N.lib()
    assert hasattr(lib, "dilqr_mlp2_linearize_vjp_ws_bytes") and hasattr(lib, "dilqr_mlp2_linearize_vjp_f32")
    assert lib.dilqr_version() == 11 == N.ABI_VERSION
    assert "dilqr_mlp2_linearize_vjp_f32" in N.SIGNATURES
    assert "dilqr_mlp2_linearize_vjp_ws_bytes" in N.SIZE_SIGNATURES
    # the one-layer call's arguments with the descriptor exchanged, two more outputs and one more width
    args, res = N.SIGNATURES["dilqr_mlp2_linearize_vjp_f32"]
    args1, res1 = N.SIGNATURES["dilqr_mlp_linearize_vjp_f32"]
    assert res is res1 and [N.Mlp if a is N.Mlp2 else a for a in args] == args1[:13] + [ctypes.c_void_p] * 2 + args1[13:]
    assert len(N.SIZE_SIGNATURES["dilqr_mlp2_linearize_vjp_ws_bytes"][0]) == 7


def ws_floats(n, m, rows, H1, H2, max_waves=0):
    """The header's formula."""
    C = n + m + 1
    LB = 4 if n * (n + m) <= 30 else 2
    NB = (H2 + LB - 1) // LB
    P = n * H2 + H2 + H2 * C * H1 + NB * H1 * C + n
    chunks = (rows + 63) // 64
    G = max(1, min(chunks, max_waves if max_waves > 0 else min(512, max(1, 2 ** 24 // P))))
    return (G + 1) * P


def vjp(N, n=5, m=1, T=4, B=65, H1=32, H2=16, act=0, W=None, x=16, gF=16, gf=16, out=None, max_waves=0, ws=16,
        short=0):
    """The call with fake (never dereferenced) pointers and an exactly sized
    workspace, less `short` bytes.  W: {weight name: pointer}, out: {output
    name: pointer}; everything else is 16."""
    P = ctypes.c_void_p
    w = dict(W1=16, b1=16, W2=16, b2=16, W3=16, b3=16)
    w.update(W or {})
    o = dict(dW1=16, db1=16, dW2=16, db2=16, dW3=16, db3=16)
    o.update(out or {})
    nbytes = 4 * ws_floats(n, m, max(T - 1, 0) * max(B, 0), max(H1, 1), max(H2, 1), max(max_waves, 0))
    desc = N.Mlp2(H1, H2, act, 1, *(w[k] for k in ("W1", "b1", "W2", "b2", "W3", "b3")))
    return N.lib().dilqr_mlp2_linearize_vjp_f32(
        n, m, T, B, desc, P(x), P(16), P(gF), P(gf), *(P(o[k]) for k in ("dW1", "db1", "dW2", "db2", "dW3", "db3")),
        max_waves, P(ws), nbytes - short, None)


def test_vjp_rejects_bad_arguments_without_launch():
    from dilqr import _native as N
    assert vjp(N, T=1) == 0                        # the baseline call is valid (no rows: nothing launched)
    for name in ("dW1", "db1", "dW2", "db2", "dW3", "db3"):
        for bad in (None, 4, 8, 20):
            assert vjp(N, out={name: bad}) == E_ARG, (name, bad)
    for name in ("W1", "b1", "W2", "b2", "W3", "b3"):
        for bad in (None, 4):
            assert vjp(N, W={name: bad}) == E_ARG, (name, bad)
    for kw in ({"x": None}, {"x": 4}, {"gF": 4}, {"gf": 8}, {"ws": None}, {"ws": 8}, {"short": 1},
               {"max_waves": -1}, {"T": 0}, {"B": -1}):
        assert vjp(N, **kw) == E_ARG, kw
    for kw in ({"n": 7, "m": 3}, {"n": 13, "m": 3}, {"H1": 0}, {"H2": 0}, {"H1": N.MLP_MAX_HIDDEN + 1},
               {"H2": N.MLP_MAX_HIDDEN + 1}, {"H1": N.MLP2_VJP_MAX_HIDDEN1 + 1}):
        assert vjp(N, **kw) == E_SHAPE, kw
    for kw in ({"act": 2}, {"act": -1}):
        assert vjp(N, **kw) == E_MODE, kw
    # both widths at their limits are inside the envelope: only the alignment is left to refuse
    assert vjp(N, H1=N.MLP2_VJP_MAX_HIDDEN1, H2=N.MLP_MAX_HIDDEN, T=1) == 0
    assert vjp(N, H1=N.MLP2_VJP_MAX_HIDDEN1, H2=N.MLP_MAX_HIDDEN, x=4) == E_ARG
    # no rows: valid, nothing launched
    assert vjp(N, B=0) == 0
    assert vjp(N, T=1, gF=None, gf=None) == 0


def test_ws_bytes():
    """4 (G + 1) P bytes with P = n H2 + H2 + H2 (n+m+1) H1 + NB H1 (n+m+1) + n,
    NB = ceil(H2 / LB), LB = 4 (2 where n (n+m) > 30), G = min(chunks, max_waves
    or min(512, 2^24 // P)), at least 1: the numbers below are worked out by hand
    from that; never smaller for more rows."""
    from dilqr import _native as N
    size = N.lib().dilqr_mlp2_linearize_vjp_ws_bytes
    table = (
        # n, m, T, B, H1, H2, max_waves, bytes
        (5, 1, 3, 65, 33, 7, 0, 4 * 4 * 2126),                  # P = 35 + 7 + 1617 + 2*231 + 5; 3 chunks: 34016
        (5, 1, 1, 8, 32, 16, 0, 4 * 2 * 4581),                  # P = 80 + 16 + 3584 + 4*224 + 5; no rows: one slab
        (5, 1, 4, 0, 32, 16, 0, 4 * 2 * 4581),
        (5, 1, 5, 50, 33, 7, 1, 4 * 2 * 2126),                  # 4 chunks, capped
        (5, 1, 5, 50, 33, 7, 2, 4 * 3 * 2126),
        (5, 1, 5, 50, 33, 7, 9, 4 * 5 * 2126),
        (4, 2, 25, 65536, 64, 64, 0, 4 * 464 * 36164),          # P = 256 + 64 + 28672 + 16*448 + 4; the budget caps
                                                                # G at 2^24 // P = 463: 67120384
        (6, 2, 2, 10 ** 6, 64, 256, 0, 4 * 76 * 222982),        # LB = 2: P = 1536 + 256 + 147456 + 128*576 + 6;
                                                                # the budget caps G at 2^24 // P = 75: 67786528
        (2, 1, 2, 1, 1, 1, 0, 4 * 2 * (2 + 1 + 4 + 4 + 2)),
    )
    assert table[0][-1] == 34016 and table[6][-1] == 67120384 and table[7][-1] == 67786528
    for n, m, T, B, H1, H2, mw, nbytes in table:
        assert size(n, m, T, B, H1, H2, mw) == nbytes == 4 * ws_floats(n, m, max(T - 1, 0) * B, H1, H2, mw), \
            (n, m, T, B, H1, H2, mw)
    for bad in ((5, 1, 4, 8, 32, 16, -1), (5, 1, 0, 8, 32, 16, 0), (5, 1, 4, -1, 32, 16, 0), (5, 1, 4, 8, 0, 16, 0),
                (5, 1, 4, 8, 32, 0, 0), (5, 1, 4, 8, N.MLP2_VJP_MAX_HIDDEN1 + 1, 16, 0),
                (5, 1, 4, 8, 32, N.MLP_MAX_HIDDEN + 1, 0), (0, 1, 4, 8, 32, 16, 0)):
        assert size(*bad) == 0, bad
    for mw in (0, 1, 7):
        for H1, H2 in ((64, 64), (64, 256), (3, 5)):
            sizes = [size(5, 1, 2, B, H1, H2, mw) for B in (0, 1, 63, 64, 65, 200, 448, 449, 10 ** 5, 10 ** 7)]
            assert sizes == sorted(sizes) and sizes[0] > 0, (mw, H1, H2)


def test_model_vjp_ok_and_call_type_checks():
    from dilqr import _native as N
    from dilqr import ops
    from dilqr.dynamics import NNDynamics
    like = torch.zeros(1)
    cap = N.MLP2_VJP_MAX_HIDDEN1
    inside = NNDynamics(5, 1, hidden_sizes=[cap, 8]).device_model(like, deep=True)
    assert inside.vjp_ok is True
    one = NNDynamics(5, 1, hidden_sizes=[8]).device_model(like)
    x, u = torch.zeros(4, 3, 5), torch.zeros(4, 3, 1)
    with pytest.raises(TypeError):
        ops.mlp2_linearize_vjp(one, x, u, None, None)
    with pytest.raises(ValueError):
        ops.mlp2_linearize_vjp(inside, torch.zeros(3, 5), torch.zeros(3, 1), None, None)
    with pytest.raises(ValueError):
        ops.mlp2_linearize_vjp(inside, x, u, torch.zeros(3, 3, 5, 5), None)
    with pytest.raises(ValueError):
        ops.mlp2_linearize_vjp(inside, x, u, None, None, max_waves=-1)
    if cap < N.MLP_MAX_HIDDEN:
        outside = NNDynamics(5, 1, hidden_sizes=[cap + 1, 8]).device_model(like, deep=True)
        assert outside.vjp_ok is False
        with pytest.raises(ValueError):
            ops.mlp2_linearize_vjp(outside, x, u, None, None)
    dx = NNDynamics(5, 1, hidden_sizes=[8, 8])
    md = dx.device_model(like, deep=True)
    with pytest.raises(ValueError, match="six parameters"):
        ops.mlp2_linearize_diff(md, [p for p in dx.parameters()][:4], x, u)
    with pytest.raises(ValueError, match="six parameters"):
        ops.mlp2_linearize_diff(md, [torch.zeros_like(p) for p in dx.parameters()], x, u)


class _Taken(Exception):
    pass


class FakeCuda(torch.Tensor):
    is_cuda = True


def test_linearize_diff_routing(monkeypatch):
    """generic.linearize(diff=True) reaches ops.mlp2_linearize_diff, with the
    module's own six parameters, for a two-hidden-layer sigmoid or relu module
    on GPU fp32 tensors (`is_cuda` faked: the routing reads nothing else of the
    device) only with DEVICE_MLP, DEVICE_MLP_DEEP, DEVICE_MLP_VJP and
    DEVICE_MLP_DEEP_VJP all on, and the torch graph for everything else."""
    from dilqr import _native as N
    from dilqr import generic, ops
    from dilqr.dynamics import NNDynamics
    from dilqr.mpc_explicit import GradMethods

    def device2(mlp, params, x, u):
        assert isinstance(mlp, ops.Mlp2Model) and mlp.vjp_ok and len(params) == 6
        device2.params = params
        raise _Taken("device2")

    def device1(mlp, params, x, u):
        assert isinstance(mlp, ops.MlpModel) and len(params) == 4
        raise _Taken("device1")

    def torch_graph(self, x, u):
        raise _Taken("torch")

    monkeypatch.setattr(ops, "mlp2_linearize_diff", device2)
    monkeypatch.setattr(ops, "mlp_linearize_diff", device1)
    monkeypatch.setattr(NNDynamics, "grad_input", torch_graph)
    monkeypatch.setattr(NNDynamics, "forward", torch_graph)

    def route(dx, gm=GradMethods.ANALYTIC, diff=True):
        dt = next(dx.parameters()).dtype
        x = torch.zeros(4, 3, 5, dtype=dt).as_subclass(FakeCuda)
        u = torch.zeros(4, 3, 1, dtype=dt).as_subclass(FakeCuda)
        with pytest.raises(_Taken) as e:
            generic.linearize(types.SimpleNamespace(grad_method=gm), x, u, dx, diff)
        return str(e.value)

    # the defaults
    assert generic.DEVICE_MLP_DEEP_VJP is False and generic.DEVICE_MLP_DEEP is False
    assert generic.DEVICE_MLP is True and generic.DEVICE_MLP_VJP is True
    two, one = NNDynamics(5, 1, hidden_sizes=[8, 8]), NNDynamics(5, 1, hidden_sizes=[32])
    switches = ("DEVICE_MLP", "DEVICE_MLP_DEEP", "DEVICE_MLP_VJP", "DEVICE_MLP_DEEP_VJP")
    assert route(two) == "torch" and route(one) == "device1"
    for s in switches:
        monkeypatch.setattr(generic, s, True)
    assert route(two) == "device2"
    assert len(device2.params) == 6 and all(a is b for a, b in zip(
        device2.params, (two.fcs[0].weight, two.fcs[0].bias, two.fcs[1].weight, two.fcs[1].bias, two.fcs[2].weight,
                         two.fcs[2].bias)))
    assert route(NNDynamics(5, 1, hidden_sizes=[N.MLP2_VJP_MAX_HIDDEN1, 7], activation="relu",
                            passthrough=False)) == "device2"
    assert route(one) == "device1"
    # any one switch off: the torch graph for two layers
    for s in switches:
        monkeypatch.setattr(generic, s, False)
        assert route(two) == "torch", s
        if s in ("DEVICE_MLP_DEEP", "DEVICE_MLP_DEEP_VJP"):
            assert route(one) == "device1", s
        monkeypatch.setattr(generic, s, True)
    # outside the envelope, or another grad method: the torch graph
    if N.MLP2_VJP_MAX_HIDDEN1 < N.MLP_MAX_HIDDEN:
        assert route(NNDynamics(5, 1, hidden_sizes=[N.MLP2_VJP_MAX_HIDDEN1 + 1, 8])) == "torch"
    assert route(NNDynamics(5, 1, hidden_sizes=[8, 8], activation="elu")) == "torch"
    assert route(NNDynamics(5, 1, hidden_sizes=[8, 8]).double()) == "torch"
    assert route(NNDynamics(5, 1, hidden_sizes=[8, 8, 8])) == "torch"
    assert route(two, GradMethods.AUTO_DIFF) == "torch"
    assert route(two, GradMethods.FINITE_DIFF) == "torch"
    # CPU tensors keep the torch graph
    with pytest.raises(_Taken, match="torch"):
        generic.linearize(types.SimpleNamespace(grad_method=GradMethods.ANALYTIC), torch.zeros(4, 3, 5),
                          torch.zeros(4, 3, 1), two, True)
