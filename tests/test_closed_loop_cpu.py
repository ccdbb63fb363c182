"""CPU checks of the closed-loop episode (dilqr.closed_loop, csrc/tu_advance.hip):
the numpy episode the GPU tests lean on against the reference's fp64 golden,
the new entry point across header, library and binding, its argument checks
(nothing is launched), the warm-start index rule as a host program, and
mpc_episode's refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import closed_loop_oracle as clo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dilqr.h")


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|const char\s*\*)\s+(dilqr_\w+)\s*\(", src)))
SRC = os.path.join(ROOT, "tests", "host", "advance_host.cpp")
CSRC = os.path.join(ROOT, "differentiable-ilqr_amd", "csrc")
CASES = ("pend", "cart", "pend_b1", "pend_mismatch", "pend_t3", "complex", "rocket")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


# ---------------------------------------------------------------- golden / oracle
def test_golden_holds_the_cases_and_their_spread(golden):
    g64, g32 = golden("closed_loop_f64"), golden("closed_loop_f32")
    assert tuple(g64["cases"]) == CASES == tuple(g32["cases"])
    for name in CASES:
        T, steps = (int(v) for v in g64[f"{name}_settings"][:2])
        B, n = g64[f"{name}_x0"].shape
        assert g64[f"{name}_x"].shape == (steps + 1, B, n) and g64[f"{name}_u"].shape[:2] == (steps, B)
        assert g64[f"{name}_plan_costs"].shape == (steps, B)
        assert np.array_equal(g64[f"{name}_x"][0], g64[f"{name}_x0"])
        # the generator's condition: the reference's own fp32-vs-fp64 spread
        assert float(g32[f"{name}_spread_x"]) < 1e-4 and float(g32[f"{name}_spread_u"]) < 1e-4
        assert rel(g32[f"{name}_x"], g64[f"{name}_x"]) == pytest.approx(float(g32[f"{name}_spread_x"]))


@pytest.mark.parametrize("name", CASES)
def test_oracle_episode_f64(golden, name):
    """The numpy episode reproduces the reference's fp64 episode at the
    tolerance test_oracle_golden.py holds its MPC solves to."""
    g = golden("closed_loop_f64")
    model, x0, C, c, T, steps, kw = clo.golden_case(g, name)
    x, u, stage, plan_costs = clo.episode(model, x0, C, c, T, steps, **kw)
    assert rel(x, g[f"{name}_x"]) < 1e-8
    assert rel(u, g[f"{name}_u"]) < 1e-8
    assert rel(plan_costs, g[f"{name}_plan_costs"]) < 1e-8
    assert stage.shape == plan_costs.shape


def test_oracle_warm_rules():
    u = np.arange(9, dtype=np.float64).reshape(9, 1, 1) + 1.0       # row t holds t + 1
    flat = lambda w: [int(v) for v in w[:, 0, 0]]                   # noqa: E731
    assert flat(clo.warm_start(u, "reference")) == [2, 3, 4, 5, 6, 7, 8, 8, 0]
    assert flat(clo.warm_start(u, "shift")) == [2, 3, 4, 5, 6, 7, 8, 9, 0]
    assert flat(clo.warm_start(u, "cold")) == [0] * 9
    assert flat(clo.warm_start(u[:3], "reference")) == [2, 2, 0]
    with pytest.raises(IndexError):
        clo.warm_start(u[:2], "reference")


# ---------------------------------------------------------------- header / ABI
def test_entry_point_declared_exported_and_bound():
    from dilqr import _native
    assert "dilqr_mpc_advance_f32" in header_functions()
    assert hasattr(_native.lib(), "dilqr_mpc_advance_f32")
    args, res = _native.SIGNATURES["dilqr_mpc_advance_f32"]
    assert len(args) == 14 and res is ctypes.c_int
    src = open(os.path.join(ROOT, "include", "dilqr.h")).read()
    for name, value in (("REFERENCE", _native.WARM_REFERENCE), ("SHIFT", _native.WARM_SHIFT),
                        ("COLD", _native.WARM_COLD)):
        assert f"#define DILQR_WARM_{name} {value}" in src
    assert "il_env.py:134-140" in src


def test_advance_rejects_bad_arguments_without_launch():
    from dilqr import _native as N
    adv = N.lib().dilqr_mpc_advance_f32
    p = ctypes.c_void_p
    ok = dict(model=N.MODEL_PENDULUM, T=5, B=4, theta=p(16), u_plan=p(4096), x_cur=p(8192), u_warm=p(12288),
              mode=N.WARM_REFERENCE, C=None, c=None, x_log=p(16388), u_log=p(20484), cost_log=None)

    def rc(**kw):
        a = dict(ok, **kw)
        return adv(a["model"], a["T"], a["B"], a["theta"], a["u_plan"], a["x_cur"], a["u_warm"], a["mode"], a["C"],
                   a["c"], a["x_log"], a["u_log"], a["cost_log"], None)

    assert rc(B=0) == 0                                       # nothing to do, nothing launched
    for null in ("theta", "u_plan", "x_cur", "u_warm", "x_log", "u_log"):
        assert rc(B=0, **{null: None}) == 2, null
    assert rc(B=0, cost_log=p(64)) == 2                       # a cost log without the cost
    assert rc(B=0, cost_log=p(64), C=p(32), c=None) == 2
    assert rc(B=0, cost_log=p(64), C=p(32), c=p(48)) == 0
    assert rc(B=0, mode=3) == 2 and rc(B=0, mode=-1) == 2     # unknown warm mode
    assert rc(B=0, T=2) == 2                                  # the reference's rule needs T >= 3
    assert rc(B=0, T=2, mode=N.WARM_SHIFT) == 0 and rc(B=0, T=1, mode=N.WARM_COLD) == 0
    assert rc(B=0, T=0, mode=N.WARM_COLD) == 2 and rc(B=-1) == 2
    for name in ("u_plan", "x_cur", "u_warm"):                # 16-byte alignment of the buffers
        assert rc(B=0, **{name: p(4100)}) == 2, name
    assert rc(B=0, C=p(36), c=p(48)) == 2
    assert rc(B=0, x_log=p(16390)) == 2 and rc(B=0, u_log=p(20482)) == 2      # 4 bytes for the log rows
    assert rc(u_warm=p(4096)) == 2                            # u_warm is u_plan
    assert rc(u_warm=p(4096 + 16)) == 2                       # ... or overlaps it (T*B*m floats = 80 bytes)
    assert rc(u_plan=p(12288 + 64)) == 2
    for model in (N.MODEL_LINDX, N.MODEL_MLP, 42):            # no forward
        assert rc(B=0, model=model) == 1, model


# ---------------------------------------------------------------- the index rule on the host
def test_warm_start_rule_on_host(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ not found"
    exe = str(tmp_path / "advance_host")
    base = [gxx, "-std=c++17", "-O1", "-g", "-I", CSRC, SRC, "-o", exe]
    # the sanitizer runtimes linked into the program itself (as test_stop_rule_host.py)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(base + san, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert run.stdout.startswith("ok:"), run.stdout


# ---------------------------------------------------------------- python layer
def test_il_env_pendulum_complex_constructs():
    from dilqr import _native as N
    from dilqr.il import IL_Env, ILTrainer
    env = IL_Env("pendulum-complex", lqr_iter=10, mpc_T=6, device="cpu")
    assert env.true_dx.model_id == N.MODEL_PENDULUM_COMPLEX
    assert [float(v) for v in env.true_dx.params] == pytest.approx([10., 1., 1., 1.0, 0.1])
    assert tuple(env.sample_xinit(4).shape) == (4, 3)
    with pytest.raises(NotImplementedError):
        ILTrainer(env, mode="sysid")
    with pytest.raises(NotImplementedError):
        IL_Env("acrobot")


def test_mpc_episode_refusals():
    """Every refusal names its reason and is raised before the device is touched
    (CPU tensors here: nothing could be launched)."""
    import torch
    import dilqr
    from dilqr import mpc as classic
    from dilqr.closed_loop import mpc_episode
    from dilqr.dynamics import AffineDynamics, NNDynamics
    from dilqr.env_dx.cartpole import CartpoleDx
    from dilqr.env_dx.pendulum import PendulumDx
    dx = PendulumDx()
    q, p = dx.get_true_obj()
    cost = dilqr.QuadCost(torch.diag(q), p)
    x0 = torch.zeros(2, 3)
    kw = dict(lqr_iter=3, exit_unconverged=False, detach_unconverged=False)

    def refused(match, mpc, cost_=cost, dx_=dx, steps=2, **ekw):
        with pytest.raises(NotImplementedError, match=match):
            mpc_episode(mpc, x0, cost_, dx_, steps, **ekw)

    refused("non-quadratic", dilqr.MPC(3, 1, 5, **kw), cost_=torch.nn.Identity())
    refused("slew_rate_penalty", dilqr.MPC(3, 1, 5, slew_rate_penalty=0.1, **kw))
    refused("delta_u", dilqr.MPC(3, 1, 5, u_lower=-1.0, u_upper=1.0, delta_u=0.1, **kw))
    refused("verbose", dilqr.MPC(3, 1, 5, verbose=1, **kw))
    refused("u_zero_I", dilqr.MPC(3, 1, 5, u_zero_I=torch.zeros(5, 2, 1, dtype=torch.bool), **kw))
    refused("grad_method", dilqr.MPC(3, 1, 5, grad_method=dilqr.GradMethods.FINITE_DIFF, **kw))
    refused("T >= 3", dilqr.MPC(3, 1, 2, **kw))
    lin = dilqr.LinDx(torch.zeros(4, 2, 3, 4))
    refused("LinDx", classic.MPC(3, 1, 5, **kw), dx_=lin)
    refused("LinDx", dilqr.MPC(3, 1, 5, **kw), plant=lin)
    # a plant that is not an env_dx model: a network, or a network planner without a plant
    net = NNDynamics(3, 1, hidden_sizes=(8,))
    refused("plant", dilqr.MPC(3, 1, 5, **kw), plant=net)
    refused("plant", dilqr.MPC(3, 1, 5, **kw), dx_=net)
    refused("plant", dilqr.MPC(3, 1, 5, **kw), plant=AffineDynamics(torch.eye(3), torch.zeros(3, 1)))
    with pytest.raises(ValueError, match="same env_dx model"):
        mpc_episode(dilqr.MPC(3, 1, 5, **kw), x0, cost, dx, 2, plant=PendulumDx(simple=False))
    with pytest.raises(ValueError, match="plant is"):
        mpc_episode(dilqr.MPC(3, 1, 5, **kw), x0, cost, dx, 2, plant=CartpoleDx())
    with pytest.raises(ValueError, match="warm_start"):
        mpc_episode(dilqr.MPC(3, 1, 5, **kw), x0, cost, dx, 2, warm_start="hot")
    with pytest.raises(ValueError, match="steps"):
        mpc_episode(dilqr.MPC(3, 1, 5, **kw), x0, cost, dx, 0)
    # T = 2 is fine without the quirk; what is left is the missing GPU
    for warm in ("shift", "cold"):
        with pytest.raises(RuntimeError, match="GPU"):
            mpc_episode(dilqr.MPC(3, 1, 2, **kw), x0, cost, dx, 2, warm_start=warm)
    # a network planner against an env_dx plant needs its device model
    with pytest.raises(RuntimeError, match="GPU"):
        mpc_episode(dilqr.MPC(3, 1, 5, **kw), x0, cost, net, 2, plant=dx)


def test_mpc_advance_checks_shapes_before_the_library():
    import torch
    from dilqr import _native as N
    from dilqr import ops
    T, B, n, m = 4, 3, 3, 1
    z = torch.zeros
    good = dict(u_plan=z(T, B, m), x_cur=z(B, n), u_warm=z(T, B, m), x_next_log=z(B, n), u_log=z(B, m))

    def call(**kw):
        a = dict(good, **kw)
        ops.mpc_advance(N.MODEL_PENDULUM, z(3), a["u_plan"], a["x_cur"], a["u_warm"], "shift", a["x_next_log"],
                        a["u_log"], a.get("C"), a.get("c"), a.get("cost_log"))

    for name, bad in (("u_warm", z(T - 1, B, m)), ("x_next_log", z(B + 1, n)), ("u_log", z(B, m + 1)),
                      ("cost_log", z(B + 1)), ("C", z(T, B, 4, 3)), ("c", z(T, B, 5))):
        with pytest.raises(ValueError, match=name):
            call(**{name: bad})
    with pytest.raises(ValueError, match="model"):
        call(x_cur=z(B, 5), x_next_log=z(B, 5))
    with pytest.raises(RuntimeError, match="not on the GPU"):     # shapes fine: refused at the pointers
        call()
