"""CPU checks of per-joint actuator usage (include/go1eval.h, sixth kernel family): the ctypes mirrors against the header, the
refusals without a GPU, the host-side definition against the reference's four per-joint reward terms, the model of
tests/joint_ref.py on hand-computable cases, go1eval.hip itself under the SIMT emulator against that model bit for bit (accumulators,
state, histogram and both result tables), the environment hooks where there is no GPU, and the sweep's host pieces."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import joint_ref as J
from test_response_trace import C_TYPES, HEADER, REPO, eval_emu, bits, enum_order, struct_fields
from test_terrain_metrics import scripted_groups

NAN = float("nan")
f32 = np.float32
ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]


# ---- 1. the mirrors against the header ---------------------------------------------------------------------------------------------
def test_joint_mirrors_match_the_header():
    import go1eval_host as G
    import go1sim_host as H
    src = open(HEADER).read()
    for macro, value in (("GO1EVAL_NUM_JOINT", G.NUM_JOINT), ("GO1JOINT_TAU_BINS", G.JOINT_TAU_BINS), ("GO1JOINT_VEL_BINS", G.JOINT_VEL_BINS)):
        assert f"#define {macro} {value}" in src
    assert (G.NUM_JOINT, G.JOINT_TAU_BINS, G.JOINT_VEL_BINS, G.NUM_DOF) == (10, 8, 8, 12) == (J.M, J.TAU_BINS, J.VEL_BINS, J.DOF)
    want = struct_fields(src, "Go1JointConfig")
    assert [f for f, _ in want] == [f for f, _ in G.Go1JointConfig._fields_] == [
        "num_envs", "warmup_steps", "num_groups", "dt", "soft_torque_limit", "soft_vel_limit", "torque_limit", "vel_limit", "pos_lower", "pos_upper"]
    for (field, ctext), (_, ctype) in zip(want, G.Go1JointConfig._fields_):
        if ctext.endswith("[12]"):
            assert ctext == "float[12]" and ctype._type_ is ctypes.c_float and ctype._length_ == 12, field
        else:
            assert ctype is C_TYPES[ctext], field
    assert ctypes.sizeof(G.Go1JointConfig) == 6 * 4 + 4 * 12 * 4
    want = struct_fields(src, "Go1JointBuffers")
    assert [f for f, _ in want] == [f for f, _ in G.Go1JointBuffers._fields_]
    assert all(ctext.endswith("*") for _, ctext in want) and all(t is ctypes.c_void_p for _, t in G.Go1JointBuffers._fields_)
    assert [f for f, _ in want] == J.INPUTS + ACCUMULATORS + J.STATE + ["group", "results", "hist_results"]
    types_ = dict(want)
    assert types_["hist"] == "uint32_t*" and types_["hist_results"] == "uint64_t*" and types_["prev_dof_vel"] == "float*" and types_["results"] == "double*"
    assert G._JOINT_INPUTS == J.INPUTS and G._JOINT_STATE == J.STATE
    assert enum_order(src, "Go1JointMetric", "GO1JOINT_") == G.JOINT_NAMES == J.METRICS and len(J.METRICS) == G.NUM_JOINT
    assert enum_order(src, "Go1JointGroupField", "GO1JOINT_G_") == G.JOINT_GROUP_FIELDS == J.GROUP_FIELDS
    assert G.DOF_NAMES == H.DOF_NAMES and len(G.DOF_NAMES) == 12 and G.DOF_NAMES[:4] == ["FL_hip_joint", "FL_thigh_joint", "FL_calf_joint", "FR_hip_joint"]
    assert H._DOF_VELOCITY == [50.0, 28.0, 28.0] * 4 and len(H._DOF_EFFORT) == 12
    assert set(G.EXPORTED_SYMBOLS) >= {"go1eval_joint_clear", "go1eval_joint_accumulate", "go1eval_joint_reduce"}
    from go1_gym_learn.eval_metrics import joints
    assert joints.JOINT_TERMS == G.JOINT_NAMES and joints.DOF_VELOCITY == H._DOF_VELOCITY


def test_existing_layouts_are_as_they_were():
    import go1eval_host as G
    assert [ctypes.sizeof(s) for s in (G.Go1EvalConfig, G.Go1BehaviourConfig, G.Go1TraceConfig, G.Go1PushConfig, G.Go1RecoveryConfig)] == [20, 28, 20, 8, 36]
    assert ctypes.sizeof(G.Go1ResponseConfig) == 11 * 4 + G.MAX_SIGNALS * 16 and ctypes.sizeof(G.Go1TerrainConfig) == 48
    assert ctypes.sizeof(G.Go1ResponseSignal) == 16
    assert [ctypes.sizeof(s) // 8 for s in (G.Go1EvalBuffers, G.Go1BehaviourBuffers, G.Go1TraceBuffers, G.Go1ResponseBuffers, G.Go1PushBuffers,
                                            G.Go1RecoveryBuffers, G.Go1TerrainBuffers)] == [22, 24, 13, 5, 3, 5, 23]


def test_the_library_exports_the_joint_symbols():
    import __graft_entry__ as g
    import go1eval_host as G
    g.build_eval_hip()
    lib = ctypes.CDLL(G.LIB_PATH)
    for name in G.EXPORTED_SYMBOLS:
        assert hasattr(lib, name), name


# ---- 2. the refusals without a GPU ---------------------------------------------------------------------------------------------------
def _joint_cfg(G, **over):
    c = G.Go1JointConfig()
    c.num_envs, c.warmup_steps, c.num_groups, c.dt, c.soft_torque_limit, c.soft_vel_limit = 8, 0, 1, 0.02, 1.0, 1.0
    for j in range(12):
        c.torque_limit[j], c.vel_limit[j], c.pos_lower[j], c.pos_upper[j] = 33.5, 28.0, -1.0, 1.0
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


def test_joint_arguments_are_checked_before_any_launch():
    import __graft_entry__ as g
    import go1eval_host as G
    g.build_eval_hip()
    lib = G.load_library()
    ref = ctypes.byref
    anything = np.zeros(12 * 64 * 8, np.float64)
    calls = (lib.go1eval_joint_clear, lib.go1eval_joint_accumulate, lib.go1eval_joint_reduce)
    buf = G.Go1JointBuffers()
    for fn in calls:
        assert fn(None, None, None) == -1
        assert fn(ref(_joint_cfg(G)), None, None) == -1
        assert fn(ref(_joint_cfg(G, num_envs=0)), ref(buf), None) == -1
        assert fn(ref(_joint_cfg(G)), ref(buf), None) == -2                       # no accumulators, no state
    for n in ACCUMULATORS + G._JOINT_STATE[:-1]:
        setattr(buf, n, anything.ctypes.data)
    for fn in calls:
        assert fn(ref(_joint_cfg(G)), ref(buf), None) == -2                       # the histogram is missing
    buf.hist = anything.ctypes.data
    assert lib.go1eval_joint_clear(ref(_joint_cfg(G)), ref(buf), None) == -3      # no dof_vel to take the previous velocity from
    assert lib.go1eval_joint_accumulate(ref(_joint_cfg(G)), ref(buf), None) == -3
    assert lib.go1eval_joint_reduce(ref(_joint_cfg(G)), ref(buf), None) == -5     # no group, no tables
    buf.group = buf.results = anything.ctypes.data
    assert lib.go1eval_joint_reduce(ref(_joint_cfg(G)), ref(buf), None) == -5     # no histogram table
    buf.hist_results = anything.ctypes.data
    assert lib.go1eval_joint_reduce(ref(_joint_cfg(G, num_groups=0)), ref(buf), None) == -5
    for n in G._JOINT_INPUTS[:-1]:
        setattr(buf, n, anything.ctypes.data)
    assert lib.go1eval_joint_accumulate(ref(_joint_cfg(G)), ref(buf), None) == -3      # episode_length_buf is missing
    buf.episode_length_buf = anything.ctypes.data
    refused = [dict(dt=0.0), dict(dt=-0.02), dict(dt=NAN), dict(dt=np.inf), dict(soft_torque_limit=0.0), dict(soft_torque_limit=NAN),
               dict(soft_vel_limit=-1.0), dict(soft_vel_limit=np.inf), dict(torque_limit=(0, 0.0)), dict(torque_limit=(11, NAN)), dict(torque_limit=(5, -33.5)),
               dict(vel_limit=(3, 0.0)), dict(vel_limit=(11, np.inf)), dict(pos_lower=(7, 1.5)), dict(pos_upper=(0, -1.25)), dict(pos_lower=(2, NAN)),
               dict(pos_upper=(11, NAN))]
    for over in refused:
        assert lib.go1eval_joint_accumulate(ref(_joint_cfg(G, **over)), ref(buf), None) == -12, over
    assert not anything.any()


# ---- 3. the host-side definition against the reference's reward terms -----------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_joint_terms_sum_to_the_reference_rewards(seed):
    from go1_gym_learn.eval_metrics import joints
    z = np.load(os.path.join(REPO, "tests", "golden", "joint_metrics.npz"))
    x = {k: torch.from_numpy(z[f"s{seed}_in_{k}"]) for k in ("torques", "dof_vel", "last_dof_vel", "dof_pos", "dof_pos_limits")}
    env = types.SimpleNamespace(dt=float(z["dt"]), torque_limits=torch.full((12,), 33.5), **x)
    terms = joints.joint_terms(env)
    assert list(terms) == J.METRICS and all(t.shape == (64, 12) and t.dtype == torch.float32 for t in terms.values())
    for term, reward in (("torque_sq", "torques"), ("vel_sq", "dof_vel"), ("acc_sq", "dof_acc"), ("pos_limit_excess", "dof_pos_limits")):
        got, want = terms[term].sum(dim=1).numpy(), z[f"s{seed}_out_{reward}"]
        assert got.tobytes() == want.tobytes(), (term, np.abs(got - want).max())
    assert z[f"s{seed}_out_dof_pos_limits"].min() == 0.0 < z[f"s{seed}_out_dof_pos_limits"].max()          # rows on the limits, rows beyond
    # and the model's values are the same numbers: the same fp32 operations, elementwise
    cfg = J.config(dt=float(z["dt"]), pos_lower=x["dof_pos_limits"][:, 0].tolist(), pos_upper=x["dof_pos_limits"][:, 1].tolist())
    for j in range(12):
        values = J.step_values(cfg, j, *(x[k][:, j].numpy() for k in ("torques", "dof_vel", "dof_pos", "last_dof_vel")))
        for m, name in enumerate(J.METRICS):
            assert bits(values[m]) == bits(terms[name][:, j].numpy()), (name, j)


# ---- 4. the model by hand ---------------------------------------------------------------------------------------------------------------
def test_model_bins():
    L = 28.0
    x = np.array([-28.0, -21.0, np.nextafter(f32(-21.0), f32(-np.inf)), -0.0, 0.0, -0.001, 6.99, 7.0, 20.99, 21.0, 27.99,
                  28.0, 1e30, -1e30, -29.0, 3.0e38, -14.0, -7.0, 14.0], f32)
    assert J.bin_of(x, L).tolist() == [0, 1, 0, 4, 4, 3, 4, 5, 6, 7, 7, 7, 7, 0, 0, 7, 2, 3, 6]
    assert J.bin_of(np.array([-1e-30], f32), L).tolist() == [4]          # x / L + 1 rounds to 1: the bin is the fp32 expression's
    for k in range(8):                                                  # every edge opens its bin; a thousandth below it is the bin below
        edge = f32(33.5) * (f32(k) / f32(4) - f32(1))
        assert J.bin_of(np.array([edge, edge - f32(0.001)], f32), 33.5).tolist() == [k, max(k - 1, 0)]
    # one ulp below an edge: x / L + 1 is rounded to fp32, which can land on the edge itself (here 0.75 - 3e-8 -> 0.75)
    assert J.bin_of(np.array([np.nextafter(f32(-8.375), f32(-np.inf))], f32), 33.5).tolist() == [3]
    import go1eval_host as G
    assert G.joint_edges(28.0).tolist() == [-28.0, -21.0, -14.0, -7.0, 0.0, 7.0, 14.0, 21.0, 28.0]


def one_step(cfg, tau, qd, q, prev=0.0, reset=0, age=5, st=None):
    """a model of one environment whose twelve joints all carry the same values; returns the state"""
    full = lambda v: np.full((12, 1), v, f32)
    st = st or J.State(1, full(prev))
    snap = dict(torques=full(tau), dof_vel=full(qd), dof_pos=full(q), reset_buf=np.array([reset], np.uint8), episode_length_buf=np.array([age], np.int32))
    return J.accumulate(st, cfg, snap)


def folded(st, j=0):
    """{metric: (count, nonfinite, min, max)} of joint j of environment 0"""
    return {name: (int(st.count[j * J.M + m, 0]), int(st.nonfinite[j * J.M + m, 0]), float(st.min[j * J.M + m, 0]), float(st.max[j * J.M + m, 0]))
            for m, name in enumerate(J.METRICS)}


def test_model_values_of_one_step():
    cfg = J.config()                                                    # hip: 33.5 N m, 50 rad/s, [-0.72, 0.72]
    st = one_step(cfg, tau=2.0, qd=-3.0, q=-0.97, prev=-2.5)
    acc = f32((f32(-2.5) - f32(-3.0)) / f32(0.02))
    excess = float(-(f32(-0.97) - f32(-0.72)))
    one = lambda v: (1, 0, float(v), float(v))
    assert folded(st) == dict(torque_abs=one(2.0), torque_sq=one(4.0), vel_abs=one(3.0), vel_sq=one(9.0), acc_sq=one(acc * acc), power_pos=one(0.0),
                              power_neg=one(6.0), pos_limit_excess=one(excess), torque_saturated=one(0.0), vel_saturated=one(0.0))
    assert st.sum[J.POWER_NEG, 0] == 6.0 and st.sumsq[J.POWER_NEG, 0] == 36.0 and not np.signbit(st.min[J.POWER_POS, 0])
    assert st.hist[0, :, 0].sum() == 1 and st.hist[0, 4 * 8 + 3, 0] == 1        # tau = 2 in bin 4, qd = -3 in bin 3
    thigh = folded(st, 1)                                               # the thigh's limits are [-0.78, 3.92]: -0.97 is below them too
    assert thigh["pos_limit_excess"] == one(float(-(f32(-0.97) - f32(-0.78)))) and st.hist[1, 4 * 8 + 3, 0] == 1
    st = one_step(cfg, tau=-2.0, qd=-3.0, q=0.97)
    assert folded(st)["power_pos"] == one(6.0) and folded(st)["power_neg"] == one(0.0)
    assert folded(st)["pos_limit_excess"] == one(float(f32(0.97) - f32(0.72))) and folded(st, 1)["pos_limit_excess"] == one(0.0)
    for q in (-0.72, 0.72, 0.0):                                        # on a limit is inside
        assert folded(one_step(cfg, 1.0, 1.0, q))["pos_limit_excess"] == one(0.0)


def test_model_saturation_edges():
    cfg = J.config(soft_torque_limit=0.9, soft_vel_limit=0.8)
    at = f32(0.9) * f32(33.5)
    for tau, want in ((at, 1.0), (-at, 1.0), (np.nextafter(at, f32(0)), 0.0), (np.nextafter(-at, f32(0)), 0.0), (f32(33.5), 1.0), (f32(1e30), 1.0), (f32(0), 0.0)):
        assert folded(one_step(cfg, tau, 1.0, 0.0))["torque_saturated"][2] == want, tau
    for j, limit in ((0, 50.0), (1, 28.0), (2, 28.0)):
        at = f32(0.8) * f32(limit)
        for qd, want in ((at, 1.0), (-at, 1.0), (np.nextafter(at, f32(0)), 0.0), (np.nextafter(at, f32(100)), 1.0)):
            assert folded(one_step(cfg, 1.0, qd, 0.0), j)["vel_saturated"][2] == want, (j, qd)


def test_model_nonfinite_inputs():
    cfg = J.config()
    got = folded(one_step(cfg, NAN, 1.0, 0.0))
    assert got["torque_abs"][:2] == (0, 1) and got["torque_sq"][:2] == (0, 1) and got["vel_abs"][:2] == (1, 0)
    assert got["power_pos"] == (1, 0, 0.0, 0.0) and got["power_neg"] == (1, 0, 0.0, 0.0) and got["torque_saturated"] == (1, 0, 0.0, 0.0)
    st = one_step(cfg, np.inf, -1.0, 0.0)
    got = folded(st)
    assert got["torque_abs"][:2] == (0, 1) and got["power_neg"][:2] == (0, 1) and got["power_pos"] == (1, 0, 0.0, 0.0) and got["torque_saturated"][2] == 1.0
    assert st.hist.sum() == 0                                           # no sample without a finite torque and a finite speed
    st = one_step(cfg, 1.0, -np.inf, 0.0, prev=1.0)
    got = folded(st)
    assert got["vel_abs"][:2] == (0, 1) and got["acc_sq"][:2] == (0, 1) and got["vel_saturated"][2] == 1.0 and st.hist.sum() == 0
    assert np.isneginf(st.prev_dof_vel).all()                           # the previous velocity is whatever dof_vel held
    for q in (NAN, np.inf, -np.inf):
        st = one_step(cfg, 1.0, 1.0, q)
        assert folded(st)["pos_limit_excess"][:2] == (0, 1) and folded(st)["torque_abs"][:2] == (1, 0) and st.hist.sum() == 12
    st = one_step(cfg, 1e30, 1e30, 0.0)                                 # finite, far outside: the last bins, squares overflow
    assert st.hist[:, 63, 0].tolist() == [1] * 12 and folded(st)["torque_sq"][:2] == (0, 1) and folded(st)["torque_abs"][:2] == (1, 0)


def test_model_previous_velocity_across_a_reset_and_the_warm_up():
    cfg = J.config(warmup_steps=2)
    acc = lambda a, b: float(f32((f32(a) - f32(b)) / f32(0.02)) * f32((f32(a) - f32(b)) / f32(0.02)))
    st = one_step(cfg, 1.0, 3.0, 0.0, prev=2.0, age=3)                  # the clear took 2.0 from dof_vel
    assert folded(st)["acc_sq"] == (1, 0, acc(2, 3), acc(2, 3)) and st.prev_dof_vel[0, 0] == 3.0
    one_step(cfg, 1.0, 0.0, 0.0, reset=1, age=0, st=st)                 # a reset step: the simulator left 0; nothing is folded
    assert folded(st)["acc_sq"][0] == 1 and st.hist.sum() == 12 and (st.steps[0], st.resets[0]) == (2, 1) and st.prev_dof_vel[0, 0] == 0.0
    one_step(cfg, 1.0, 0.5, 0.0, age=1, st=st)                          # warm-up: counted in steps only, but the velocity is remembered
    one_step(cfg, 1.0, 0.75, 0.0, age=2, st=st)                         # age == warmup_steps is still warm-up
    assert folded(st)["acc_sq"][0] == 1 and (st.steps[0], st.resets[0]) == (4, 1) and st.prev_dof_vel[0, 0] == 0.75
    one_step(cfg, 1.0, 1.0, 0.0, age=3, st=st)
    assert folded(st)["acc_sq"] == (2, 0, acc(0.75, 1), acc(2, 3)) and st.hist.sum() == 24
    one_step(cfg, 1.0, 0.0, 0.0, reset=2, age=0, st=st)                 # two resets in a row
    one_step(cfg, 1.0, 0.0, 0.0, reset=1, age=0, st=st)
    one_step(cfg, 1.0, -1.0, 0.0, age=3, st=st)
    assert folded(st)["acc_sq"][0] == 3 and st.max[J.ACC_SQ, 0] == acc(0, -1) == acc(2, 3) and (st.steps[0], st.resets[0]) == (8, 3)
    table, hist = J.reduce(st, [0], 2)
    assert table.shape == (2, 121, 6) and hist.shape == (2, 12, 8, 8) and hist.dtype == np.uint64
    assert table[0, 120].tolist() == [1.0, 8.0, 3.0, 0.0, 0.0, 0.0] and table[1, 120].tolist() == [0.0] * 6
    assert table[0, J.ACC_SQ, 0] == 3.0 and table[0, J.ACC_SQ, 4] == acc(2, 3) and table[0, 11 * J.M + J.TORQUE_ABS].tolist() == [3.0, 1.0, 0.0, 1.0, 1.0, 0.0]
    assert table[1, :120, 0].tolist() == [0.0] * 120 and np.isnan(table[1, :120, 1:5]).all() and hist[0].sum() == 36 and hist[1].sum() == 0
    assert hist[0, :, 4].sum() == 36                                    # tau = 1: torque bin 4 in every sample


# ---- 5. go1eval.hip under the SIMT emulator against the model -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    import go1eval_host as G
    return G.load_library(eval_emu())


def joints_on(device, cfg, N, lib=None):
    """a go1eval_host.Go1Joints on buffers of its own on `device`, as the environment would build it, and those buffers"""
    import go1eval_host as G
    tensors = {k: torch.zeros(12, N, device=device) for k in ("torques", "dof_vel", "dof_pos")}
    tensors.update(reset_buf=torch.zeros(N, dtype=torch.uint8, device=device), episode_length_buf=torch.zeros(N, dtype=torch.int32, device=device))
    B = types.SimpleNamespace(device=torch.device(device), **tensors)
    S = types.SimpleNamespace(num_envs=N, torque_limits=cfg.torque_limit, dof_pos_soft_lower=cfg.pos_lower, dof_pos_soft_upper=cfg.pos_upper)
    jm = G.Go1Joints(S, B, cfg.dt, cfg.vel_limit, soft_torque_limit=cfg.soft_torque_limit, soft_vel_limit=cfg.soft_vel_limit, lib=lib)
    if torch.device(device).type == "cpu":
        jm._stream = lambda: None
    return jm, B


def drive(jm, B, cfg, snaps, start, group, groups):
    """the scripted steps through the library: the velocities of the clear, arm for `groups` groups, upload a snapshot, accumulate,
    ...; returns read() and the accumulators.  arm() sizes the tables by the largest id it is given, so the ids outside the tables are
    handed to the kernels afterwards."""
    inside = np.where(group >= groups, -1, group)
    assert inside.max() == groups - 1
    B.dof_vel.copy_(torch.from_numpy(start))
    jm.arm(inside, cfg.warmup_steps)
    jm.group.copy_(torch.from_numpy(group))
    for s in snaps:
        for k, a in s.items():
            getattr(B, k).copy_(torch.from_numpy(a))
        jm.accumulate()
    jm.disarm()
    res = jm.read()
    acc = {k: t.cpu().numpy() for k, t in jm.acc.items()}
    return res, acc


def check_against_the_model(res, acc, cfg, snaps, start, kind, group, groups, N):
    """accumulators, state, histogram and both result tables against tests/joint_ref.py, bit for bit; then what the script was written
    to drive"""
    st = J.run(cfg, snaps, N, start)
    for k in ACCUMULATORS:
        assert acc[k].shape == (120, N) and bits(acc[k].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    for k, name in (("prev_dof_vel", "prev_dof_vel"), ("steps", "steps"), ("resets", "resets"), ("hist", "env_hist")):
        assert res[name].shape == getattr(st, k).shape and bits(res[name].view(getattr(st, k).dtype)) == bits(getattr(st, k)), k
    want, want_hist = J.reduce(st, group, groups)
    table = np.concatenate([np.stack([res["metrics"][m] for m in J.METRICS], axis=2).reshape(groups, 120, 6), np.zeros((groups, 1, 6))], axis=1)
    table[:, 120, :3] = res["groups"]
    assert table.shape == want.shape == (groups, J.ROWS, 6)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and bits(table) == bits(want)
    assert res["hist"].shape == (groups, 12, 8, 8) and bits(res["hist"].view(np.uint64)) == bits(want_hist)
    # the script: resets on the first step, mid-script and twice in a row; the warm-up after each
    count, nonfinite = acc["count"].view(np.uint32).reshape(12, 10, N), acc["nonfinite"].view(np.uint32).reshape(12, 10, N)
    steps = len(snaps)
    assert (res["steps"] == steps).all() and (res["resets"][kind == 1] >= 4).all() and snaps[0]["reset_buf"][kind == 1].all()
    assert (count[:, J.TORQUE_SATURATED, kind == 0] <= steps - cfg.warmup_steps).all() and count[:, J.TORQUE_SATURATED].max() == steps - cfg.warmup_steps
    assert (count[:, J.TORQUE_SATURATED, kind == 1] <= 2).all()           # steps 3, 4 of the script only: every other one resets or is warm-up
    # saturation on both sides of both tests, every bin of both axes, samples beyond both position limits
    for m in (J.TORQUE_SATURATED, J.VEL_SATURATED):
        assert set(np.unique(acc["max"].reshape(12, 10, N)[:, m][count[:, m] > 0]).tolist()) == {0.0, 1.0}
    env_hist = res["env_hist"].view(np.uint32).reshape(12, 8, 8, N)
    assert (env_hist[:, :, :, kind == 2].sum(axis=(0, 2, 3)) > 0).all() and (env_hist[:, :, :, kind == 3].sum(axis=(0, 1, 3)) > 0).all()
    assert acc["max"].reshape(12, 10, N)[:, J.POS_LIMIT_EXCESS, kind == 4].max() == 0.5 and (acc["min"].reshape(12, 10, N)[:, J.POS_LIMIT_EXCESS, kind == 4] == 0.0).any()
    # +-inf and NaN in each of the three inputs were met, and entered no sum; 1e30 overflowed its square and nothing else
    odd = kind == 5
    for m in (J.TORQUE_ABS, J.VEL_ABS, J.POS_LIMIT_EXCESS, J.ACC_SQ, J.TORQUE_SQ):
        assert nonfinite[:, m, odd].sum() > 0, J.METRICS[m]
    assert np.isfinite(acc["sum"]).all() and np.isfinite(acc["sumsq"]).all() and nonfinite[:, J.TORQUE_SATURATED:].sum() == 0
    assert nonfinite[:, J.TORQUE_SQ, kind == 2].sum() > 0 and nonfinite[:, J.TORQUE_ABS, kind == 2].sum() == 0
    # the histogram holds one sample per folded step wherever both inputs were finite, and fewer where they were not
    quiet = ~odd
    assert (env_hist.sum(axis=(1, 2))[:, quiet] == count[:, J.TORQUE_SATURATED, quiet]).all()
    assert (env_hist.sum(axis=(1, 2))[:, odd] < count[:, J.TORQUE_SATURATED, odd]).any()
    # a joint that never moves: zero speed, zero acceleration, zero power, speed bin 4
    still = kind == 6
    assert (acc["max"].reshape(12, 10, N)[:, [J.VEL_ABS, J.ACC_SQ, J.POWER_POS, J.POWER_NEG]][:, :, still] == 0.0).all()
    assert (env_hist[:, :, 4, still].sum(axis=1) == count[:, J.VEL_ABS, still]).all()
    g = res["groups"]
    assert g[:, 0].sum() == np.isin(group, range(groups)).sum() < N and (g[:, 1] == steps * g[:, 0]).all() and g[1].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(want[1, :120, 1:5]).all() and res["hist"][1].sum() == 0
    return st


@pytest.mark.parametrize("N", [70, 300])                                 # one ragged block per joint; a full block and a ragged one per joint
def test_emulated_joint_kernels_follow_the_model(emu, N):
    groups = 4
    rng = np.random.default_rng(200 + N)
    cfg, snaps, start, kind = J.scripted_steps(rng, N)
    assert len(snaps) == 12 and set(kind.tolist()) == set(range(len(J.KINDS)))
    group = scripted_groups(rng, N, groups)
    jm, B = joints_on("cpu", cfg, N, lib=emu)
    res, acc = drive(jm, B, cfg, snaps, start, group, groups)
    assert jm.cfg.num_groups == groups and {-1, groups} <= set(group.tolist())
    check_against_the_model(res, acc, cfg, snaps, start, kind, group, groups, N)
    assert res["tau_edges"].shape == res["vel_edges"].shape == (12, 9) and res["tau_edges"][1, 8] == 30.0 and res["vel_edges"][2, 0] == -28.0
    with pytest.raises(RuntimeError, match="go1eval_joint_accumulate failed: -12"):
        jm.cfg.vel_limit[4] = 0.0
        jm.accumulate()


# ---- 6. the environment hooks without a GPU ---------------------------------------------------------------------------------------------------
def test_joint_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    monkeypatch.delitem(sys.modules, "go1eval_host", raising=False)
    cfg = apply_train_config(make_cfg(), num_envs=16)
    cfg.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=cfg)
    env.step(torch.zeros(16, 12))
    for call in (lambda: env.start_joint_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_joint_metrics, env.read_joint_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert "go1eval_host" not in sys.modules and env._joints is None          # an environment that never measures never imports the library
    env.step(torch.zeros(16, 12))                                             # and stepping goes on


# ---- 7. the sweep's host pieces and the tool -----------------------------------------------------------------------------------------------------
def fixed_result():
    import go1eval_host as G
    row = lambda mean, top: np.array([[[30.0, mean, 0.5, 0.0, top, 0.0]] * 12, [[10.0, 3 * mean, 0.5, 0.0, 2 * top, 1.0]] * 12])
    joints = {m: row(0.25, 2.0) for m in J.METRICS}
    joints["torque_saturated"], joints["acc_sq"] = row(0.125, 1.0), row(400.0, 900.0)
    joints["pos_limit_excess"][1] = [[0.0, NAN, NAN, NAN, NAN, 0.0]] * 12     # a cell that folded nothing
    hist = np.zeros((2, 12, 8, 8), np.int64)
    hist[0, :, 4, 4], hist[1, :, 7, 0], hist[1, 0, 0, 7] = 30, 10, 5
    return dict(preset="static_medium", cells=[(0.5, 0.0, (0.5, 0.0, 0.0)), (1.0, 0.0, (0.5, 0.0, 0.0))], joints=joints,
                joint_groups=np.array([[8.0, 320.0, 1.0], [8.0, 320.0, 0.0]]), hist=hist, tau_edges=np.stack([G.joint_edges(33.5)] * 12),
                vel_edges=np.stack([G.joint_edges(v) for v in [50.0, 28.0, 28.0] * 4]), metrics={}, groups=np.zeros((2, 5)), torque_limit=[33.5] * 12,
                vel_limit=[50.0, 28.0, 28.0] * 4, soft_torque_limit=1.0, soft_vel_limit=1.0, dof_names=list(G.DOF_NAMES), num_envs=16, steps=40,
                warmup_steps=5, seed=1, dt=0.02)


def test_joint_table_json_and_envelope(tmp_path):
    from go1_gym_learn.eval_metrics import joints
    res = fixed_result()
    pooled = joints.pool_cells(res["joints"]["torque_abs"])
    mean = (30 * 0.25 + 10 * 0.75) / 40
    second = (30 * (0.25 + 0.0625) + 10 * (0.25 + 0.5625)) / 40
    assert pooled.shape == (12, 6) and pooled[3].tolist() == [40.0, mean, np.sqrt(second - mean * mean), 0.0, 4.0, 12.0 / 12]
    assert joints.pool_cells(res["joints"]["pos_limit_excess"])[0].tolist() == [30.0, 0.25, 0.5, 0.0, 2.0, 0.0]
    md = joints.joint_markdown_table(res).splitlines()
    assert md[0] == ("| joint | mean \\|tau\\| | max \\|tau\\| | at torque limit | max \\|qd\\| | at speed limit | driving power | braking power | rms acc | "
                     "mean limit excess | max limit excess |").replace("\\|", "|") and md[1] == "|" + "---|" * 11 and len(md) == 14
    assert md[2] == "| FL_hip_joint | 0.38 | 4.00 | 0.1875 | 4.00 | 0.3750 | 0.38 | 0.38 | 24.5 | 0.2500 | 2.0000 |" and md[13].startswith("| RR_calf_joint | 0.38 |")
    js = json.loads(json.dumps(joints.joint_to_json(res)))
    assert js["cells"][1] == dict(vx=1.0, yaw=0.0, gait=[0.5, 0.0, 0.0]) and js["group_fields"] == J.GROUP_FIELDS and js["dof_names"][11] == "RR_calf_joint"
    assert js["joints"]["acc_sq"][0][5][1] == 400.0 and js["hist"][1][0][0][7] == 5 and js["tau_edges"][0][0] == -33.5 and js["vel_limit"][:3] == [50.0, 28.0, 28.0]
    assert np.array(js["hist"]).shape == (2, 12, 8, 8) and js["joint_groups"][0] == [8.0, 320.0, 1.0]
    path = tmp_path / "envelope.png"
    joints.plot_envelope(res["hist"], str(path))
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and path.stat().st_size > 5000
    joints.plot_envelope(np.zeros((12, 8, 8)), str(path))                     # an empty histogram still draws


def test_tool_accepts_a_joint_sweep(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import joints
    base = ["--checkpoint", "c", "--out", str(tmp_path)]
    a = eval_sweep.parse_args(base + ["--joints", "--vx", "0.5", "1.0", "--envs", "16", "--steps", "40", "--warmup-steps", "5", "--presets", "static_medium"])
    assert a.joints and not a.tiles and (a.vx, a.envs, a.steps, a.terrain) == ([0.5, 1.0], 16, 40, None)
    assert not eval_sweep.parse_args(base).joints and eval_sweep.parse_args(base + ["--joints", "--terrain", "heightfield"]).terrain == "heightfield"
    for bad in (["--joints", "--terrain"], ["--joints", "--behaviour"], ["--joints", "--response", "--switch", "vx", "0", "1"],
                ["--joints", "--push", "--magnitude", "1", "--direction", "0"]):
        with pytest.raises(SystemExit):
            eval_sweep.parse_args(base + bad)
    seen = {}

    def sweep_stub(policy, preset, grid, **kw):
        seen.update(kw, preset=preset, grid=grid)
        return fixed_result()
    monkeypatch.setattr(joints, "run_joint_sweep", sweep_stub)
    (tmp_path / "eval").mkdir()
    eval_sweep.run_joints(a, None, dict(vx=a.vx, yaw=a.yaw, gait=[(0.5, 0.0, 0.0)]))
    assert seen == dict(preset="static_medium", grid=dict(vx=[0.5, 1.0], yaw=[0.0], gait=[(0.5, 0.0, 0.0)]), num_envs=16, steps=40, warmup_steps=5, seed=1,
                        terrain=None)
    js = json.load(open(tmp_path / "eval" / "static_medium_joints.json"))
    assert js["preset"] == "static_medium" and js["hist"][0][3][4][4] == 30
    md = (tmp_path / "eval" / "static_medium_joints.md").read_text()
    assert "| FL_hip_joint | 0.38 | 4.00 | 0.1875 |" in md and md in capsys.readouterr().out + "\n"
    assert (tmp_path / "eval" / "static_medium_envelope.png").read_bytes()[:4] == b"\x89PNG"
