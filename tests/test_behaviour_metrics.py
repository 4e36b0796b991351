"""CPU checks of the behaviour table (gait and behaviour tracking in evaluation sweeps): the host mirror against
include/go1eval.h, the host definitions BEHAVIOUR_FNS against a fixture produced by executing the reference's reward methods
(tests/golden/gen_behaviour_metrics.py), the stride rules on a hand-computed case (the fp64 model tests/behaviour_ref.py and
the host's StrideTracker alike), the kernel source under the SIMT emulator against the model, and the host surface."""
import ctypes
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import behaviour_ref as R
import eval_ref as E
from test_eval_metrics import eval_emu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "include", "go1eval.h")
GOLDEN = os.path.join(REPO, "tests", "golden")


# ---- 1. the host mirror against the header ------------------------------------------------------------------------------------
def test_behaviour_mirror_matches_the_header():
    import go1eval_host as G
    from go1_gym_learn.eval_metrics import behaviour as BH
    src = open(HEADER).read()
    assert f"#define GO1EVAL_NUM_BEHAVIOUR {G.NUM_BEHAVIOUR}" in src and G.NUM_BEHAVIOUR == R.M == len(G.BEHAVIOUR_NAMES)
    body = src[src.index("typedef struct Go1BehaviourBuffers"):src.index("} Go1BehaviourBuffers;")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in G.Go1BehaviourBuffers._fields_]
    body = src[src.index("typedef struct Go1BehaviourConfig"):src.index("} Go1BehaviourConfig;")]
    fields = re.findall(r"\b(int32_t|float) (\w+);", body)
    assert [n for _, n in fields] == [f for f, _ in G.Go1BehaviourConfig._fields_]
    assert [n for _, n in fields] == ["num_envs", "num_commands", "num_height_points", "warmup_steps", "num_groups", "dt", "base_height_target"]
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [ctype[t] for t, _ in fields] == [t for _, t in G.Go1BehaviourConfig._fields_]
    enum = src[src.index("enum Go1BehaviourMetric"):src.index("};", src.index("enum Go1BehaviourMetric"))]
    order = [n for n, _ in sorted(re.findall(r"GO1EVAL_(\w+) = (\d+)", enum), key=lambda p: int(p[1]))]
    assert [n.lower() for n in order] == G.BEHAVIOUR_NAMES == R.METRICS == BH.BEHAVIOUR_NAMES
    assert list(BH.BEHAVIOUR_FNS) == G.BEHAVIOUR_NAMES[:7] and G.STRIDE_NAMES == BH.PER_STRIDE == G.BEHAVIOUR_NAMES[7:]
    assert R.INPUTS == G._BEHAVIOUR_INPUTS
    assert set(G.EXPORTED_SYMBOLS) >= {"go1eval_behaviour_clear", "go1eval_behaviour_accumulate", "go1eval_behaviour_reduce"}
    assert BH.COMMAND_INDEX == dict(vx=0, vy=1, yaw=2, body_height=3, frequency=4, phase=5, offset=6, bound=7, duration=8,
                                    footswing_height=9, pitch=10, roll=11, stance_width=12, stance_length=13)


def test_behaviour_entry_points_validate_their_arguments_without_a_gpu():
    import __graft_entry__ as g
    import go1eval_host as G
    g.build_eval_hip()
    lib = G.load_library()
    cfg, buf = G.Go1BehaviourConfig(), G.Go1BehaviourBuffers()
    fns = (lib.go1eval_behaviour_clear, lib.go1eval_behaviour_accumulate, lib.go1eval_behaviour_reduce)
    for fn in fns:
        assert fn(None, None, None) == -1
        assert fn(ctypes.byref(cfg), None, None) == -1
        assert fn(ctypes.byref(cfg), ctypes.byref(buf), None) == -1        # num_envs = 0
    cfg.num_envs = -3
    assert all(fn(ctypes.byref(cfg), ctypes.byref(buf), None) == -1 for fn in fns)
    cfg.num_envs = 8
    assert all(fn(ctypes.byref(cfg), ctypes.byref(buf), None) == -2 for fn in fns)     # no accumulators, no stride state
    keep = [np.zeros(8 * 16, np.float64) for _ in range(10)]
    for name, a in zip(G._ACCUMULATORS + G._STRIDE_STATE, keep):
        setattr(buf, name, a.ctypes.data)
    assert lib.go1eval_behaviour_accumulate(ctypes.byref(cfg), ctypes.byref(buf), None) == -3      # no inputs
    assert lib.go1eval_behaviour_reduce(ctypes.byref(cfg), ctypes.byref(buf), None) == -5          # no groups, no table
    for name in G._BEHAVIOUR_INPUTS:
        setattr(buf, name, keep[0].ctypes.data)
    assert lib.go1eval_behaviour_accumulate(ctypes.byref(cfg), ctypes.byref(buf), None) == -4      # heights without a point count
    cfg.num_height_points = 3
    assert lib.go1eval_behaviour_accumulate(ctypes.byref(cfg), ctypes.byref(buf), None) == -6      # num_commands 0, dt 0
    cfg.num_commands = 15
    assert lib.go1eval_behaviour_accumulate(ctypes.byref(cfg), ctypes.byref(buf), None) == -6      # dt 0


# ---- 2. the host definitions against the reference's reward methods ---------------------------------------------------------------
CASES = [(0, 15), (1, 13), (0, 12)]


def _fixture_env(z, key, num_commands):
    t = lambda k: torch.from_numpy(z[f"{key}_in_{k}"])
    N = t("commands").shape[0]
    env = types.SimpleNamespace(measured_heights=0, feet_indices=torch.tensor([4, 8, 12, 16]))
    env.cfg = types.SimpleNamespace(rewards=types.SimpleNamespace(base_height_target=float(z["base_height_target"])),
                                    commands=types.SimpleNamespace(num_commands=num_commands))
    env.commands = t("commands")
    env.root_states = torch.zeros(N, 13)
    env.root_states[:, 0:7] = t("base_pose")
    env.contact_forces = torch.zeros(N, 17, 3)
    env.contact_forces[:, [4, 8, 12, 16], :] = t("foot_forces")
    for k in ("foot_positions", "foot_velocities", "desired_contact_states", "foot_indices"):
        setattr(env, k, t(k))
    env.last_actions, env.last_last_actions = t("actions_now"), t("actions_before")
    return env


@pytest.mark.parametrize("seed,num_commands", CASES)
def test_behaviour_fns_equal_the_references_reward_values(seed, num_commands):
    from go1_gym_learn.eval_metrics.behaviour import BEHAVIOUR_FNS
    z = np.load(os.path.join(GOLDEN, "behaviour_metrics.npz"))
    key = f"s{seed}_c{num_commands}"
    env = _fixture_env(z, key, num_commands)
    assert env.commands.shape == (64, num_commands)
    got = {n: fn(env, None, None).numpy() for n, fn in BEHAVIOUR_FNS.items()}
    want = {n: z[f"{key}_out_{n}"] for n in ("jump", "orientation_control", "feet_clearance_cmd_linear", "raibert_heuristic", "feet_slip", "action_rate")}
    assert all(v.shape == (64,) and v.dtype == np.float32 for v in list(got.values()) + list(want.values()))
    # the same fp32 operations as the reference's: the same bits (the bound executing the reference twice on one machine gives)
    assert (got["body_height_err"] * got["body_height_err"]).tobytes() == (-want["jump"]).tobytes()
    assert got["feet_clearance"].tobytes() == want["feet_clearance_cmd_linear"].tobytes()
    assert np.array_equal(got["raibert_heuristic"], want["raibert_heuristic"], equal_nan=True)
    assert np.array_equal(np.isnan(got["raibert_heuristic"]), np.isnan(want["raibert_heuristic"]))
    assert not np.isfinite(want["raibert_heuristic"][0]) and np.isfinite(want["raibert_heuristic"][1:]).all()     # the robot commanded to 0 Hz
    assert got["feet_slip"].tobytes() == want["feet_slip"].tobytes()
    assert got["action_rate"].tobytes() == want["action_rate"].tobytes()
    # orientation_err is the square root of the reference's value.  The root of the same fp32 number is the same fp32 number ...
    assert got["orientation_err"].tobytes() == np.sqrt(want["orientation_control"]).tobytes()
    # ... and squared again (in fp64, so that the square adds nothing) it is within ONE fp32 ROUNDING OF THE VALUE: the root's
    # relative error is at most 2^-24, squaring doubles it, 2^-23 * value
    back = got["orientation_err"].astype(np.float64) ** 2
    assert (np.abs(back - want["orientation_control"].astype(np.float64)) <= 2.0 ** -23 * want["orientation_control"].astype(np.float64)).all()
    assert want["orientation_control"].max() > 0.01
    # contact_match has no counterpart among the reward methods: by its definition, from the fixture's forces
    contact = z[f"{key}_in_foot_forces"][:, :, 2] > 1.0
    assert 0 < contact.mean() < 1 and not contact[1, 0] and contact[2, 1]              # forces of exactly 1.0 N and of 1.5 N
    assert np.array_equal(got["contact_match"], (contact == (z[f"{key}_in_desired_contact_states"] > 0.5)).mean(axis=1).astype(np.float32))


def test_model_step_values_follow_the_host_definitions():
    """the fp64 model (from the header's text) and the fp32 host definitions (pinned to the reference above) state the same formulas"""
    from go1_gym_learn.eval_metrics.behaviour import BEHAVIOUR_FNS
    z = np.load(os.path.join(GOLDEN, "behaviour_metrics.npz"))
    for seed, num_commands in CASES:
        env = _fixture_env(z, f"s{seed}_c{num_commands}", num_commands)
        snap = _snapshot_of(env)
        with np.errstate(all="ignore"):
            model = R.step_values(snap, num_commands, float(z["base_height_target"]))
        for m, name in enumerate(BEHAVIOUR_FNS):
            host = BEHAVIOUR_FNS[name](env, None, None).double().numpy()
            fin = np.isfinite(host)
            assert np.array_equal(fin, np.isfinite(model[m])), name
            assert np.allclose(host[fin], model[m][fin], rtol=2e-5, atol=2e-6), (name, np.abs(host[fin] - model[m][fin]).max())


def _snapshot_of(env):
    """the SoA buffers ([k][N]) of an environment object with [N, k] views"""
    N = env.commands.shape[0]
    s = dict(commands=env.commands.t(), root_states=env.root_states.t(), contact_forces=env.contact_forces.reshape(N, 51).t(),
             foot_positions=env.foot_positions.reshape(N, 12).t(), foot_velocities=env.foot_velocities.reshape(N, 12).t(),
             desired_contact_states=env.desired_contact_states.t(), foot_indices=env.foot_indices.t(), last_actions=env.last_actions.t(),
             last_last_actions=env.last_last_actions.t())
    s = {k: np.ascontiguousarray(v.numpy()) for k, v in s.items()}
    s["measured_heights"] = None
    return s


# ---- 3. the stride rules on a hand-computed case ---------------------------------------------------------------------------------------
DT = 0.02
CONTACTS = [1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 1]
HEIGHTS = [0.02, 0.02, 0.05, 0.09, 0.06, 0.02, 0.021, 0.02, 0.07, 0.11, 0.02]


def _run_strides(contacts, heights, counted, commands):
    """contacts, heights: [steps][feet of one environment]; counted: [steps] bool.  Returns (model state, events per step of the
    model, events per step of StrideTracker in fp64)"""
    from go1_gym_learn.eval_metrics.behaviour import StrideTracker
    st, tracker = R.State(1), StrideTracker(1, DT, dtype=np.float64)
    cmd = np.asarray(commands, np.float64).reshape(-1, 1)
    per_step, tracked = [], []
    for c, h, live in zip(contacts, heights, counted):
        c4, h4 = np.zeros((4, 1), bool), np.zeros((4, 1))
        c4[:len(c), 0], h4[:len(h), 0] = c, h
        before = st.count[R.FREQ, 0]
        R.accumulate(st, np.zeros((7, 1)), c4, h4, cmd, [0 if live else 1], [50], 0, DT)
        per_step.append(int(st.count[R.FREQ, 0] - before))
        tracked.append(tracker.step(c4.T, h4.T, cmd.T, np.array([live])))
    assert np.array_equal(tracker.prev_contact.T, st.prev_contact) and np.array_equal(tracker.stride_steps.T, st.stride_steps)
    assert np.array_equal(tracker.stance_steps.T, st.stance_steps) and np.array_equal(tracker.swing_peak.T, st.swing_peak)
    return st, per_step, tracked


def _commands(frequency=3.0, duty=0.5, swing=0.08):
    cmd = np.zeros(15)
    cmd[4], cmd[8], cmd[9] = frequency, duty, swing
    return cmd


def test_stride_rules_by_hand():
    n = len(CONTACTS)
    st, per_step, tracked = _run_strides([[c] for c in CONTACTS], [[h] for h in HEIGHTS], [True] * n, _commands())
    # index 0: prev_contact is unknown, no touchdown.  index 5: the first touchdown, no stride has ended.  index 10: L = 5, stance 3
    assert per_step == [0] * 10 + [1] and [len(t) for t in tracked] == per_step
    dt32 = np.float64(np.float32(DT))
    assert st.count[R.FREQ, 0] == st.count[R.DUTY, 0] == st.count[R.SWING, 0] == 1 and st.completed_strides == 1
    assert np.isclose(st.sum[R.FREQ, 0], 10.0 - 3.0, rtol=1e-7) and st.sum[R.FREQ, 0] == 1.0 / (5 * dt32) - 3.0
    assert np.isclose(st.sum[R.DUTY, 0], 0.6 - 0.5, rtol=1e-12)
    peak = max(HEIGHTS[5:10])
    assert peak == 0.11 and np.isclose(st.sum[R.SWING, 0], (0.11 - 0.02) - 0.08, rtol=1e-5)
    e, f, freq, duty, swing = tracked[10][0]
    assert (e, f) == (0, 0) and np.isclose(freq, 7.0) and np.isclose(duty, 0.1) and np.isclose(swing, 0.01, rtol=1e-5)
    # after the touchdown at index 10 the next stride has begun: one step, in stance, peak = this step's height
    assert st.stride_steps[0, 0] == 1 and st.stance_steps[0, 0] == 1 and st.swing_peak[0, 0] == HEIGHTS[10] and st.prev_contact[0, 0] == 1
    # the feet that never touched the ground saw no touchdown
    assert (st.stride_steps[1:, 0] == -1).all() and (st.prev_contact[1:, 0] == 0).all()


@pytest.mark.parametrize("what", ["reset", "warmup"])
def test_a_reset_or_a_warmup_step_mid_stride_discards_the_stride(what):
    from go1_gym_learn.eval_metrics.behaviour import StrideTracker
    st, tracker = R.State(1), StrideTracker(1, DT, dtype=np.float64)
    cmd = _commands().reshape(-1, 1)
    events = 0
    for k, (c, h) in enumerate(zip(CONTACTS + [1, 0, 0, 1], HEIGHTS + [0.02, 0.05, 0.05, 0.02])):
        c4, h4 = np.zeros((4, 1), bool), np.zeros((4, 1))
        c4[0, 0], h4[0, 0] = c, h
        hit = k == 7                                                   # mid-stride: the stride began at index 5
        reset, elb = ([1], [0]) if (hit and what == "reset") else ([0], [3]) if hit else ([0], [40])
        R.accumulate(st, np.ones((7, 1)), c4, h4, cmd, reset, elb, 3, DT)        # warm-up 3: episode_length_buf = 3 is excluded
        events += len(tracker.step(c4.T, h4.T, cmd.T, np.array([not hit])))
        if hit:
            assert st.prev_contact[0, 0] == 2 and st.stride_steps[0, 0] == -1 and st.discarded_strides == 1
    # index 10 is a touchdown (index 9 was counted, out of contact) but no stride is under way: nothing folded there; the stride
    # 10 -> 14 (contacts 1, 1, 0, 0 | 1) is the only one that completes: L = 4, stance 2
    assert st.count[R.FREQ, 0] == 1 and st.completed_strides == 1 and events == 1
    assert st.sum[R.FREQ, 0] == 1.0 / (4 * np.float64(np.float32(DT))) - 3.0 and st.sum[R.DUTY, 0] == 0.0
    assert st.count[0, 0] == len(CONTACTS) + 4 - 1 and st.excluded == 1          # the per-step metrics skipped that one step


def test_two_feet_touching_down_in_one_step_fold_in_foot_order():
    #            foot 1 strides of 4 steps, foot 3 strides of 6 steps; both touch down at index 13
    c1 = [0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1]
    c3 = [0, 1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1]
    h1 = [0.05 + 0.01 * k for k in range(14)]
    h3 = [0.30 - 0.01 * k for k in range(14)]
    contacts = [[0, a, 0, b] for a, b in zip(c1, c3)]
    heights = [[0, a, 0, b] for a, b in zip(h1, h3)]
    st, per_step, tracked = _run_strides(contacts, heights, [True] * 14, _commands(frequency=0.0, duty=0.0, swing=0.0))
    assert per_step == [0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 2] and st.double_touchdowns == 2         # index 1 (no stride yet) and index 13
    assert [(e, f) for e, f, *_ in tracked[13]] == [(0, 1), (0, 3)]
    dt32 = np.float64(np.float32(DT))
    f4, f6 = 1.0 / (4 * dt32), 1.0 / (6 * dt32)
    assert st.sum[R.FREQ, 0] == (((f4 + f6) + f4) + f4) + f6                      # index 5: foot 1; 7: foot 3; 9: foot 1; 13: foot 1, then foot 3
    assert st.count[R.DUTY, 0] == 5 and np.isclose(st.sum[R.DUTY, 0], 3 * 0.5 + 2 * 0.5)
    assert st.max[R.SWING, 0] == (h3[1] - np.float64(np.float32(0.02)))           # foot 3's first stride: its highest sample is its first
    assert tracked[13][0][2] == f4 and tracked[13][1][2] == f6


# ---- 4. the kernel source under the SIMT emulator against the model -----------------------------------------------------------------------
class Synthetic:
    """snapshots whose contacts follow per-foot periodic schedules (period 3..6 steps, random phase, occasional chatter)"""

    def __init__(self, rng, N, P):
        self.rng, self.N, self.P = rng, N, P
        self.period = rng.integers(3, 7, (4, N))
        self.stance = rng.integers(1, self.period)                      # 1 .. period - 1 steps of a period in contact
        self.phase = rng.integers(0, 6, (4, N))
        self.phase[1, ::2] = self.phase[0, ::2]                        # feet 0 and 1 of every second environment in step: double touchdowns
        self.period[1, ::2], self.stance[1, ::2] = self.period[0, ::2], self.stance[0, ::2]
        self.elb = rng.integers(1, 30, N)
        self.commands = rng.standard_normal((15, N))
        self.commands[4] = rng.uniform(2.0, 4.0, N)
        self.commands[4, rng.random(N) < 0.05] = 0.0                    # robots commanded to 0 Hz: a non-finite raibert_heuristic
        self.commands[12], self.commands[13] = rng.uniform(0.1, 0.4, N), rng.uniform(0.35, 0.45, N)

    def step(self, k):
        rng, N, P = self.rng, self.N, self.P
        contact = ((k + self.phase) % self.period) < self.stance
        contact ^= rng.random((4, N)) < 0.03                            # chatter
        forces = 10.0 * rng.standard_normal((17, 3, N))
        forces[list(R.FEET_BODIES), 2, :] = np.where(contact, rng.uniform(1.5, 80.0, (4, N)), rng.uniform(0.0, 1.0, (4, N)))
        q = rng.standard_normal((4, N))
        root = rng.standard_normal((13, N))
        root[3:7] = q / np.linalg.norm(q, axis=0)
        pos = rng.standard_normal((4, 3, N)) * 0.2 + root[None, 0:3]
        pos[:, 2] = rng.uniform(0.0, 0.2, (4, N))
        desired = rng.random((4, N))
        desired[:, ::3] = desired[:, ::3] > 0.5
        s = dict(commands=self.commands, root_states=root, measured_heights=None if P == 0 else 0.1 * rng.standard_normal((P, N)),
                 contact_forces=forces.reshape(51, N), foot_positions=pos.reshape(12, N), foot_velocities=rng.standard_normal((12, N)),
                 desired_contact_states=desired, foot_indices=rng.random((4, N)), last_actions=rng.standard_normal((12, N)),
                 last_last_actions=rng.standard_normal((12, N)))
        s = {n: (None if v is None else np.ascontiguousarray(v, np.float32)) for n, v in s.items()}
        reset = rng.random(N) < 0.1
        self.elb = np.where(reset, 0, self.elb + 1)
        s["reset_buf"], s["episode_length_buf"] = reset.astype(np.uint8), self.elb.astype(np.int32)
        return s


@pytest.mark.parametrize("N,P,num_commands", [(300, 17, 15), (64, 0, 12)])
def test_emulated_behaviour_kernels_follow_the_model(N, P, num_commands):
    import go1eval_host as G
    lib = ctypes.CDLL(eval_emu())
    rng = np.random.default_rng(17 + N)
    W, groups, target = 2, 3, 0.30
    group = rng.integers(-1, groups + 1, N).astype(np.int32)           # includes -1 and an id outside the table
    group[group == 1] = 0                                               # group 1 stays empty
    dt = dict(count=np.uint32, sum=np.float64, sumsq=np.float64, min=np.float32, max=np.float32, nonfinite=np.uint32)
    acc = {k: np.full((R.M, N), 99, d) for k, d in dt.items()}          # (garbage: go1eval_behaviour_clear has to initialise)
    sdt = dict(prev_contact=np.uint8, stride_steps=np.int32, stance_steps=np.int32, swing_peak=np.float32)
    stride = {k: np.full((4, N), 77, d) for k, d in sdt.items()}
    table = np.full((groups, R.M, 6), -1.0)
    cfg, buf = G.Go1BehaviourConfig(), G.Go1BehaviourBuffers()
    cfg.num_envs, cfg.num_commands, cfg.num_height_points, cfg.warmup_steps, cfg.num_groups = N, num_commands, P, W, groups
    cfg.dt, cfg.base_height_target = DT, target
    for k, a in list(acc.items()) + list(stride.items()):
        setattr(buf, k, a.ctypes.data)
    buf.group, buf.results = group.ctypes.data, table.ctypes.data
    assert lib.go1eval_behaviour_clear(ctypes.byref(cfg), ctypes.byref(buf), None) == 0
    assert (acc["count"] == 0).all() and (acc["min"] == np.inf).all() and (stride["prev_contact"] == 2).all() and (stride["stride_steps"] == -1).all()
    model, source = R.State(N), Synthetic(rng, N, P)
    for step in range(40):
        s = source.step(step)
        for k, a in s.items():
            setattr(buf, k, None if a is None else a.ctypes.data)
        assert lib.go1eval_behaviour_accumulate(ctypes.byref(cfg), ctypes.byref(buf), None) == 0
        R.accumulate_snapshot(model, s, W, DT, num_commands, target)
    assert lib.go1eval_behaviour_reduce(ctypes.byref(cfg), ctypes.byref(buf), None) == 0
    # one of each event in the data
    assert model.completed_strides > 100 and model.discarded_strides > 0 and model.double_touchdowns > 0 and model.excluded > 0
    assert model.nonfinite[R.METRICS.index("raibert_heuristic")].sum() > 0 and model.nonfinite.sum() == model.nonfinite[4].sum()
    for k in ("count", "nonfinite"):
        assert np.array_equal(acc[k], getattr(model, k)), k
    for k in sdt:
        assert np.array_equal(stride[k].astype(np.float64), getattr(model, k).astype(np.float64)), k
    assert np.array_equal(acc["sum"][0], model.sum[0]) and np.array_equal(acc["sumsq"][0], model.sumsq[0])       # contact_match: multiples of 0.25
    assert np.array_equal(acc["min"][0], model.min[0]) and np.array_equal(acc["max"][0], model.max[0])
    for m in range(R.M):                                                # fp32 arithmetic against fp64: a few roundings of the largest term
        scale = max(1.0, np.abs(model.sum[m]).max())
        err = np.abs(acc["sum"][m] - model.sum[m]).max()
        assert err <= 2e-6 * scale, (R.METRICS[m], err, scale)
    want = R.reduce(model, group, groups)
    assert np.array_equal(table[:, :, 0], want[:, :, 0]) and np.array_equal(table[:, :, 5], want[:, :, 5])
    assert np.array_equal(np.isnan(table), np.isnan(want)) and np.isnan(table[1, :, 1:5]).all()
    assert np.allclose(table, want, rtol=2e-4, atol=1e-5, equal_nan=True)
    # the reduction of the kernel's own accumulators in the model's fixed order: the same bits
    own = R.State(N)
    for k in dt:
        setattr(own, k, acc[k].astype(np.float64 if dt[k] != np.uint32 else np.int64))
    assert np.array_equal(table, R.reduce(own, group, groups), equal_nan=True)


# ---- 5. the host surface -------------------------------------------------------------------------------------------------------------------
def test_behaviour_hooks_on_cpu_buffers(monkeypatch):
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
    assert env._behaviour is None and env._metrics is None
    with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
        env.start_metrics(torch.zeros(16, dtype=torch.int32), warmup_steps=2, behaviour=True)
    assert "go1eval_host" not in sys.modules and env._behaviour is None
    env.step(torch.zeros(16, 12))
    # the host definitions run on the environment object itself
    from go1_gym_learn.eval_metrics.behaviour import BEHAVIOUR_FNS
    for name, fn in BEHAVIOUR_FNS.items():
        v = fn(env, None, None)
        assert v.shape == (16,) and v.dtype == torch.float32, name


def test_behaviour_cells_commands_and_tables():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import behaviour as BH
    from go1_gym_learn.eval_metrics import sweep
    axes = dict(frequency=[2, 4], footswing_height=[0.05, 0.15], pitch=[-0.2])
    cells = BH.behaviour_cells(axes)
    assert cells == [dict(frequency=2.0, footswing_height=0.05, pitch=-0.2), dict(frequency=2.0, footswing_height=0.15, pitch=-0.2),
                     dict(frequency=4.0, footswing_height=0.05, pitch=-0.2), dict(frequency=4.0, footswing_height=0.15, pitch=-0.2)]
    with pytest.raises(KeyError, match="unknown command"):
        BH.behaviour_cells(dict(speed=[1.0]))
    cmd = BH.behaviour_command_table(cells, 15, "cpu")
    held = sweep.command_table([(1.0, 0.0, sweep.GAITS["trotting"])], 15, "cpu")[0]
    assert cmd.shape == (4, 15) and cmd[:, 4].tolist() == [2.0, 2.0, 4.0, 4.0] and torch.allclose(cmd[:, 9], torch.tensor([0.05, 0.15, 0.05, 0.15]))
    assert torch.allclose(cmd[:, 10], torch.full((4,), -0.2))
    others = [c for c in range(15) if c not in (4, 9, 10)]
    assert torch.equal(cmd[:, others], held[others].repeat(4, 1)) and cmd[0, 0] == 1.0 and cmd[0, 8] == 0.5
    assert BH.behaviour_command_table(cells, 15, "cpu", base_cell=(0.5, 0.25, sweep.GAITS["pacing"]))[2, [0, 2, 7]].tolist() == [0.5, 0.25, 0.5]
    with pytest.raises(ValueError, match="none for 'stance_length'"):
        BH.behaviour_command_table([dict(stance_length=0.4)], 13, "cpu")
    res = dict(preset="static_medium", cells=cells, num_envs=256, steps=60, warmup_steps=5, seed=5,
               metrics={n: np.arange(24, dtype=np.float64).reshape(4, 6) for n in E.METRICS}, groups=np.ones((4, 5)),
               behaviour={n: np.arange(24, dtype=np.float64).reshape(4, 6) + i for i, n in enumerate(R.METRICS)})
    md = BH.behaviour_markdown_table(res).splitlines()
    assert len(md) == 6 and md[0].startswith("| frequency | footswing_height | pitch | envs | fall rate | contact_match | body_height_err")
    assert md[0].endswith("| swing_height_err | strides |") and md[-1].startswith("| 4 | 0.15 | -0.2 | 1 | 1.000 | 19 ± 20 | 20 ± 21 |") and md[-1].endswith("| 25 |")
    js = json.loads(json.dumps(BH.behaviour_to_json(res)))
    assert js["cells"][3] == dict(frequency=4.0, footswing_height=0.15, pitch=-0.2) and js["fields"] == E.FIELDS
    assert sorted(js["behaviour"]) == sorted(R.METRICS) and js["behaviour"]["duty_factor_err"][3][1] == 27.0 and js["metrics"]["CoT"][3][1] == 19.0
    # a result without the behaviour table goes through eval_sweep.to_json as before
    cells3 = sweep.grid_cells(dict(vx=[0.5], yaw=[0.0, 0.5], gait=[sweep.GAITS["trotting"]]))
    plain = dict(preset="rand_large", cells=cells3, num_envs=64, steps=10, warmup_steps=1, seed=2,
                 metrics={n: np.arange(12, dtype=np.float64).reshape(2, 6) for n in E.METRICS}, groups=np.ones((2, 5)))
    js = json.loads(json.dumps(eval_sweep.to_json(plain)))
    assert sorted(js) == sorted(["preset", "num_envs", "steps", "warmup_steps", "seed", "cells", "fields", "metrics", "group_fields", "groups"])
    assert js["cells"] == [dict(vx=0.5, yaw=0.0, gait=[0.5, 0.0, 0.0]), dict(vx=0.5, yaw=0.5, gait=[0.5, 0.0, 0.0])]
    assert js["metrics"]["CoT"] == [[0.0, 1.0, 2.0, 3.0, 4.0, 5.0], [6.0, 7.0, 8.0, 9.0, 10.0, 11.0]] and js["groups"] == [[1.0] * 5] * 2


def test_eval_sweep_parses_the_behaviour_axes():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--behaviour", "--axis", "frequency", "2", "4", "--axis", "pitch", "-0.2"])
    assert a.behaviour and eval_sweep.behaviour_axes(a) == dict(frequency=[2.0, 4.0], pitch=[-0.2])
    a = eval_sweep.parse_args(["--checkpoint", "c", "--out", "o"])
    assert not a.behaviour and a.axis is None
    with pytest.raises(SystemExit):
        eval_sweep.behaviour_axes(eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--behaviour", "--axis", "speed", "1"]))
    with pytest.raises(SystemExit):
        eval_sweep.behaviour_axes(eval_sweep.parse_args(["--checkpoint", "c", "--out", "o", "--behaviour"]))
