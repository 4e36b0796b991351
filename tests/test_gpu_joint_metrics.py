"""GPU checks of per-joint actuator usage (include/go1eval.h, sixth kernel family): the scripted buffers of the emulator test through
libgo1eval.so against the model of tests/joint_ref.py bit for bit, the simulation's indifference to an armed measurement, the real
environment under random actions with the model replayed on the buffers read back after every step, the two cross-family identities
with the scalar table, the joint sweep end to end through the tool, and the recorded cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (joint_metrics_cost.txt: the source of
profiles/joint_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import joint_ref as J
from test_gpu_response_trace import DEVICE, StandStill, make_env, report
from test_gpu_terrain_metrics import same_bits
from test_joint_metrics import ACCUMULATORS, REPO, check_against_the_model, drive, joints_on
from test_terrain_metrics import scripted_groups

pytestmark = pytest.mark.gpu
MAX_TORQUES, POWER = 5, 6                                                # rows of the scalar table (enum Go1EvalMetric)


# ---- 1. the kernels on the scripted buffers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 300])                                 # one ragged block per joint; a full block and a ragged one per joint
def test_joint_kernels_equal_the_model_bit_for_bit(N):
    groups = 4
    rng = np.random.default_rng(200 + N)                                 # the emulator test's script
    cfg, snaps, start, kind = J.scripted_steps(rng, N)
    group = scripted_groups(rng, N, groups)
    jm, B = joints_on(DEVICE, cfg, N)
    res, acc = drive(jm, B, cfg, snaps, start, group, groups)
    check_against_the_model(res, acc, cfg, snaps, start, kind, group, groups, N)
    again = jm.read()                                                    # the reduction leaves what it reads as it is
    assert all(again[k].tobytes() == res[k].tobytes() for k in ("groups", "hist", "steps", "resets", "prev_dof_vel", "env_hist"))
    assert all(again["metrics"][m].tobytes() == res["metrics"][m].tobytes() for m in J.METRICS)


# ---- 2. the real environment --------------------------------------------------------------------------------------------------------------
def test_arming_writes_nothing_of_the_simulators():
    N, STEPS = 40, 30
    plain, armed = make_env(N, "plane", 20.0, seed=3), make_env(N, "plane", 20.0, seed=3)
    armed.start_joint_metrics(torch.arange(N) % 4, warmup_steps=3)
    assert plain._joints is None
    generator = torch.Generator().manual_seed(11)
    for step in range(STEPS):
        action = (2.0 * torch.rand(N, 12, generator=generator) - 1.0).to(DEVICE)
        plain.step(action)
        armed.step(action)
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, armed.buffers.tensors[name]), (step, name)
    assert torch.allclose(plain.buffers.episode_log, armed.buffers.episode_log, rtol=1e-5, atol=1e-6)
    armed.stop_joint_metrics()
    res = armed.read_joint_metrics()
    assert res["steps"].tolist() == [STEPS] * N and res["groups"][:, :2].tolist() == [[10.0, 10.0 * STEPS]] * 4
    armed.step(torch.zeros(N, 12, device=DEVICE))                        # disarmed: no further launch
    assert armed.read_joint_metrics()["steps"].tolist() == [STEPS] * N


def snapshot(env):
    """host copies of the buffers go1eval_joint_accumulate reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in J.INPUTS}


def make_pd_env(N, seed):
    """test_gpu_response_trace.make_env on the plane with the position controller in place of the actuator network: the network's
    output stays below about 26 N m whatever it is asked for, so under it no torque ever reaches the 33.5 N m clip"""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    c = apply_train_config(make_cfg(), num_envs=N)
    c.terrain.mesh_type = "plane"
    c.control.control_type = "P"
    c.env.episode_length_s = 20.0
    torch.manual_seed(seed)
    np.random.seed(seed)
    return VelocityTrackingEasyEnv(sim_device=DEVICE, headless=True, cfg=c)


# The random actions are uniform in [-SCALE, SCALE] and drawn anew every step.  The action scale of the configuration is 0.25 rad per
# unit (half of that at the hips) on a 20 N m / rad position gain: SCALE = 8 asks for targets up to 2 rad away, 40 N m, beyond the 33.5 N m
# clip, and throws the joints against their limits and the robot off its feet.
SCALE, SEED = 8.0, 21


def test_joints_through_the_environment():
    N, STEPS, WARMUP, GROUPS = 40, 40, 2, 3
    env = make_pd_env(N, seed=4)
    assert env.sim_config.control_type == 0 and env.sim_config.kp == 20.0
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    idle = torch.arange(N) % 3 == 0                                      # a third of the robots gets zero actions
    env.step(torch.zeros(N, 12, device=DEVICE))
    start = env.buffers.dof_vel.cpu().numpy().copy()                     # what go1eval_joint_clear takes as the previous velocity
    env.start_metrics(group, warmup_steps=WARMUP)
    env.start_joint_metrics(group, warmup_steps=WARMUP)
    generator = torch.Generator().manual_seed(SEED)
    snaps = []
    for _ in range(STEPS):
        action = SCALE * (2.0 * torch.rand(N, 12, generator=generator) - 1.0)
        action[idle] = 0.0
        env.step(action.to(DEVICE))
        snaps.append(snapshot(env))
    env.stop_metrics()
    env.stop_joint_metrics()
    res = env.read_joint_metrics()
    scalar = env.read_metrics()
    jm = env._joints
    c = jm.cfg
    S = env.sim_config
    assert list(c.torque_limit) == [33.5] * 12 and list(c.vel_limit) == [50.0, 28.0, 28.0] * 4 and c.dt == np.float32(env.dt)
    assert list(c.pos_lower) == [np.float32(v) for v in S.dof_pos_soft_lower] and list(c.pos_upper) == [np.float32(v) for v in S.dof_pos_soft_upper]
    assert (c.soft_torque_limit, c.soft_vel_limit) == (env.cfg.rewards.soft_torque_limit, env.cfg.rewards.soft_dof_vel_limit)
    cfg = J.config(dt=c.dt, soft_torque_limit=c.soft_torque_limit, soft_vel_limit=c.soft_vel_limit, torque_limit=list(c.torque_limit),
                   vel_limit=list(c.vel_limit), pos_lower=list(c.pos_lower), pos_upper=list(c.pos_upper), warmup_steps=WARMUP)
    # the model on the buffers read back after each step.  First what the inputs were chosen to show (conditions on the inputs, seen
    # through the model): both values of torque_saturated, a positive excess beyond a position limit, and at least one reset
    st = J.run(cfg, snaps, N, start)
    rows = lambda a, m: a.reshape(12, 10, N)[:, m]
    saturated, excess = rows(st.max, J.TORQUE_SATURATED), rows(st.max, J.POS_LIMIT_EXCESS)
    print(f"\nresets {int(st.resets.sum())} in {int((st.resets > 0).sum())} environments; joints that saturated in {int((saturated.max(axis=0) == 1.0).sum())} "
          f"environments; largest excess {excess.max():.4f} rad; largest |tau| {rows(st.max, J.TORQUE_ABS).max():.3f} N m, |qd| {rows(st.max, J.VEL_ABS).max():.2f} rad/s")
    assert saturated.max() == 1.0 and rows(st.min, J.TORQUE_SATURATED).min() == 0.0 and excess.max() > 0.0 and st.resets.sum() >= 1
    # the kernel's accumulators, state and tables equal the replay bit for bit
    for k in ACCUMULATORS:
        assert jm.acc[k].cpu().numpy().view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    for k, name in (("prev_dof_vel", "prev_dof_vel"), ("steps", "steps"), ("resets", "resets"), ("hist", "env_hist")):
        assert res[name].view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    want, want_hist = J.reduce(st, group.numpy(), GROUPS)
    for m, name in enumerate(J.METRICS):
        assert res["metrics"][name].shape == (GROUPS, 12, 6) and res["metrics"][name].tobytes() == np.ascontiguousarray(want[:, m:120:10]).tobytes(), name
    assert res["groups"].tobytes() == np.ascontiguousarray(want[:, 120, :3]).tobytes() and res["hist"].view(np.uint64).tobytes() == want_hist.tobytes()
    assert res["hist"].sum(axis=(2, 3)).tolist() == res["metrics"]["torque_abs"][:, :, 0].tolist()      # every folded step is one sample
    # ---- the cross-family identities, per environment, with the scalar table armed with the same groups and warm-up
    sacc = {k: t.cpu().numpy() for k, t in env._metrics.acc.items()}
    assert scalar["groups"][:, 0].tolist() == res["groups"][:, 0].tolist()
    assert (sacc["count"][MAX_TORQUES] == rows(st.count, J.TORQUE_ABS)[0].view(np.int32)).all()           # the same steps were folded
    # max over the joints of max[torque_abs] == max[max_torques]: the same fabsf values, the same fmaxf
    assert rows(st.max, J.TORQUE_ABS).max(axis=0).tobytes() == sacc["max"][MAX_TORQUES].tobytes()
    # the sum of the joints' driving minus braking power against sum[power_consumption]: the scalar family rounds each step's fp64 sum
    # of the twelve fp32 products to fp32 once, an error of at most 2^-24 |P_step| <= 2^-24 max(|min|, |max|) per step; the joint rows
    # add the same products in fp64.  Twice that, times the steps: a derived bound.
    signed = (rows(st.sum, J.POWER_POS) - rows(st.sum, J.POWER_NEG)).sum(axis=0)
    count = sacc["count"][POWER].astype(np.float64)
    largest = np.where(count > 0, np.maximum(np.abs(sacc["min"][POWER].astype(np.float64)), np.abs(sacc["max"][POWER].astype(np.float64))), 0.0)
    bound = 2.0 * 2.0 ** -24 * count * largest
    gap = np.abs(signed - sacc["sum"][POWER])
    print(f"power: largest gap {gap.max():.3e} W steps against a bound of {bound[gap.argmax()]:.3e}; largest |power sum| {np.abs(sacc['sum'][POWER]).max():.1f}")
    assert sacc["nonfinite"][POWER].sum() == 0 and (gap <= bound).all(), (gap.max(), bound.min())


# ---- 3. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_joint_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    N, WINDOW, WARMUP = 64, 30, 5
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--joints", "--vx", "0.5", "1.0", "--envs", str(N), "--steps", str(WINDOW),
                               "--warmup-steps", str(WARMUP), "--seed", "5", "--presets", "static_medium", "--terrain", "plane"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_joints(a, StandStill(), dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits]))
    stem = tmp_path / "eval" / "static_medium"
    js = json.load(open(str(stem) + "_joints.json"))
    md = open(str(stem) + "_joints.md").read()
    print(md)
    assert open(str(stem) + "_envelope.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(str(stem) + "_envelope.png") > 5000
    assert [c["vx"] for c in js["cells"]] == [0.5, 1.0] and js["dof_names"][0] == "FL_hip_joint" and len(md.splitlines()) >= 16
    hist, joints = np.array(js["hist"]), {m: np.array(t) for m, t in js["joints"].items()}
    assert hist.shape == (2, 12, 8, 8) and all(joints[m].shape == (2, 12, 6) for m in J.METRICS)
    groups = np.array(js["joint_groups"])
    assert groups[:, 0].tolist() == [N / 2] * 2 and groups[:, 1].tolist() == [N / 2 * WINDOW] * 2
    # histogram totals equal the metric counts: every folded step of a finite robot is one sample
    assert hist.sum(axis=(2, 3)).tolist() == joints["torque_abs"][:, :, 0].tolist() == joints["vel_saturated"][:, :, 0].tolist()
    # the sweep's reset() has already taken one step: window step k leaves episode_length_buf = k + 1, so steps WARMUP .. WINDOW fold
    assert (joints["torque_abs"][:, :, 0] > 0).all() and (joints["torque_abs"][:, :, 0] <= N / 2 * (WINDOW - WARMUP + 1)).all()
    assert sum(joints[m][:, :, 5].sum() for m in J.METRICS) == 0          # nothing non-finite in a standing robot
    assert (joints["torque_abs"][:, :, 4] <= 33.5).all() and (joints["power_pos"][:, :, 3] >= 0).all() and (joints["power_neg"][:, :, 3] >= 0).all()


# ---- 4. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_joint_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_joint_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_joint_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_joint_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].tolist() == [STEPS] * ENVS
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "joints armed", "read"]
    lines = [f"Cost of the per-joint measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  joints armed: the same loop after start_joint_metrics(): one go1eval_joint_accumulate launch more",
              "per step (12 x 1024 threads); its cost is the difference of the two columns.  read: read_joint_metrics() (go1eval_joint_reduce over",
              "16 groups: 16 x 121 metric rows and 16 x 12 histograms, and the device-to-host copies of the two tables, the per-environment",
              "histogram and the state arrays), events around the call."]
    report("joint_metrics_cost.txt", "\n".join(lines))
