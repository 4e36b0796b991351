"""GPU checks of foot loading (include/go1feet.h, libgo1feet.so): the scripted buffers of the emulator test through the compiled kernels
against the model of tests/feet_ref.py bit for bit, the real environment under a scripted trot-like action pattern with the model
replayed on the buffers read back after every step and the simulation's indifference to an armed measurement, the standing robot's
vertical load against its weight, and the recorded cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (foot_metrics_cost.txt: the source of
profiles/foot_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import feet_ref as F
from test_foot_metrics import ACCUMULATORS, REPO, SHAPES, STANDING_D, check_against_the_model, drive, feet_groups, feet_on, standing_env, trot_action
from test_gpu_response_trace import DEVICE, StandStill, make_env, report
from test_gpu_terrain_metrics import same_bits

pytestmark = pytest.mark.gpu


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPES)
def test_feet_kernels_equal_the_model_bit_for_bit(N):
    groups = 3
    rng = np.random.default_rng(300 + N)                                 # the emulator test's script
    cfg, snaps, kind = F.scripted_steps(rng, N)
    group = feet_groups(rng, N, groups)
    fm, B = feet_on(DEVICE, cfg, N)
    res, acc = drive(fm, B, cfg, snaps, group, groups)
    check_against_the_model(res, acc, cfg, snaps, kind, group, groups, N)
    again = fm.read()                                                    # the reduction leaves what it reads as it is
    assert all(again[k].tobytes() == res[k].tobytes() for k in ("groups", "profile_sum", "profile_count", "steps", "resets", "prev_contact", "stance_impulse"))
    assert all(again["metrics"][m].tobytes() == res["metrics"][m].tobytes() for m in F.METRICS)


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def snapshot(env):
    """host copies of the buffers go1feet_accumulate reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in F.INPUTS}


def test_feet_through_the_environment():
    """80 steps of the trot-like script: the kernel's accumulators, state, profile and tables equal the model replayed on the buffers read
    back after every step, bit for bit; the simulation is bit-identical with the measurement armed and not armed; and the script did
    what it is there for: every foot folded at least one touchdown and one completed stance."""
    N, STEPS, WARMUP, GROUPS = 64, 80, 2, 3
    plain, env = make_env(N, "plane", 20.0, seed=4), make_env(N, "plane", 20.0, seed=4)
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    for e in (plain, env):
        e.reset()
    env.start_foot_metrics(group, warmup_steps=WARMUP)
    assert plain._feet is None
    snaps = []
    for step in range(STEPS):
        action = trot_action(step, N).to(DEVICE)
        plain.step(action)
        env.step(action)
        snaps.append(snapshot(env))
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, env.buffers.tensors[name]), (step, name)
    env.stop_foot_metrics()
    res = env.read_foot_metrics()
    fm = env._feet
    c, S = fm.cfg, env.sim_config
    assert c.dt == np.float32(env.dt) and c.terrain_friction == np.float32(S.terrain_friction) == np.float32(env.cfg.terrain.static_friction)
    assert c.max_contact_force == np.float32(env.cfg.rewards.max_contact_force) and (c.num_envs, c.warmup_steps, c.num_groups) == (N, WARMUP, GROUPS)
    cfg = F.config(dt=c.dt, terrain_friction=c.terrain_friction, max_contact_force=c.max_contact_force, warmup_steps=WARMUP)
    st = F.run(cfg, snaps, N)
    count = st.count.reshape(4, 12, N)
    touchdowns, stances = count[:, F.TOUCHDOWN_FORCE].sum(axis=1), count[:, F.STANCE_TIME].sum(axis=1)
    print(f"\ntouchdowns per foot {touchdowns.tolist()}, completed stances per foot {stances.tolist()}, resets {int(st.resets.sum())}, "
          f"duty factors {(st.sum.reshape(4, 12, N)[:, F.CONTACT].sum(axis=1) / count[:, F.CONTACT].sum(axis=1)).round(3).tolist()}, "
          f"largest Fz {st.max.reshape(4, 12, N)[:, F.FORCE_NORMAL].max():.1f} N, largest friction use {st.max.reshape(4, 12, N)[:, F.FRICTION_USE].max():.3f}")
    assert (touchdowns >= 1).all() and (stances >= 1).all()              # else the comparison below would assert nothing about the events
    for k in ACCUMULATORS:
        assert fm.acc[k].cpu().numpy().view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    for k in F.STATE:
        name = "env_" + k if k.startswith("profile") else k
        assert res[name].view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    want, want_profile = F.reduce(st, group.numpy(), GROUPS)
    for m, name in enumerate(F.METRICS):
        assert res["metrics"][name].shape == (GROUPS, 4, 6) and res["metrics"][name].tobytes() == np.ascontiguousarray(want[:, m:48:12]).tobytes(), name
    assert res["groups"].tobytes() == np.ascontiguousarray(want[:, 48, :3]).tobytes()
    assert np.stack([res["profile_sum"], res["profile_count"]], axis=-1).tobytes() == want_profile.tobytes()
    assert res["steps"].tolist() == [STEPS] * N and (res["profile_count"].sum(axis=2) == res["metrics"]["contact"][:, :, 0]).all()
    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_foot_metrics()["steps"].tolist() == [STEPS] * N


def test_a_standing_robot_loads_its_feet_with_its_weight():
    """Zero actions on the plane (test_foot_metrics.standing_env: no gravity randomisation), N = 64, a 50-step warm-up, then 100 steps:
    the four feet's mean vertical force (the profile over all bins) sums to (total mass + mean payload) x 9.81 within max(2 d, 1 %).
    d is the CPU oracle's relative deviation on the same scenario, test_foot_metrics.test_standing_robot_through_the_oracle:
    d = -3.65 % (the oracle, as the kernel, reports the last substep's force, one substep in four, of a robot that rocks on its
    hind feet: their duty factor is 0.95; and the simulator's g is 9.8).  Twice that covers the kernel-against-oracle contact-force
    tolerance of 1 %: the bound is 7.3 %."""
    from go1_gym_learn.eval_metrics import feet
    N, WARMUP, STEPS = 64, 50, 100
    env = standing_env(N, DEVICE)
    env.reset()
    env.start_foot_metrics(torch.zeros(N, dtype=torch.int32), warmup_steps=WARMUP)
    for _ in range(WARMUP + STEPS):
        env.step(torch.zeros(N, 12, device=DEVICE))
    env.stop_foot_metrics()
    res = env.read_foot_metrics()
    assert res["resets"].sum() == 0 and (res["profile_count"][0].sum(axis=1) == N * (STEPS + 1)).all()     # reset() took the first step of the episode
    load = (res["profile_sum"][0].sum(axis=1) / res["profile_count"][0].sum(axis=1)).sum()
    weight = (feet.total_mass() + float(env.payloads.mean())) * 9.81
    bound = max(2.0 * abs(STANDING_D), 0.01)
    print(f"\nvertical load {load:.3f} N against a weight of {weight:.3f} N: {100.0 * (load / weight - 1.0):+.3f} % (bound {100.0 * bound:.2f} %); "
          f"duty factors {res['metrics']['contact'][0, :, 1].round(4).tolist()}")
    assert abs(load / weight - 1.0) <= bound


# ---- 3. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_foot_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    N, WINDOW, WARMUP = 64, 30, 5
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--feet", "--vx", "0.5", "1.0", "--envs", str(N), "--steps", str(WINDOW),
                               "--warmup-steps", str(WARMUP), "--seed", "5", "--presets", "static_medium", "--terrain", "plane"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_feet(a, StandStill(), dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits]))
    stem = tmp_path / "eval" / "static_medium"
    js = json.load(open(str(stem) + "_feet.json"))
    md = open(str(stem) + "_feet.md").read()
    print(md)
    assert open(str(stem) + "_grf.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(str(stem) + "_grf.png") > 5000
    assert [c["vx"] for c in js["cells"]] == [0.5, 1.0] and js["foot_names"] == ["FL", "FR", "RL", "RR"] and len(md.splitlines()) >= 2 + 2 + 8
    feet = {m: np.array([[[np.nan if x is None else x for x in row] for row in cell] for cell in t]) for m, t in js["feet"].items()}
    count = np.array(js["profile_count"])
    assert count.shape == (2, 4, 16) and all(feet[m].shape == (2, 4, 6) for m in F.METRICS)
    groups = np.array(js["feet_groups"])
    assert groups[:, 0].tolist() == [N / 2] * 2 and groups[:, 1].tolist() == [N / 2 * WINDOW] * 2
    # the sweep's reset() has already taken one step: window step k leaves episode_length_buf = k + 1, so steps WARMUP .. WINDOW fold
    assert (feet["contact"][:, :, 0] > 0).all() and (feet["contact"][:, :, 0] <= N / 2 * (WINDOW - WARMUP + 1)).all()
    assert count.sum(axis=2).tolist() == feet["contact"][:, :, 0].tolist()                # every folded step of a finite robot is one profile sample
    assert sum(feet[m][:, :, 5].sum() for m in F.METRICS) == 0                            # nothing non-finite in a standing robot
    assert (feet["contact"][:, :, 1] > 0.5).all() and (feet["force_normal"][:, :, 3] > 1.0).all() and (feet["friction_use"][:, :, 3] >= 0).all()
    profile = np.array([[[np.nan if x is None else x for x in foot] for foot in cell] for cell in js["profile"]])
    load = (np.nansum(profile * count, axis=2) / count.sum(axis=2)).sum(axis=1)           # per cell: the four feet's mean vertical force
    assert (0.5 * js["body_weight"] < load).all() and (load < 1.5 * js["body_weight"]).all()
    assert np.allclose(np.array(js["load_share"]).sum(axis=1), 1.0)


# ---- 4. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_foot_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_foot_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_foot_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_foot_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].tolist() == [STEPS] * ENVS
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "feet armed", "read"]
    lines = [f"Cost of the foot-loading measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  feet armed: the same loop after start_foot_metrics(): one go1feet_accumulate launch more",
              "per step (4 x 1024 threads); its cost is the difference of the two columns.  read: read_foot_metrics() (go1feet_reduce over",
              "16 groups: 16 x 49 metric rows and 16 x 4 profiles, and the device-to-host copies of the two tables, the per-environment",
              "profile and the state arrays), events around the call."]
    report("foot_metrics_cost.txt", "\n".join(lines))
