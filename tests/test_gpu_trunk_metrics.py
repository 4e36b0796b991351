"""GPU checks of the trunk family (include/go1trunk.h, libgo1trunk.so): the scripted buffers of the emulator test through the compiled
kernels against the model of tests/trunk_ref.py bit for bit, the real environment under a scripted trot with the model replayed on the
buffers read back after every step, the simulation's indifference to an armed measurement, the agreement with the foot family's
contact counts, the telescoping of the accelerations, the standing robot's support margin, the sweep through the tool, and the
recorded cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (trunk_metrics_cost.txt: the source of
profiles/trunk_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import trunk_ref as T
from test_gpu_response_trace import DEVICE, StandStill, make_env, report
from test_gpu_terrain_metrics import same_bits
from test_trunk_metrics import (ACCUMULATORS, REPO, SHAPES, STANDING_MARGIN_FP32_DEVIATION, STANDING_MARGIN_FP64, STANDING_STEPS, STANDING_WARMUP, TROT_SEGMENT,
                                TROT_STEPS, TROT_WARMUP, check_against_the_model, drive, set_down, trot_events, trot_with_pauses, trunk_groups, trunk_on)

pytestmark = pytest.mark.gpu


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPES)
def test_trunk_kernels_equal_the_model_bit_for_bit(N):
    groups = 3
    rng = np.random.default_rng(500 + N)                                 # the emulator test's script
    cfg, snaps, kind = T.scripted_steps(rng, N)
    group = trunk_groups(rng, N, groups)
    tm, B = trunk_on(DEVICE, cfg, N)
    res, acc = drive(tm, B, cfg, snaps, group, groups)
    check_against_the_model(res, acc, cfg, snaps, kind, group, groups, N)
    again = tm.read()                                                    # the reduction leaves what it reads as it is
    assert all(again[k].tobytes() == res[k].tobytes() for k in ("groups", "tilt_hist", "steps", "resets", "seg_anchor", "seg_command", "prev_lin_vel"))
    assert all(again["metrics"][m].tobytes() == res["metrics"][m].tobytes() for m in T.METRICS)


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def snapshot(env):
    """host copies of the buffers go1trunk_accumulate reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in T.INPUTS}


def test_trunk_through_the_environment():
    """80 steps of the trot script with pauses, the yaw command held at 0: the kernel's accumulators, state, histogram and tables equal
    the model replayed on the buffers read back after every step, bit for bit; the simulation is bit-identical with the measurement
    armed and not armed; every environment folded a step on three or more feet, one on exactly two and one closed segment; with the
    foot family armed beside it, the supporting feet are the four feet's contacts; and the accelerations telescope to the velocity
    difference."""
    N, GROUPS = 64, 3
    plain, env = make_env(N, "plane", 20.0, seed=4), make_env(N, "plane", 20.0, seed=4)
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    for e in (plain, env):
        e.reset()
    env.start_trunk_metrics(group, warmup_steps=TROT_WARMUP, segment_steps=TROT_SEGMENT)
    env.start_foot_metrics(group, warmup_steps=TROT_WARMUP)
    assert plain._trunk is None and plain._feet is None
    snaps = []
    for step in range(TROT_STEPS):
        action = trot_with_pauses(step, N).to(DEVICE)
        for e in (plain, env):
            e.commands[:, 2] = 0.0
            e.step(action)
        snaps.append(snapshot(env))
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, env.buffers.tensors[name]), (step, name)
    env.stop_trunk_metrics()
    env.stop_foot_metrics()
    res, feet = env.read_trunk_metrics(), env.read_foot_metrics()
    tm = env._trunk
    c = tm.cfg
    assert c.dt == np.float32(env.dt) and (c.num_envs, c.warmup_steps, c.num_groups, c.segment_steps) == (N, TROT_WARMUP, GROUPS, TROT_SEGMENT)
    assert c.tilt_limit == np.float32(0.25)
    cfg = T.config(dt=c.dt, tilt_limit=c.tilt_limit, segment_steps=TROT_SEGMENT, warmup_steps=TROT_WARMUP)
    st, formed = T.State(N), []
    for s in snaps:
        formed.append(T.accumulate(st, cfg, s))
    events = trot_events(st)
    print(f"\nper environment, the fewest steps on >= 3 feet {events[0].min()}, on 2 feet {events[1].min()}, closed segments {events[2].min()}; "
          f"resets {int(st.resets.sum())}, dropped {int(st.segments_dropped.sum())}, largest tilt {st.max[T.TILT].max():.3f}, "
          f"smallest margin {st.min[T.SUPPORT_MARGIN].min():.4f} m, largest |lateral drift| {np.abs(st.sum[T.LATERAL_DRIFT]).max():.4f} m")
    assert all((e >= 1).all() for e in events)                           # else the comparison below would assert nothing about the events
    for k in ACCUMULATORS:
        assert tm.acc[k].cpu().numpy().view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    for k in T.STATE:
        name = "env_" + k if k == "tilt_hist" else k
        assert res[name].view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    want, want_hist = T.reduce(st, group.numpy(), GROUPS)
    for m, name in enumerate(T.METRICS):
        assert res["metrics"][name].shape == (GROUPS, 6) and res["metrics"][name].tobytes() == np.ascontiguousarray(want[:, m]).tobytes(), name
    assert res["groups"].tobytes() == np.ascontiguousarray(want[:, 17, :4]).tobytes() and res["tilt_hist"].tobytes() == want_hist.tobytes()
    assert res["steps"].tolist() == [TROT_STEPS] * N and (res["tilt_hist"].sum(axis=1) == res["metrics"]["tilt"][:, 0]).all()
    assert res["env_max_tilt"].tobytes() == st.max[T.TILT].tobytes()

    # the foot family beside it, same warm-up: per environment the supporting feet summed over the steps are the four feet's contacts
    trunk_sum = tm.acc["sum"][T.SUPPORT_FEET].cpu().numpy()
    feet_sum = env._feet.acc["sum"].cpu().numpy().reshape(4, 12, N)[:, 0].sum(axis=0)
    assert (tm.acc["count"][T.SUPPORT_FEET].cpu().numpy() == env._feet.acc["count"].cpu().numpy().reshape(4, 12, N)[0, 0]).all()
    assert trunk_sum.tobytes() == feet_sum.tobytes() and trunk_sum.sum() > 0

    # the telescoping identity: dt x the sum of the accelerations is the velocity difference over the window, within two roundings per
    # sample; the vertical component from the kernel's own sums, the horizontal ones from the model's per-step values (bit-identical rows)
    dt = float(np.float32(env.dt))
    live = np.stack([f["live"] for f in formed])
    whole = (st.resets == 0) & live[TROT_WARMUP:].all(axis=0)
    assert whole.sum() >= N // 2
    first = live.argmax(axis=0)                                          # the first folded step: it sets the previous velocity and folds no acceleration
    assert (first[whole] == TROT_WARMUP - 1).all()                       # reset() took the episode's first step
    n = tm.acc["count"][T.ACCEL_VERTICAL].cpu().numpy().astype(np.float64)
    assert (n[whole] == TROT_STEPS - TROT_WARMUP).all()
    vel = np.stack([s["root_states"][7:10].astype(np.float64) for s in snaps])          # (steps, 3, N)
    dv = vel[-1] - vel[TROT_WARMUP - 1]
    low, high = tm.acc["min"][T.ACCEL_VERTICAL].cpu().numpy().astype(np.float64), tm.acc["max"][T.ACCEL_VERTICAL].cpu().numpy().astype(np.float64)
    sums = [np.sum([np.where(f["accel_valid"], f[k].astype(np.float64), 0.0) for f in formed], axis=0) for k in ("ax", "ay")] + [tm.acc["sum"][T.ACCEL_VERTICAL].cpu().numpy()]
    tops = [np.max([np.where(f["accel_valid"], np.abs(f[k].astype(np.float64)), 0.0) for f in formed], axis=0) for k in ("ax", "ay")] + [np.maximum(np.abs(low), np.abs(high))]
    for k, name in enumerate(("x", "y", "z")):
        gap = np.abs(dt * sums[k] - dv[k])[whole]
        bound = (n * 3.0 * 2.0 ** -24 * tops[k] * dt)[whole]
        print(f"telescoping {name}: largest gap {gap.max():.3e} m/s, its bound {bound[gap.argmax()]:.3e}, largest gap / bound {(gap / bound).max():.3f}")
        assert (gap <= bound).all(), name
    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_trunk_metrics()["steps"].tolist() == [TROT_STEPS] * N


def test_a_standing_robot_is_over_its_feet():
    """Zero actions on the plane, the robots set down at rest (test_trunk_metrics.set_down), N = 64, a 50-step warm-up, then 100 steps:
    four supporting feet on every folded step, and the mean support margin is the model's on the oracle's run of the same scenario
    (test_trunk_metrics.test_standing_robot_through_the_oracle: 0.156953 m) within max(2 d, 1 mm), d the deviation of the oracle's
    fp32 build from its fp64 build there (6.2e-9 m): the floor of 1 mm holds."""
    from test_foot_metrics import standing_env
    N = 64
    env = standing_env(N, DEVICE)
    env.reset()
    set_down(env)
    env.start_trunk_metrics(torch.zeros(N, dtype=torch.int32), warmup_steps=STANDING_WARMUP)
    for _ in range(STANDING_WARMUP + STANDING_STEPS):
        env.commands[:, 2] = 0.0
        env.step(torch.zeros(N, 12, device=DEVICE))
    env.stop_trunk_metrics()
    res = env.read_trunk_metrics()
    m = res["metrics"]
    assert res["resets"].sum() == 0 and m["tilt"][0, 0] == N * (STANDING_STEPS + 1)      # reset() took the first step of the episode
    allowance = max(2.0 * abs(STANDING_MARGIN_FP32_DEVIATION), 1e-3)
    print(f"\nmean support margin {m['support_margin'][0, 1]:.6f} m (smallest {m['support_margin'][0, 3]:.6f} m) against the oracle's "
          f"{STANDING_MARGIN_FP64:.6f} m: {m['support_margin'][0, 1] - STANDING_MARGIN_FP64:+.3e} m (allowance {allowance:.1e} m); supporting feet "
          f"{m['support_feet'][0, 1]:.4f} (fewest {m['support_feet'][0, 3]:.0f}), mean tilt {m['tilt'][0, 1]:.5f}")
    assert m["support_feet"][0, 1] == 4.0 and m["support_feet"][0, 3] == 4.0 and m["margin_negative"][0, 1] == 0.0
    assert abs(m["support_margin"][0, 1] - STANDING_MARGIN_FP64) <= allowance


# ---- 3. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_trunk_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    N, WINDOW, WARMUP, SEGMENT = 64, 30, 5, 8
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--trunk", "--vx", "0.5", "1.0", "--envs", str(N), "--steps", str(WINDOW),
                               "--warmup-steps", str(WARMUP), "--seed", "5", "--presets", "static_medium", "--terrain", "plane", "--segment-steps", str(SEGMENT)])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_trunk(a, StandStill(), dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits]))
    stem = tmp_path / "eval" / "static_medium"
    js = json.load(open(str(stem) + "_trunk.json"))
    md = open(str(stem) + "_trunk.md").read()
    print(md)
    assert open(str(stem) + "_tilt.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(str(stem) + "_tilt.png") > 5000
    assert [c["vx"] for c in js["cells"]] == [0.5, 1.0] and js["segment_steps"] == SEGMENT and js["tilt_limit"] == 0.25 and len(md.splitlines()) >= 2 + 2 + 2
    trunk = {m: np.array([[np.nan if x is None else x for x in cell] for cell in t]) for m, t in js["trunk"].items()}
    hist = np.array(js["tilt_hist"])
    assert hist.shape == (2, 16) and all(trunk[m].shape == (2, 6) for m in T.METRICS)
    groups = np.array(js["trunk_groups"])
    assert groups[:, 0].tolist() == [N / 2] * 2 and groups[:, 1].tolist() == [N / 2 * WINDOW] * 2
    # the sweep's reset() has already taken one step: window step k leaves episode_length_buf = k + 1, so steps WARMUP .. WINDOW fold
    assert (trunk["tilt"][:, 0] > 0).all() and (trunk["tilt"][:, 0] <= N / 2 * (WINDOW - WARMUP + 1)).all()
    assert hist.sum(axis=1).tolist() == trunk["tilt"][:, 0].tolist()                       # every folded step of a finite robot is one histogram sample
    assert sum(trunk[m][:, 5].sum() for m in T.METRICS) == 0                               # nothing non-finite in a standing robot
    assert (trunk["support_feet"][:, 0] == trunk["tilt"][:, 0]).all() and (trunk["support_feet"][:, 1] > 2.0).all() and (trunk["tilt"][:, 1] < 0.5).all()
    # the yaw command of the grid is 0: segments of 8 steps close, and a robot that stands falls behind what it is commanded
    assert (trunk["progress_err"][:, 0] > 0).all() and trunk["progress_err"][1, 1] < trunk["progress_err"][0, 1] < 0.0
    assert (trunk["accel_vertical"][:, 0] <= trunk["tilt"][:, 0]).all() and (trunk["accel_vertical"][:, 0] > 0).all()


# ---- 4. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_trunk_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_trunk_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_trunk_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_trunk_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].tolist() == [STEPS] * ENVS
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "trunk armed", "read"]
    lines = [f"Cost of the trunk measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  trunk armed: the same loop after start_trunk_metrics(): one go1trunk_accumulate launch more",
              "per step (1024 threads); its cost is the difference of the two columns.  read: read_trunk_metrics() (go1trunk_reduce over",
              "16 groups: 16 x 18 table rows and 16 histograms, and the device-to-host copies of the two tables, the per-environment",
              "histogram and the state arrays), events around the call."]
    report("trunk_metrics_cost.txt", "\n".join(lines))
