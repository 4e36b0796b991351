"""GPU checks of the gait family (include/go1gait.h, libgo1gait.so): the scripted buffers of the emulator test through the compiled
kernels against the model of tests/gait_ref.py bit for bit, the real environment under a scripted trot with the model replayed on the
buffers read back after every step, the simulation's indifference to an armed measurement, the agreement with the foot family's contact
counts, a standing robot, the sweep through the tool, and the recorded cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (gait_metrics_cost.txt: the source of
profiles/gait_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import gait_ref as T
from test_gait_metrics import (ACCUMULATORS, REPO, SHAPES, TROT_STEPS, TROT_WARMUP, assert_trot_events, bits, check_against_the_model, drive, gait_groups, gait_on,
                               same_as_the_model)
from test_gpu_response_trace import DEVICE, StandStill, make_env, report
from test_gpu_terrain_metrics import same_bits

pytestmark = pytest.mark.gpu


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPES)
def test_gait_kernels_equal_the_model_bit_for_bit(N):
    groups = 3
    rng = np.random.default_rng(900 + N)                                 # the emulator test's script
    cfg, snaps, kind = T.scripted_steps(rng, N)
    group = gait_groups(rng, N, groups)
    gm, B = gait_on(DEVICE, cfg, N)
    res, acc = drive(gm, B, cfg, snaps, group, groups)
    check_against_the_model(res, acc, cfg, snaps, kind, group, groups, N)
    again = gm.read()                                                    # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ("groups", "support_hist", "phase_hist", "env_support_hist", "env_phase_hist", "last_td", "td_count",
                                                        "ref_steps", "prev_contact", "steps", "resets", "strides", "strides_dropped"))
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def snapshot(env):
    """host copies of the buffers go1gait_accumulate reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in T.INPUTS}


def test_gait_through_the_environment():
    """80 steps of the foot family's trot script: the simulation is bit-identical with the measurement armed and not armed; every
    environment closes a reference stride and one in which all three other feet touched down, and the diagonal pairs move together more
    than the others (asserted first, so that the comparison is not empty); the kernel's accumulators, state, histograms and tables equal
    the model replayed on the buffers read back after every step, bit for bit; with the foot family armed beside it the support
    patterns that hold a foot add up to that foot's contact count; and a step after the stop launches nothing."""
    from test_foot_metrics import trot_action
    N, GROUPS = 64, 3
    plain, env = make_env(N, "plane", 20.0, seed=4), make_env(N, "plane", 20.0, seed=4)
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    for e in (plain, env):
        e.reset()
    env.start_gait_metrics(group, warmup_steps=TROT_WARMUP, min_stride_steps=1, max_stride_steps=100)
    env.start_foot_metrics(group, warmup_steps=TROT_WARMUP)
    assert plain._gait is None and plain._feet is None
    snaps = []
    for step in range(TROT_STEPS):
        action = trot_action(step, N).to(DEVICE)
        for e in (plain, env):
            e.step(action)
        snaps.append(snapshot(env))
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, env.buffers.tensors[name]), (step, name)
    env.stop_gait_metrics()
    env.stop_foot_metrics()
    res, feet = env.read_gait_metrics(), env.read_foot_metrics()
    gm = env._gait
    c = gm.cfg
    assert (c.num_envs, c.warmup_steps, c.num_groups, c.min_stride_steps, c.max_stride_steps) == (N, TROT_WARMUP, GROUPS, 1, 100)
    cfg = T.config(warmup_steps=TROT_WARMUP, min_stride_steps=1, max_stride_steps=100)
    st, did = T.run(cfg, snaps, N)
    assert_trot_events(st, did, "MI355X")                                # else the comparison below would assert nothing about the strides
    acc = {k: t.cpu().numpy() for k, t in gm.acc.items()}
    same_as_the_model(res, acc, st, group.numpy(), GROUPS)
    assert res["steps"].tolist() == [TROT_STEPS] * N and (res["support_hist"].sum(axis=1) == res["metrics"]["sync_FL_FR"][:, 0]).all()
    assert (res["phase_hist"].sum(axis=2) == np.stack([res["metrics"][f"phase_err_{leg}"][:, [0, 5]].sum(axis=1) for leg in ("FR", "RL", "RR")], axis=1)).all()

    # the foot family beside it, same warm-up: per foot and environment the steps in the support patterns that hold the foot are the foot's
    # contact steps, out of as many folded steps
    support = res["env_support_hist"].view(np.uint32).astype(np.int64)   # (16, N)
    feet_acc = {k: env._feet.acc[k].cpu().numpy().reshape(4, 12, N)[:, 0] for k in ("sum", "count")}          # row 0 of a foot: contact
    for f in range(4):
        with_foot = support[[m for m in range(16) if m >> f & 1]].sum(axis=0)
        assert (with_foot == feet_acc["sum"][f]).all() and with_foot.sum() > 0, f
        assert (support.sum(axis=0) == feet_acc["count"][f].view(np.uint32)).all(), f
    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_gait_metrics()["steps"].tolist() == [TROT_STEPS] * N
    with pytest.raises(RuntimeError, match="gait"):                      # an armed family refuses a restore
        env.start_gait_metrics(group)
        env.load_state(env.save_state())
    env.stop_gait_metrics()


# ---- 3. a standing robot ----------------------------------------------------------------------------------------------------------------------
def test_a_standing_robot_has_no_gait():
    """Zero actions on the plane, the robots set down at rest (test_trunk_metrics.set_down), N = 64, a 50-step warm-up, then 100 steps:
    every folded step is on four feet, every pair is in step on every one of them, no stride is ever opened, and the class is "none\""""
    from go1_gym_learn.eval_metrics import gait
    from test_foot_metrics import standing_env
    from test_trunk_metrics import STANDING_STEPS, STANDING_WARMUP, set_down
    N = 64
    env = standing_env(N, DEVICE)
    env.reset()
    set_down(env)
    env.start_gait_metrics(torch.zeros(N, dtype=torch.int32), warmup_steps=STANDING_WARMUP)
    for _ in range(STANDING_WARMUP + STANDING_STEPS):
        env.step(torch.zeros(N, 12, device=DEVICE))
    env.stop_gait_metrics()
    res = env.read_gait_metrics()
    m = res["metrics"]
    folded = N * (STANDING_STEPS + 1)                                    # reset() took the first step of the episode
    assert res["resets"].sum() == 0 and res["support_hist"][0].tolist() == [0.0] * 15 + [float(folded)]
    for i, j in T.PAIRS:
        assert m[f"sync_{T.FEET[i]}_{T.FEET[j]}"][0].tolist() == [float(folded), 1.0, 0.0, 1.0, 1.0, 0.0]
    assert res["groups"][0].tolist() == [N, N * (STANDING_WARMUP + STANDING_STEPS), 0.0, 0.0, 0.0] and res["strides"].sum() == 0 and (res["ref_steps"] == -1).all()
    assert not res["phase_hist"].any() and all(m[f"touchdowns_{leg}"][0, 0] == 0 for leg in ("FR", "RL", "RR"))
    name, distance = gait.classify([gait.circular_stats(res["phase_hist"][0, k])[0] for k in range(3)])
    assert name == "none" and np.isnan(distance)


# ---- 4. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_gait_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    N, WINDOW, WARMUP = 64, 30, 5
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--coordination", "--vx", "0.5", "--gaits", "trotting", "pacing", "--envs", str(N),
                               "--steps", str(WINDOW), "--warmup-steps", str(WARMUP), "--seed", "5", "--presets", "static_medium", "--terrain", "plane"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_gait(a, StandStill(), dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits]))
    stem = tmp_path / "eval" / "static_medium"
    js = json.load(open(str(stem) + "_gait.json"))
    md = open(str(stem) + "_gait.md").read()
    print(md)
    assert open(str(stem) + "_gait.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(str(stem) + "_gait.png") > 5000
    assert [c["gait_name"] for c in js["cells"]] == ["trotting", "pacing"] and [c["gait"] for c in js["cells"]] == [[0.5, 0.0, 0.0], [0.0, 0.0, 0.5]]
    assert [s["commanded_gait"] for s in js["summary"]] == ["trotting", "pacing"] and [s["commanded"] for s in js["summary"]] == [[0.5, 0.5, 0.0], [0.5, 0.0, 0.5]]
    assert "| trotting |" in md and "| pacing |" in md and len(md.splitlines()) >= 2 + 2 + 2
    table = {m: np.array([[np.nan if x is None else x for x in cell] for cell in t]) for m, t in js["gait"].items()}
    support, phase, groups = np.array(js["support_hist"]), np.array(js["phase_hist"]), np.array(js["gait_groups"])
    assert support.shape == (2, 16) and phase.shape == (2, 3, 16) and all(table[m].shape == (2, 6) for m in T.METRICS)
    assert groups[:, 0].tolist() == [N / 2] * 2 and groups[:, 1].tolist() == [N / 2 * WINDOW] * 2
    # the sweep's reset() has already taken one step: window step k leaves episode_length_buf = k + 1, so steps WARMUP .. WINDOW fold
    assert (table["sync_FL_RR"][:, 0] > 0).all() and (table["sync_FL_RR"][:, 0] <= N / 2 * (WINDOW - WARMUP + 1)).all()
    for pair in T.METRICS[:6]:
        assert support.sum(axis=1).tolist() == table[pair][:, 0].tolist(), pair            # every folded step is one support-pattern sample
    assert sum(table[m][:, 5].sum() for m in T.METRICS) == 0                               # nothing non-finite
    assert (phase.sum(axis=2) <= groups[:, 3:4]).all()


# ---- 5. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_gait_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_gait_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_gait_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_gait_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].tolist() == [STEPS] * ENVS
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "gait armed", "read"]
    lines = [f"Cost of the gait measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  gait armed: the same loop after start_gait_metrics(): one go1gait_accumulate launch more",
              "per step (1024 threads); its cost is the difference of the two columns.  read: read_gait_metrics() (go1gait_reduce over",
              "16 groups: 16 x 16 table rows and 16 x 4 histograms, and the device-to-host copies of the two tables, the per-environment",
              "histograms and the state arrays), events around the call."]
    report("gait_metrics_cost.txt", "\n".join(lines))
