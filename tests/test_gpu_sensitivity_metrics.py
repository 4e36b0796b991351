"""GPU checks of the sensitivity family (include/go1sens.h, libgo1sens.so): the scripted buffers of the emulator test through the compiled
kernels against the model of tests/sens_ref.py bit for bit, the real environment under random actions with every randomisation on and
the model replayed on the buffers read back after every step, the simulation's indifference to an armed measurement, the agreement with
the scalar table's falls, the sweep through the tool, and the recorded cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (sensitivity_metrics_cost.txt: the source of
profiles/sensitivity_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import sens_ref as T
from test_gpu_response_trace import DEVICE, StandStill, make_env as plain_env, report
from test_gpu_terrain_metrics import same_bits
from test_sensitivity_metrics import (REPO, ROLL_CUTS, ROLL_GROUPS, ROLL_N, ROLL_PAIR, ROLL_STEPS, ROLL_WARMUP, SCRIPTS, assert_rollout_events, bits,
                                      check_against_the_model, drive, make_env, replay, rollout_config, rollout_steps, same, same_as_the_model, sens_groups,
                                      sens_on, snapshot)

pytestmark = pytest.mark.gpu


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,pair", SCRIPTS)
def test_sensitivity_kernels_equal_the_model_bit_for_bit(N, pair):
    groups = 3
    rng = np.random.default_rng(1300 + N)                                # the emulator test's script
    cfg, first, snaps, outside, kind = T.scripted_steps(rng, N, pair=pair)
    group = sens_groups(rng, N, groups)
    family, B = sens_on(DEVICE, N)
    res, acc = drive(family, B, cfg, first, snaps, outside, group, groups)
    check_against_the_model(res, acc, cfg, first, snaps, outside, kind, group, groups, N)
    again = family.read()                                                # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ["groups", "counts"] + ["env_" + k for k in T.STATE])
    assert all(bits(again["curves"][q]) == bits(res["curves"][q]) for q in T.QUANTITIES) and all(same(again["value"][m], res["value"][m]) for m in T.PARAMETERS)
    assert (again["pair_map"] is None) == (not pair) and (not pair or bits(again["pair_map"]) == bits(res["pair_map"]))


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def test_sensitivity_through_the_environment():
    """The scenario of test_sensitivity_metrics.py section 8 (64 environments, episodes of 1 s, all seven randomisations on, the
    rigid-body parameters re-drawn after the start, everything re-drawn every 0.2 s, 120 steps of random actions, four environments reset
    from outside before step 60), the scalar table and the family armed after reset().  The simulation is bit-identical with the
    measurement armed and not armed; the kernel's accumulators, state and four tables equal the model replayed on the buffers read back
    after every step, bit for bit; for every parameter the steps over all bins plus the unbinned ones are the launches and the falls over
    all bins are the scalar table's terminated episodes.  Conditions, asserted so that the comparison is not empty: at least one fall,
    at least one fall charged to a bin other than the bin of the value the buffer holds after that step, at least 64 re-draws.
    Counted first on the CPU with the oracle-backed environment of tests/fake_sim.py (the CPU generator's actions for the same seed;
    test_sensitivity_metrics.test_the_rollout_script_produces_events_on_the_oracle): 7 falls, 121 time-outs, 60 falls charged to another
    bin than the buffer's (over the nine parameters), 6309 re-draws (701 of the friction).  MEASURED on an MI355X for this seed (the
    device generator's actions): 6 falls, 122 time-outs, 51 falls charged to another bin, 6300 re-draws (700 of the friction)."""
    N, GROUPS = ROLL_N, ROLL_GROUPS
    plain, env = make_env(N, device=DEVICE), make_env(N, device=DEVICE)
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    cfg = rollout_config(env)
    events = []
    for what, k in rollout_steps([plain, env]):
        events.append((what, snapshot(env)))
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, env.buffers.tensors[name]), (what, k, name)
        if what == "reset":
            env.start_metrics(group, warmup_steps=ROLL_WARMUP)
            env.start_sensitivity_metrics(group, warmup_steps=ROLL_WARMUP, pair=ROLL_PAIR)
            assert plain._sens is None and plain._metrics is None
    env.stop_metrics()
    env.stop_sensitivity_metrics()
    res, scalar = env.read_sensitivity_metrics(), env.read_metrics()
    family = env._sens
    c = family.cfg
    assert (c.num_envs, c.warmup_steps, c.num_groups, c.pair_a, c.pair_b) == (N, ROLL_WARMUP, GROUPS, 0, 6) and list(c.active) == [1] * 9
    assert bits(np.array(list(c.lo), np.float32)) == bits(cfg.lo) and bits(np.array(list(c.scale), np.float32)) == bits(cfg.scale)
    st, did, snaps = replay(cfg, events)
    assert len(did) == ROLL_STEPS and [what for what, _ in events].count("outside") == 1
    falls = assert_rollout_events(cfg, st, did, snaps, "MI355X")          # else the comparison below would assert nothing about a fall
    acc = {k: t.cpu().numpy() for k, t in family.acc.items()}
    same_as_the_model(res, acc, st, cfg, group.numpy(), GROUPS)
    curves, counts = res["curves"], res["counts"]
    assert res["groups"][:, 0].tolist() == [22.0, 21.0, 21.0] and (res["groups"][:, 1] == ROLL_STEPS * res["groups"][:, 0]).all()
    for p in range(T.P):
        assert (curves["steps"][:, p].sum(axis=1) + counts[:, p, 0] == res["groups"][:, 1]).all(), T.PARAMETERS[p]
        assert (curves["falls"][:, p].sum(axis=1) == scalar["groups"][:, 2]).all(), T.PARAMETERS[p]
        assert (curves["timeouts"][:, p].sum(axis=1) == scalar["groups"][:, 3]).all(), T.PARAMETERS[p]
    assert curves["falls"][:, 0].sum() == falls and res["pair_map"][:, 1].sum() == falls and (res["pair_map"][:, 0].sum(axis=(1, 2)) == res["groups"][:, 1]).all()
    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_sensitivity_metrics()["env_launches"].tolist() == [ROLL_STEPS] * N
    with pytest.raises(ValueError, match="sensitivity:"):
        env.start_sensitivity_metrics(group, ranges={"grip": (0.0, 1.0)})
    with pytest.raises(RuntimeError, match="sensitivity"):               # an armed family refuses a restore
        env.start_sensitivity_metrics(group)
        env.load_state(env.save_state())
    env.stop_sensitivity_metrics()


# ---- 3. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_sensitivity_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    N, WINDOW, WARMUP = 64, 30, 5
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--sensitivity", "--vx", "0.5", "1.0", "--envs", str(N), "--steps", str(WINDOW),
                               "--warmup-steps", str(WARMUP), "--seed", "5", "--presets", "rand_large", "--terrain", "plane", "--pair", "friction", "payload"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_sensitivity(a, StandStill(), dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits]))
    stem = tmp_path / "eval" / "rand_large"
    js = json.load(open(str(stem) + "_sensitivity.json"))
    md = open(str(stem) + "_sensitivity.md").read()
    print(md)
    assert open(str(stem) + "_sensitivity.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(str(stem) + "_sensitivity.png") > 5000
    active = T.PARAMETERS[:7]                                            # what rand_large randomises
    assert [c["vx"] for c in js["cells"]] == [0.5, 1.0] and js["reported"] == active and js["active"] == [True] * 7 + [False] * 2 and js["min_exposure"] == 200
    assert js["ranges"]["friction"] == [0.04, 6.0] and js["ranges"]["payload"] == [-1.5, 4.0] and js["pair"] == ["friction", "payload"]
    for name in active:
        assert md.count(f"| {name} |") == 2, name                        # a row per cell
    assert "| Kp_factor |" not in md and md.count("by effect on the hazard") == 2
    steps, counts, groups = np.array(js["curves"]["steps"]), np.array(js["counts"]), np.array(js["sens_groups"])
    assert steps.shape == (2, 9, 16) and groups.tolist() == [[N / 2, N / 2 * WINDOW]] * 2 and np.array(js["pair_map"]).shape == (2, 4, 8, 8)
    assert (steps[:, :7].sum(axis=2) + counts[:, :7, 0] == N / 2 * WINDOW).all() and not steps[:, 7:].any()
    value = js["value"]["friction"]
    assert value[0][0] == N / 2 * WINDOW and 0.0399 <= value[0][3] <= value[0][4] <= 6.0001         # (the bounds are rounded to fp32)


# ---- 4. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_sensitivity_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = plain_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    ranges = {name: None for name in T.PARAMETERS}                       # all nine, over the configuration's ranges
    env.reset()

    def window(armed):
        if armed:
            env.start_sensitivity_metrics(group, warmup_steps=0, ranges=ranges, pair=("friction", "motor_strength"))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_sensitivity_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_sensitivity_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["env_launches"].tolist() == [STEPS] * ENVS and res["active"].all()
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "sensitivity armed", "read"]
    lines = [f"Cost of the sensitivity measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  sensitivity armed: the same loop after start_sensitivity_metrics() with all nine parameters",
              "and a pair: one go1sens_accumulate launch more per step (10 x 1024 threads); its cost is the difference of the two columns.",
              "read: read_sensitivity_metrics() (go1sens_reduce over 16 groups: 16 x 10 table rows, 16 x 9 curves, 16 x 9 counts and 16 x 4",
              "pair-map parts, and the device-to-host copies of the four tables and the state arrays, about 8.5 KB per environment),",
              "events around the call."]
    report("sensitivity_metrics_cost.txt", "\n".join(lines))
