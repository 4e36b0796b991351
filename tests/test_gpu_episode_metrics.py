"""GPU checks of the episode family (include/go1episode.h, libgo1episode.so): the scripted buffers of the emulator test through the
compiled kernels against the model of tests/episode_ref.py bit for bit, the real environment under random actions with the model
replayed on the buffers read back after every step, the simulation's indifference to an armed measurement, the agreement with the scalar
table's episode counts and with the simulator's own episode_sums, a standing robot, the sweep through the tool, and the recorded cost of
an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (episode_metrics_cost.txt: the source of
profiles/episode_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import episode_ref as T
from test_episode_metrics import (REPO, ROLL_BIN_STEPS, ROLL_CUT_STEP, ROLL_CUTS, ROLL_GAMMA, ROLL_GROUPS, ROLL_N, ROLL_STEPS, ROLL_WARMUP, SCRIPTS, assert_rollout_events,
                                  bits, check_against_the_model, drive, episode_groups, episodes_on, rollout_config, rollout_steps, same_as_the_model, snapshot,
                                  state_name)
from test_gpu_response_trace import DEVICE, StandStill, make_env, report
from test_gpu_terrain_metrics import same_bits

pytestmark = pytest.mark.gpu


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,bin_steps", SCRIPTS)
def test_episode_kernels_equal_the_model_bit_for_bit(N, bin_steps):
    groups = 3
    rng = np.random.default_rng(1200 + N)                                # the emulator test's script
    cfg, snaps, kind = T.scripted_steps(rng, N, bin_steps=bin_steps)
    group = episode_groups(rng, N, groups)
    ep, B = episodes_on(DEVICE, cfg, N)
    res, acc = drive(ep, B, cfg, snaps, group, groups)
    check_against_the_model(res, acc, cfg, snaps, kind, group, groups, N)
    again = ep.read()                                                    # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ["groups", "fall_hist", "timeout_hist", "open_hist"] + [state_name(k) for k in T.STATE])
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def test_episodes_through_the_environment():
    """The scenario of test_episode_metrics.py section 8 (64 environments, episodes of 1 s, 120 steps of random actions, four episodes cut
    by a reset_idx before step 60), the family and the scalar table armed before reset().  Falls, time-outs, whole closed episodes and the
    four cuts occur (asserted first, so that the comparison is not empty); the simulation is bit-identical with the measurement armed and
    not armed; the kernel's accumulators, state, histograms and tables equal the model replayed on the buffers read back after every
    step, bit for bit; on every step without a reset the family's running return is the simulator's episode_sums total, bit for bit; and
    the episodes closed are exactly the scalar table's terminated and timed-out ones.
    Counted first on the CPU with the oracle-backed environment of tests/fake_sim.py (the CPU generator's actions for the same seed;
    test_episode_metrics.test_the_rollout_script_produces_events_on_the_oracle): 2 falls, 126 time-outs, 128 closed of which 128 whole, 4 cuts, 0
    unseen, 64 open at the end.  MEASURED on an MI355X for this seed: 3 falls, 125 time-outs, 128 closed of which 128 whole, 4 cuts, 0 unseen,
    64 open at the end."""
    N, GROUPS = ROLL_N, ROLL_GROUPS
    plain, env = make_env(N, "plane", 1.0, seed=4), make_env(N, "plane", 1.0, seed=4)
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    env.start_metrics(group, warmup_steps=ROLL_WARMUP)
    env.start_episode_metrics(group, warmup_steps=ROLL_WARMUP, gamma=ROLL_GAMMA, bin_steps=ROLL_BIN_STEPS)
    assert plain._episodes is None and plain._metrics is None
    cfg = rollout_config(env)
    snaps = []
    for k in rollout_steps([plain, env]):
        s = snapshot(env)
        snaps.append(s)
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, env.buffers.tensors[name]), (k, name)
        running = s["reset_buf"] == 0
        ret = env._episodes.state["ret"].cpu().numpy()
        assert bits(ret[running]) == bits(s["episode_sums"][cfg.return_row][running]), k
    env.stop_metrics()
    env.stop_episode_metrics()
    res, scalar = env.read_episode_metrics(), env.read_metrics()
    ep = env._episodes
    c = ep.cfg
    assert (c.num_envs, c.warmup_steps, c.num_groups, c.return_row, c.bin_steps) == (N, ROLL_WARMUP, GROUPS, int(env.sim_config.num_rewards), ROLL_BIN_STEPS)
    assert c.gamma == np.float32(ROLL_GAMMA) and len(snaps) == ROLL_STEPS + 1
    st, did = T.run(cfg, snaps, N)
    assert_rollout_events(st, did, "MI355X")                             # else the comparison below would assert nothing about a close
    assert did[ROLL_CUT_STEP + 1]["cut"].sum() == ROLL_CUTS
    acc = {k: t.cpu().numpy() for k, t in ep.acc.items()}
    same_as_the_model(res, acc, st, cfg, group.numpy(), GROUPS)
    g = res["groups"]
    assert res["steps"].tolist() == [ROLL_STEPS + 1] * N and g[:, 5].tolist() == g[:, 0].tolist()          # every environment has an open episode
    assert (g[:, 2] == scalar["groups"][:, 2] + scalar["groups"][:, 3]).all() and g[:, 2].sum() == st.closed.sum()
    assert (g[:, 3] == scalar["groups"][:, 2]).all() and (g[:, 4] == scalar["groups"][:, 3]).all() and g[:, 7].sum() == 0
    assert (res["fall_hist"].sum(axis=1) == g[:, 3]).all() and (res["timeout_hist"].sum(axis=1) == g[:, 4]).all()
    assert (res["metrics"]["step_reward"][:, 0] == g[:, 1]).all() and (res["metrics"]["length"][:, 0] == g[:, 2]).all()
    assert (res["metrics"]["length"][:, 4] <= env.max_episode_length + 1).all()
    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_episode_metrics()["steps"].tolist() == [ROLL_STEPS + 1] * N
    with pytest.raises(RuntimeError, match="episodes"):                  # an armed family refuses a restore
        env.start_episode_metrics(group)
        env.load_state(env.save_state())
    env.stop_episode_metrics()


# ---- 3. a standing robot ----------------------------------------------------------------------------------------------------------------------
def test_a_standing_robot_survives():
    """Zero actions on the plane, the robots set down at rest (test_trunk_metrics.set_down), N = 64, 150 steps of a 20 s episode: no
    episode closes, every environment's episode is open, the open histogram holds them all, and the survival estimate is 1 wherever it
    is defined"""
    from go1_gym_learn.eval_metrics.episodes import kaplan_meier
    from test_foot_metrics import standing_env
    from test_trunk_metrics import set_down
    N, STEPS, BIN = 64, 150, 10
    env = standing_env(N, DEVICE)
    env.reset()
    set_down(env)
    env.start_episode_metrics(torch.zeros(N, dtype=torch.int32), warmup_steps=0, bin_steps=BIN)
    for _ in range(STEPS):
        env.step(torch.zeros(N, 12, device=DEVICE))
    env.stop_episode_metrics()
    res = env.read_episode_metrics()
    m = res["metrics"]
    # reset() took the first step of the episode before the start: the first sight is at episode_length_buf == 2, so no episode is whole
    assert res["groups"][0].tolist() == [N, N * STEPS, 0.0, 0.0, 0.0, N, 0.0, 0.0, N * (STEPS + 1)]
    assert (res["age"] == STEPS + 1).all() and not res["whole"].any() and (res["track_steps"] == STEPS).all()
    assert not res["fall_hist"].any() and not res["timeout_hist"].any() and res["open_hist"][0].tolist() == [0.0] * 15 + [float(N)]        # 151 / 10: clamped
    assert m["step_reward"][0, 0] == N * STEPS and m["step_reward"][0, 5] == 0 and all(m[k][0, 0] == 0 for k in T.METRICS[1:])
    assert bits(res["ret"]) == bits(env.buffers.episode_sums[int(env.sim_config.num_rewards)].cpu().numpy())
    s = kaplan_meier(res["fall_hist"], res["timeout_hist"], res["open_hist"])
    assert s.shape == (1, 16) and (s == 1.0).all()


# ---- 4. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_episode_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    N, WINDOW, WARMUP = 64, 30, 5
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--episodes", "--vx", "0.5", "1.0", "--envs", str(N), "--steps", str(WINDOW),
                               "--warmup-steps", str(WARMUP), "--seed", "5", "--presets", "static_medium", "--terrain", "plane"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_episodes(a, StandStill(), dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits]))
    stem = tmp_path / "eval" / "static_medium"
    js = json.load(open(str(stem) + "_episodes.json"))
    md = open(str(stem) + "_episodes.md").read()
    print(md)
    assert open(str(stem) + "_survival.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(str(stem) + "_survival.png") > 5000
    assert [c["vx"] for c in js["cells"]] == [0.5, 1.0] and js["bin_steps"] == 2 and js["gamma"] == 0.99 and js["group_fields"] == T.GROUP_FIELDS
    assert "| closed / open / cut |" in md and len(md.splitlines()) >= 2 + 2 + 2
    table = {m: np.array([[np.nan if x is None else x for x in cell] for cell in t]) for m, t in js["episodes"].items()}
    groups, survival = np.array(js["episode_groups"]), np.array([[np.nan if x is None else x for x in row] for row in js["survival"]])
    hists = {k: np.array(js[k]) for k in ("fall_hist", "timeout_hist", "open_hist")}
    assert sorted(table) == sorted(T.METRICS) and all(table[m].shape == (2, 6) for m in T.METRICS) and groups.shape == (2, 9) and survival.shape == (2, 16)
    assert all(h.shape == (2, 16) for h in hists.values()) and len(js["bin_edges"]) == 17 and js["bin_edges"][:3] == [0.0, 2.0, 4.0] and js["bin_edges"][-1] is None
    # both tables were armed before the sweep's reset(): one launch more than the window, every first episode whole, nothing cut or unseen
    assert groups[:, 0].tolist() == [N / 2] * 2 and groups[:, 1].tolist() == [N / 2 * (WINDOW + 1)] * 2 and groups[:, 6:8].sum() == 0
    assert (groups[:, 2] == groups[:, 3] + groups[:, 4]).all() and (groups[:, 5] == N / 2).all() and (hists["open_hist"].sum(axis=1) == N / 2).all()
    assert (table["step_reward"][:, 0] + table["step_reward"][:, 5] == groups[:, 1]).all() and (table["length"][:, 0] == groups[:, 2]).all()
    assert (table["discounted_return"][:, 0] + table["discounted_return"][:, 5] == groups[:, 2]).all()       # every closed episode was whole
    defined = ~np.isnan(survival)
    assert defined[:, 0].all() and ((survival[defined] >= 0.0) & (survival[defined] <= 1.0)).all() and len(js["summary"]) == 2


# ---- 5. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_episode_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_episode_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_episode_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_episode_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].tolist() == [STEPS] * ENVS
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "episodes armed", "read"]
    lines = [f"Cost of the episode measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  episodes armed: the same loop after start_episode_metrics(): one go1episode_accumulate launch",
              "more per step (1024 threads); its cost is the difference of the two columns.  read: read_episode_metrics() (go1episode_reduce over",
              "16 groups: 16 x 13 table rows and 16 x 3 histograms, and the device-to-host copies of the two tables, the per-environment",
              "histograms and the state arrays), events around the call."]
    report("episode_metrics_cost.txt", "\n".join(lines))
