"""GPU checks of the observation family (include/go1obs.h, libgo1obs.so): the scripted buffers of the emulator test through the compiled
kernels against the model of tests/obs_ref.py bit for bit, the real environment under random actions with the observation noise on and
the model replayed on the obs_buf copies read back after every step, the simulation's indifference to an armed measurement, the
agreement with the scalar table's resets, the sweep through the tool (and a second sweep against the first one's JSON), and the recorded
cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (observation_metrics_cost.txt: the source of
profiles/observation_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import obs_ref as T
from test_gpu_response_trace import DEVICE, StandStill, make_env as plain_env, report
from test_gpu_terrain_metrics import same_bits
from test_observation_metrics import REPO, SCRIPTS, bits, check_against_the_model, drive, obs_groups, obs_on, same, same_as_the_model
from test_sensitivity_metrics import ROLL_CUT_STEP, ROLL_CUTS, ROLL_GROUPS, ROLL_N, ROLL_SEED, ROLL_STEPS, ROLL_WARMUP, make_env

pytestmark = pytest.mark.gpu


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,num_obs,num_priv,privileged", SCRIPTS)
def test_observation_kernels_equal_the_model_bit_for_bit(N, num_obs, num_priv, privileged):
    groups = 3
    rng = np.random.default_rng(1700 + N + num_obs)                      # the emulator test's script
    cfg, snaps, breaks, kind = T.scripted_steps(rng, N, num_obs, num_priv, privileged)
    group = obs_groups(rng, N, groups)
    family, B = obs_on(DEVICE, N, num_obs, num_priv)
    res, acc = drive(family, B, cfg, snaps, breaks, group, groups)
    check_against_the_model(res, acc, cfg, snaps, breaks, kind, group, groups, N)
    again = family.read()                                                # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ["groups", "hist", "tails"] + ["env_" + k for k in T.STATE])
    assert same(again["value"], res["value"]) and same(again["delta"], res["delta"])


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def test_observations_through_the_environment():
    """The protocol of test_sensitivity_metrics.py section 8 (64 environments, episodes of 1 s, the observation noise on, 120 steps of
    2.0 * randn actions from a seeded generator, four running environments reset from outside before step 60, a warm-up of 5), the scalar
    table and the family armed after reset().  The simulation is bit-identical with the measurement armed and not armed; the kernel's
    accumulators, state and three tables equal the model replayed on the obs_buf, privileged_obs_buf and reset_buf copies read back after
    every step, bit for bit; for every channel the bins, the two tails and the non-finite values add up to the measured env-steps; the
    group row's resets are the scalar table's terminated plus timed-out episodes plus the four outside resets.  The scalar table counts
    from the first step and the family from the sixth: that no environment resets inside the warm-up is a condition of that last
    comparison, asserted so.  MEASURED on an MI355X for this seed: 128 reset steps, none inside the warm-up (6 terminated, 122 timed
    out), 4 resets from outside; no value at the clip of 100; 6402 of 529920 values outside the default (placeholder) ranges; mean
    step-to-step change of gravity_x 0.0465."""
    from go1_gym_learn.eval_metrics import observations as O
    N, GROUPS = ROLL_N, ROLL_GROUPS
    plain, env = make_env(N, device=DEVICE), make_env(N, device=DEVICE)
    assert env.cfg.noise.add_noise
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    g = torch.Generator(device=DEVICE).manual_seed(ROLL_SEED)
    take = lambda: dict(obs_buf=env.obs_buf.cpu().numpy().copy(), privileged_obs_buf=env.privileged_obs_buf.cpu().numpy().copy(),
                        reset_buf=env.reset_buf.cpu().numpy().astype(np.uint8))

    def identical(what):
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, env.buffers.tensors[name]), (what, name)
    for e in (plain, env):
        e.reset()
    identical("reset")
    env.start_metrics(group, warmup_steps=ROLL_WARMUP)
    env.start_observation_metrics(group, warmup_steps=ROLL_WARMUP)
    assert plain._obs is None and plain._metrics is None
    snaps, breaks = [], {}
    for k in range(ROLL_STEPS):
        if k == ROLL_CUT_STEP:
            running = torch.nonzero(env.reset_buf == 0).reshape(-1)[:ROLL_CUTS]          # (a host read, once: not part of a measurement loop)
            assert running.numel() == ROLL_CUTS
            for e in (plain, env):
                e.reset_idx(running.clone())
            breaks[k] = running.cpu().tolist()
            identical(("outside", k))
        action = 2.0 * torch.randn(N, 12, device=DEVICE, generator=g)
        for e in (plain, env):
            e.step(action)
        snaps.append(take())
        identical(("step", k))
    env.stop_metrics()
    env.stop_observation_metrics()
    res, scalar = env.read_observation_metrics(), env.read_metrics()
    family = env._obs
    names, kinds = O.channel_names(env.cfg, True), O.channel_kinds(env.cfg, True)
    C = env.num_obs + env.num_privileged_obs
    assert res["channels"] == names and res["kinds"] == kinds and len(names) == C == family.channels
    cfg = T.config(O.channel_spans(env.cfg, names, kinds), env.num_obs, env.num_privileged_obs, True, warmup_steps=ROLL_WARMUP, clip=env.cfg.normalization.clip_observations)
    c = family.cfg
    assert (c.num_envs, c.warmup_steps, c.num_groups, c.num_obs, c.num_privileged_obs, c.privileged) == (N, ROLL_WARMUP, GROUPS, env.num_obs, env.num_privileged_obs, 1)
    assert bits(np.array(list(c.lo)[:C], np.float32)) == bits(cfg.lo) and bits(np.array(list(c.scale)[:C], np.float32)) == bits(cfg.scale) and c.clip == cfg.clip
    st, did = T.run(cfg, snaps, N, breaks)
    acc = {k: t.cpu().numpy() for k, t in family.acc.items()}
    same_as_the_model(res, acc, st, cfg, group.numpy(), GROUPS)
    # every measured value is in a bin, in a tail or not finite
    measured = res["groups"][:, 2]
    assert res["groups"][:, 0].tolist() == [22.0, 21.0, 21.0] and (res["groups"][:, 1] == ROLL_STEPS * res["groups"][:, 0]).all()
    assert (measured == (ROLL_STEPS - ROLL_WARMUP) * res["groups"][:, 0]).all()
    assert (res["hist"].sum(axis=2) + res["tails"][:, :, 0] + res["tails"][:, :, 1] + res["value"][:, :, 5] == measured[:, None]).all()
    assert (res["value"][:, :, 0] + res["value"][:, :, 5] == measured[:, None]).all()
    # the resets: the scalar table's, counted from the first step, plus those from outside
    early = int(sum((s["reset_buf"] != 0).sum() for s in snaps[:ROLL_WARMUP]))
    outside = np.bincount(group.numpy()[breaks[ROLL_CUT_STEP]], minlength=GROUPS)
    resets = int(sum((s["reset_buf"] != 0).sum() for s in snaps))
    noisy = res["delta"][:, names.index("gravity_x"), 1]
    print(f"\nMI355X: reset steps {resets} ({early} inside the warm-up), terminated {scalar['groups'][:, 2].sum():.0f}, timed out {scalar['groups'][:, 3].sum():.0f}, "
          f"outside {ROLL_CUTS}; values at the clip {res['tails'][:, :, 2].sum():.0f}, outside the default ranges {res['tails'][:, :, :2].sum():.0f} of "
          f"{measured.sum() * C:.0f}; mean step-to-step change of gravity_x {noisy.mean():.4f}")
    assert early == 0 and resets >= 64                                   # (the conditions of the comparison: every environment times out at least once)
    assert (res["groups"][:, 3] == scalar["groups"][:, 2] + scalar["groups"][:, 3] + outside).all()
    assert (res["delta"][:, :env.num_obs, 0] > 0).all() and (noisy > 0).all()         # the noise alone moves gravity_x from step to step
    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_observation_metrics()["env_launches"].tolist() == [ROLL_STEPS] * N
    with pytest.raises(ValueError, match="observations:"):
        env.start_observation_metrics(group, ranges={"grip": (0.0, 1.0)})
    wider = O.ranges_from(res)
    env.start_observation_metrics(group, ranges=wider, privileged=False)  # an earlier read's ranges; without the privileged columns
    env.step(torch.zeros(N, 12, device=DEVICE))
    with pytest.raises(RuntimeError, match="observations"):              # an armed family refuses a restore
        env.load_state(env.save_state())
    env.stop_observation_metrics()
    short = env.read_observation_metrics()
    assert short["value"].shape == (GROUPS, env.num_obs, 6) and short["channels"] == names[:env.num_obs] and list(wider) == names
    assert short["edges"][:, 0].tolist() == [float(np.float32(wider[n][0])) for n in short["channels"]] and (short["groups"][:, 2] == res["groups"][:, 0]).all()


# ---- 3. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_observation_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import observations as O, sweep
    N, WINDOW, WARMUP = 64, 30, 5
    argv = ["--checkpoint", "none", "--out", str(tmp_path), "--observations", "--vx", "0.5", "1.0", "--envs", str(N), "--steps", str(WINDOW), "--warmup-steps", str(WARMUP),
            "--seed", "5", "--terrain", "plane"]
    a = eval_sweep.parse_args(argv + ["--presets", "static_medium"])
    (tmp_path / "eval").mkdir()
    grid = dict(vx=a.vx, yaw=a.yaw, gait=[sweep.GAITS[g] for g in a.gaits])
    eval_sweep.run_observations(a, StandStill(), grid)
    stem = str(tmp_path / "eval" / "static_medium")
    js = json.load(open(stem + "_observations.json"))
    md = open(stem + "_observations.md").read()
    print(md)
    assert open(stem + "_observations.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(stem + "_observations.png") > 5000
    C = len(js["channels"])
    assert [c["vx"] for c in js["cells"]] == [0.5, 1.0] and C == 70 + 2 and js["kinds"].count("privileged") == 2 and js["shift"] is None and len(js["profiles"]) == 2
    assert [row[:3] for row in js["obs_groups"]] == [[N / 2, N / 2 * WINDOW, N / 2 * (WINDOW - WARMUP)]] * 2
    for p in js["profiles"]:
        total = np.array(p["hist"]).sum(axis=1) + np.array(p["below"]) + np.array(p["above"]) + np.array(p["nonfinite"])
        assert (total == N / 2 * (WINDOW - WARMUP)).all() and p["env_steps"] == N / 2 * (WINDOW - WARMUP)
    for kind in dict.fromkeys(js["kinds"]):
        assert md.count(f"| {kind} |") == 2, kind                         # a row per cell
    assert md.count("by the share outside the range") == 2
    zero = js["channels"].index("action_FL_hip")                          # the policy stands still: every action is 0
    assert js["min"][zero] == js["max"][zero] == 0.0 and js["delta_max"][zero] == 0.0
    # a second sweep, of the other preset, against the first one's JSON: its edges are taken over and every cell is compared with its own
    b = eval_sweep.parse_args(argv + ["--presets", "rand_large", "--against", stem + "_observations.json"])
    eval_sweep.run_observations(b, StandStill(), grid)
    stem2 = str(tmp_path / "eval" / "rand_large")
    js2 = json.load(open(stem2 + "_observations.json"))
    md2 = open(stem2 + "_observations.md").read()
    print(md2)
    assert js2["edges"] == js["edges"] and js2["channels"] == js["channels"] and len(js2["shift"]) == 2 and md2.count(": by js: ") == 2
    assert js2["shift"][0] == json.loads(json.dumps(sweep.clean(O.shift(js["profiles"][0], js2["profiles"][0]))))
    assert js2["shift"][0]["js"][zero] == 0.0 and all(x is None or 0.0 <= x <= 1.0 + 1e-12 for s in js2["shift"] for x in s["js"])
    assert open(stem2 + "_observations.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n"


# ---- 4. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_observation_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = plain_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()
    C = env.num_obs + env.num_privileged_obs

    def window(armed):
        if armed:
            env.start_observation_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_observation_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_observation_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["env_launches"].tolist() == [STEPS] * ENVS and len(res["channels"]) == C
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "observations armed", "read"]
    lines = [f"Cost of the observation measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device events",
             "around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>20}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>20.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", f"nothing armed: env.step() alone.  observations armed: the same loop after start_observation_metrics() with all {C} channels",
              f"({env.num_obs} observation and {env.num_privileged_obs} privileged columns): one go1obs_accumulate launch more per step ({C} x {ENVS} threads); its cost is the",
              "difference of the two columns.  read: read_observation_metrics() (go1obs_reduce over 16 groups: 16 x (2 C + 1) table rows,",
              "16 x C histograms and 16 x C tails, and the device-to-host copies of the three tables and the state arrays, about 84 B per",
              "channel and environment), events around the call."]
    report("observation_metrics_cost.txt", "\n".join(lines))
