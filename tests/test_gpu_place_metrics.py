"""GPU checks of the foot-placement family (include/go1place.h, libgo1place.so): the scripted buffers of the emulator test through the
compiled kernels against the model of tests/place_ref.py bit for bit, the real environment under a scripted trot with the model replayed
on the buffers read back after every step, the behaviour table's raibert_heuristic against the model's errors on the same steps, the
refusal of a restore while the family is armed, the sweep through the tool, and the recorded cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (placement_metrics_cost.txt: the source of
profiles/placement_metrics_cost.txt); it is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import place_ref as T
from test_gpu_response_trace import DEVICE, StandStill, make_env, report
from test_place_metrics import (REPO, SHAPES, TROT_STEPS, TROT_WARMUP, assert_trot_events, bits, check_against_the_model, drive, place_groups, place_on, same_as_the_model,
                                state_name)

pytestmark = pytest.mark.gpu
RAIBERT = 4                                                               # the behaviour table's row raibert_heuristic (enum Go1BehaviourMetric)


# ---- 1. the compiled kernels on the scripted buffers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SHAPES)
def test_place_kernels_equal_the_model_bit_for_bit(N):
    groups = 3
    rng = np.random.default_rng(1100 + N)                                # the emulator test's script
    cfg, snaps, kind = T.scripted_steps(rng, N)
    group = place_groups(rng, N, groups)
    pm, B = place_on(DEVICE, cfg, N)
    res, acc = drive(pm, B, cfg, snaps, group, groups)
    check_against_the_model(res, acc, cfg, snaps, kind, group, groups, N)
    again = pm.read()                                                    # the reduction leaves what it reads as it is
    assert all(bits(again[k]) == bits(res[k]) for k in ["groups", "map"] + [state_name(k) for k in T.STATE])
    assert all(bits(again["metrics"][m]) == bits(res["metrics"][m]) for m in T.METRICS)


# ---- 2. the real environment ------------------------------------------------------------------------------------------------------------------
def snapshot(env):
    """host copies of the buffers go1place_accumulate reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in T.INPUTS}


def raibert_of(values):
    """the behaviour table's raibert_heuristic of one step from the model's errors: per environment ex * ex and ey * ey (fp32 products) of
    the four feet in the feet's order added in an fp64 carry, rounded to fp32 once"""
    carry = np.zeros(values["ex"].shape[1])
    with np.errstate(all="ignore"):
        for f in range(4):
            carry = carry + (values["ex"][f] * values["ex"][f]).astype(np.float64)
            carry = carry + (values["ey"][f] * values["ey"][f]).astype(np.float64)
        return carry.astype(np.float32)


def test_placement_through_the_environment():
    """100 steps of the foot family's trot script with the placement table and the behaviour table armed: every foot of every environment
    touches down twice, closes a stride and folds a stance sweep, with no reset (asserted first, so that the comparison is not empty); the
    kernel's accumulators, state, map and tables equal the model replayed on the buffers read back after every step, bit for bit; the
    behaviour table's raibert_heuristic accumulators equal the model's ex * ex + ey * ey folded over the same steps, bit for bit; a step
    after the stop launches nothing; and an armed family refuses a restore."""
    from test_foot_metrics import trot_action
    N, GROUPS = 64, 3
    env = make_env(N, "plane", 20.0, seed=4)
    group = (torch.arange(N) % GROUPS).to(torch.int32)
    env.reset()
    env.start_placement_metrics(group, warmup_steps=TROT_WARMUP)
    env.start_metrics(group, warmup_steps=TROT_WARMUP, behaviour=True)
    snaps = []
    for step in range(TROT_STEPS):
        env.step(trot_action(step, N).to(DEVICE))
        snaps.append(snapshot(env))
    env.stop_placement_metrics()
    env.stop_metrics()
    res = env.read_placement_metrics()
    pm = env._place
    c = pm.cfg
    assert (c.num_envs, c.warmup_steps, c.num_groups, c.num_commands) == (N, TROT_WARMUP, GROUPS, int(env.sim_config.num_commands)) and c.map_cell == np.float32(0.03)
    cfg = T.config(warmup_steps=TROT_WARMUP, num_commands=c.num_commands, map_cell=0.03)
    st, did = T.run(cfg, snaps, N)
    assert_trot_events(st, "MI355X")                                     # else the comparison below would assert nothing about the events
    acc = {k: t.cpu().numpy() for k, t in pm.acc.items()}
    same_as_the_model(res, acc, st, group.numpy(), GROUPS)
    assert res["steps"].tolist() == [TROT_STEPS] * N and res["groups"][:, 2].sum() == 0
    assert res["map"].sum() + res["groups"][:, 5].sum() == res["groups"][:, 3].sum() == st.touchdowns.sum()

    # the behaviour table beside it, same warm-up, so the same steps are excluded by both: its raibert_heuristic row is the fold of the
    # model's errors, bit for bit
    fold = T.State(N)
    for d in did:
        fold.fold(0, d["live"], raibert_of(d["values"]))
    behaviour = {k: t.cpu().numpy()[RAIBERT] for k, t in env._behaviour.acc.items()}
    assert fold.count[0].sum() > 0 and (fold.count[0] == TROT_STEPS - TROT_WARMUP + 1).all()          # reset() took the first step of the episode
    for k in ("count", "nonfinite", "sum", "sumsq", "min", "max"):
        assert bits(behaviour[k].view(getattr(fold, k).dtype)) == bits(getattr(fold, k)[0]), k
    assert fold.nonfinite[0].sum() == 0 and fold.sum[0].min() > 0

    env.step(torch.zeros(N, 12, device=DEVICE))                          # disarmed: no further launch
    assert env.read_placement_metrics()["steps"].tolist() == [TROT_STEPS] * N
    with pytest.raises(RuntimeError, match="placement"):                 # an armed family refuses a restore
        env.start_placement_metrics(group)
        env.load_state(env.save_state())
    env.stop_placement_metrics()
    env.load_state(env.save_state())                                     # and a stopped one does not


# ---- 3. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_placement_sweep_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    N, WINDOW, WARMUP = 64, 30, 5
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--placement", "--axis", "stance_width", "0.1", "0.45", "--envs", str(N),
                               "--steps", str(WINDOW), "--warmup-steps", str(WARMUP), "--seed", "5", "--presets", "static_medium", "--terrain", "plane"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_placement(a, StandStill(), eval_sweep.behaviour_axes(a))
    stem = tmp_path / "eval" / "static_medium"
    js = json.load(open(str(stem) + "_placement.json"))
    md = open(str(stem) + "_placement.md").read()
    print(md)
    assert open(str(stem) + "_footprints.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(str(stem) + "_footprints.png") > 5000
    assert js["cells"] == [dict(stance_width=0.1), dict(stance_width=0.45)] and [c["width"] for c in js["commanded"]] == pytest.approx([0.1, 0.45])
    assert len(md.splitlines()) >= 2 + 2 + 2 * 4 and "| 0.45 | RR |" in md
    table = {m: np.array([[[np.nan if x is None else x for x in foot] for foot in cell] for cell in t]) for m, t in js["placement"].items()}
    groups, cells = np.array(js["placement_groups"]), np.array(js["map"])
    assert cells.shape == (2, 4, 8, 8) and all(table[m].shape == (2, 4, 6) for m in T.METRICS)
    assert groups[:, 0].tolist() == [N / 2] * 2 and groups[:, 1].tolist() == [N / 2 * WINDOW] * 2
    # the sweep's reset() has already taken one step: window step k leaves episode_length_buf = k + 1, so steps WARMUP .. WINDOW fold
    folded = table["stance_err_x"][:, :, 0] + table["swing_err_x"][:, :, 0] + table["stance_err_x"][:, :, 5] + table["swing_err_x"][:, :, 5]
    assert (folded > 0).all() and (folded <= N / 2 * (WINDOW - WARMUP + 1)).all()
    assert (cells.sum(axis=(1, 2, 3)) + groups[:, 5] == groups[:, 3]).all()
    assert np.array(js["foot_counts"]["touchdowns"]).sum(axis=1).tolist() == groups[:, 3].tolist()
    # the feet of a robot that stands on its default pose are nearer their nominal points under the narrow command than under the wide one
    # or the other way round, but not equally far: the commanded width moves the nominal point by 0.175 m
    assert not np.allclose(table["stance_err_y"][0, :, 1], table["stance_err_y"][1, :, 1], atol=0.05, equal_nan=True)


# ---- 4. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_place_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, "plane", 20.0, seed=5)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_placement_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_placement_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_placement_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].tolist() == [STEPS] * ENVS
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "placement armed", "read"]
    lines = [f"Cost of the foot-placement measurement, one MI355X, {ENVS} environments on the plane, zero actions, {STEPS} steps per window, device",
             "events around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  placement armed: the same loop after start_placement_metrics(): one go1place_accumulate launch",
              "more per step (4 x 1024 threads); its cost is the difference of the two columns.  read: read_placement_metrics() (go1place_reduce",
              "over 16 groups: 16 x 57 table rows and 16 x 16 map workgroups, and the device-to-host copies of the two tables, the",
              "per-environment maps and the state arrays), events around the call."]
    report("placement_metrics_cost.txt", "\n".join(lines))
