"""GPU checks of the state library (include/go1state.h, libgo1state.so) and of LeggedRobot.save_state / load_state: the scripted buffers of the
emulator test through the compiled kernels against the model of tests/state_ref.py, a replay of the real environment with forced events, a
load across ring phases, a branch of one robot into 64 environments, the simulation's indifference to saves, the paired push sweep through
the tool, and the recorded cost.  Every comparison is bit for bit.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (sim_state_cost.txt: the source of profiles/sim_state_cost.txt); it
is always printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_response_trace import DEVICE, report
from test_sim_state import (check_host_surface, check_scripted, differing, host_copy, logical_copy, make_env, replay, same, scripted_actions,
                            window)

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def G():
    import go1state_host
    return go1state_host


# ---- 1. the compiled kernels on the scripted buffers -------------------------------------------------------------------------------------------
# 1: one thread; 64: one wavefront; 257: two tiles per row with a ragged one; 600: three.  Both row pitches (7: the 4-byte path, 70: the 8-byte
# one) at every size; the ring lengths alternate
@pytest.mark.parametrize("N,num_obs,lag,hist", [(1, 7, 0, 1), (1, 70, 6, 30), (64, 7, 6, 30), (64, 70, 0, 1), (257, 7, 0, 30), (257, 70, 6, 1),
                                                (600, 7, 6, 1), (600, 70, 6, 30)])
def test_state_kernels_equal_the_model_bit_for_bit(N, num_obs, lag, hist):
    check_scripted(N, num_obs, lag, hist, None, DEVICE)


# ---- 2. replay -------------------------------------------------------------------------------------------------------------------------------------
def tile_grid(c):
    """the train configuration's tile grid as a trimesh terrain with the height scan (the recipe of tests/test_gpu_terrain_metrics.py)"""
    t = c.terrain
    t.mesh_type, t.curriculum, t.center_robots, t.terrain_proportions = "trimesh", True, False, [0.1, 0.1, 0.35, 0.25, 0.2]
    t.num_rows, t.num_cols, t.terrain_length, t.terrain_width, t.border_size = 2, 2, 8.0, 8.0, 5.0
    t.min_init_terrain_level, t.max_init_terrain_level = 0, 1
    t.measure_heights = True


@pytest.mark.parametrize("N,terrain", [(64, "plane"), (40, "trimesh")])
def test_replay_on_the_environment(N, terrain):
    """30 steps, the forced events (a time-out, a command resampling, a training push inside the window), save, 40 scripted steps, load, the
    same 40 steps: every tensor but episode_log, the rings in logical order and the history window have the same bits at every step"""
    env = make_env(N, DEVICE, tile_grid if terrain == "trimesh" else None, seed=4)
    base = env.env
    assert (base.buffers.height_samples is not None) == (terrain == "trimesh") and base.sim_config.add_noise and base.sim_config.push_robots
    env.reset()
    for a in scripted_actions(30, N, DEVICE, seed=200):
        env.step(a)
    state, first = replay(env, 40)
    assert state.whole and state.num_rows == N and state.device.type == "cuda"
    resets = sum(int(f[0]["reset_buf"].sum()) for f in first)
    print(f"\nreplay, {N} environments on the {terrain}: {resets} resets in the 40 steps; a state of {state.nbytes} bytes ({state.layout['bytes_per_env']} per environment)")
    assert int(base._state.skipped.cpu()) == 0


# ---- 3. across ring phases -----------------------------------------------------------------------------------------------------------------------
def test_load_across_ring_phases():
    """a second environment of the same configuration and seed has taken 3 steps more, so both rings stand elsewhere; it loads the first's whole
    state and both take the same 20 steps"""
    N = 64
    a, b = make_env(N, DEVICE, seed=6), make_env(N, DEVICE, seed=6)
    for env, steps in ((a, 30), (b, 33)):
        env.reset()
        for act in scripted_actions(steps, N, DEVICE, seed=300):
            env.step(act)
    ha, hb = a.env.sim.counters()[1], b.env.sim.counters()[1]
    assert a.env.sim.history_window_offset() != b.env.sim.history_window_offset() and ha != hb
    b.env.load_state(a.env.save_state())
    assert b.env.sim.counters() == (a.env.sim.counters()[0], hb) and b.env.common_step_counter == a.env.common_step_counter
    per_env, g = set(G().PER_ENV) - {"lag_buffer", "obs_history"}, G()
    for i, act in enumerate([None] + scripted_actions(20, N, DEVICE, seed=400)):
        if act is not None:
            a.step(act), b.step(act)
        raw_a, raw_b = host_copy(a.env.buffers), host_copy(b.env.buffers)
        assert [k for k in per_env if not same(raw_a[k], raw_b[k])] == [], i                  # every other per-environment tensor as it lies
        assert not same(raw_a["obs_history"], raw_b["obs_history"])                           # (the rings do stand elsewhere)
        assert differing(logical_copy(a.env), logical_copy(b.env), skip=("episode_log",)) == [], i      # the rings in logical order, the globals
        assert same(window(a), window(b)), i
    assert g.GLOBAL[3] == "episode_log"


# ---- 4. branch ---------------------------------------------------------------------------------------------------------------------------------------
def quiet(c):
    """no noise, no randomisation on a cadence, no pushes: what an environment draws depends on its index"""
    c.noise.add_noise = False
    d = c.domain_rand
    d.push_robots = d.randomize_gravity = False
    for k in ("randomize_friction", "randomize_restitution", "randomize_base_mass", "randomize_com_displacement", "randomize_motor_strength",
              "randomize_motor_offset", "randomize_Kp_factor", "randomize_Kd_factor", "randomize_rigids_after_start"):
        setattr(d, k, False)


def test_branch_one_robot_into_all():
    from test_foot_metrics import trot_action
    N, SRC = 64, 5
    env = make_env(N, DEVICE, quiet, seed=7)
    base = env.env
    S = base.sim_config
    assert not S.add_noise and not S.push_robots and S.resample_interval > 60 and S.max_episode_length > 60
    env.reset()
    for step in range(30):
        env.step(trot_action(step, N).to(DEVICE))
    assert int(base.buffers.episode_length_buf.min()) == 31                                   # nobody fell during the trot
    counter = base.common_step_counter
    base.load_state(base.save_state([SRC]), env_ids=list(range(N)), rows=[0] * N)
    assert base.common_step_counter == counter                                                # a branch: the clock stays
    row = trot_action(0, N)[SRC:SRC + 1].repeat(N, 1).to(DEVICE)
    for step in range(21):
        if step:
            env.step(row)
            assert int(base.buffers.reset_buf.sum()) == 0, step
        c = host_copy(base.buffers)
        for k, kind in G().PER_ENV.items():
            a = c[k] if kind in ("rows", "history") else c[k].reshape(-1, N).T
            assert all(same(a[e], a[SRC]) for e in range(N)), (step, k)
    assert same(window(env)[0], window(env)[SRC])
    assert float(base.root_states[:, :2].std(dim=0).max()) == 0.0                             # env_origins is copied: one place


# ---- 5. indifference -----------------------------------------------------------------------------------------------------------------------------------
def test_saving_changes_nothing():
    N = 64
    plain, saved = make_env(N, DEVICE, seed=8), make_env(N, DEVICE, seed=8)
    for env in (plain, saved):
        env.reset()
    before = host_copy(saved.env.buffers)
    saved.env.save_state(), saved.env.save_state([3, 1])
    assert differing(host_copy(saved.env.buffers), before) == [] and plain.env._state is None
    for i, act in enumerate(scripted_actions(30, N, DEVICE, seed=500)):
        plain.step(act), saved.step(act)
        saved.env.save_state() if i % 2 else saved.env.save_state([i % N, 0])
        assert differing(host_copy(plain.env.buffers), host_copy(saved.env.buffers), skip=("episode_log",)) == [], i
    assert "go1state_host" in sys.modules


def test_host_surface_on_the_device(tmp_path):
    env = make_env(16, DEVICE, seed=9)
    env.reset()
    env.step(torch.zeros(16, 12, device=DEVICE))
    check_host_surface(env, tmp_path)
    state = env.env.save_state()
    with pytest.raises(RuntimeError, match=r"move it with \.to\(\)"):
        env.env.load_state(state.cpu())
    env.env.start_trunk_metrics(torch.zeros(16, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="refused while trunk is armed"):
        env.env.load_state(state)
    env.env.stop_trunk_metrics()
    env.env.load_state(state)


# ---- 6. the paired sweep through the tool ---------------------------------------------------------------------------------------------------------------
def test_paired_push_sweep_through_the_tool(tmp_path, capsys):
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    from scripts.train_config import apply_train_config
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    N = 64
    c = apply_train_config(make_cfg(), num_envs=N).env
    torch.manual_seed(0)
    policy = ActorCritic(c.num_observations, c.num_privileged_obs, c.num_observations * c.num_observation_history, c.num_actions).to(DEVICE).eval()
    a = eval_sweep.parse_args(["--checkpoint", "none", "--out", str(tmp_path), "--push", "--paired", "--magnitude", "0", "1.0", "--direction", "0", "90",
                               "--envs", str(N), "--seed", "5", "--presets", "static_medium", "--terrain", "plane"])
    (tmp_path / "eval").mkdir()
    eval_sweep.run_push(a, policy)
    stem = str(tmp_path / "eval" / "static_medium")
    js = json.load(open(stem + "_push.json"))
    md = open(stem + "_push.md").read()
    print(md)
    assert "paired excess peak error [m/s]" in md and js["paired"] and js["source"] == (np.arange(N) // 4).tolist()
    ex = js["paired_excess"]
    assert len(ex) == 4 and js["cells"][0] == dict(magnitude=0.0, direction_deg=0.0)
    control_ok = int(ex[0][2])
    assert 0 <= control_ok <= N // 4 and all(int(row[2]) <= control_ok for row in ex)
    assert ex[0][:2] == ([0.0, 0.0] if control_ok else [None, None])                          # the control against itself: exactly 0
    print(f"paired excess (mean, std, sources): {ex}; status counts {js['status_counts']}")


# ---- 7. the cost -----------------------------------------------------------------------------------------------------------------------------------------
def test_state_cost_is_recorded():
    """no time is asserted: every column is timed with device events around 20 repetitions after a warm-up, two samples per column in
    alternation, and the table is printed (and written where GO1_EVAL_REPORT_DIR says)"""
    import go1sim_host as H
    ENVS, REPS, SAMPLES = 1024, 20, 2
    env = make_env(ENVS, DEVICE, seed=5)
    base = env.env
    env.reset()
    for _ in range(10):
        env.step(torch.zeros(ENVS, 12, device=DEVICE))
    whole, few_ids = base.save_state(), list(range(8))
    few = base.save_state(few_ids)
    clone = base.buffers.clone_to(DEVICE)

    def copy_back():
        for k, t in clone.tensors.items():
            if t is not None:
                base.buffers.tensors[k].copy_(t)
    columns = [("save all", lambda: base.save_state()), ("load all", lambda: base.load_state(whole)),
               ("save 8", lambda: base.save_state(few_ids)), ("load 8", lambda: base.load_state(few, env_ids=few_ids)),
               ("clone_to", lambda: base.buffers.clone_to(DEVICE)), ("copy_ back", copy_back)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / REPS
    for _, fn in columns:
        timed(fn)                                                                             # warm: every kernel and allocation size once
    rows = [[timed(fn) for _, fn in columns] for _ in range(SAMPLES)]
    assert all(x > 0 for row in rows for x in row)
    L = whole.layout
    tensors = sum(t is not None for t in clone.tensors.values())
    lines = [f"Cost of saving and loading the simulator's state, one MI355X, {ENVS} environments of the train configuration on the plane,",
             f"device events around {REPS} back-to-back calls, warm, the columns in alternation.  MEASURED; microseconds per call, host-side",
             "launch overhead included (the calls are enqueued back to back: a column is the larger of the device time and the host's enqueue time).",
             f"A state is {L['bytes_per_env']} bytes per environment ({whole.nbytes} bytes for all, {few.nbytes} for 8), {4 * L['global_words']} of them global.", "",
             f"{'sample':>6}" + "".join(f"{n:>14}" for n, _ in columns)]
    lines += [f"{r + 1:>6}" + "".join(f"{x:>14.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "save all / load all: save_state() / load_state(state) of every environment: one launch of the gather or scatter kernel and one for the",
              "global section; a save also allocates the snapshot's four tensors (zeroed).  save 8 / load 8: the same for eight environments",
              "named by the host (their ids are checked and uploaded in the call), without the global section.",
              f"clone_to / copy_ back: what the tree offered before: SimBuffers.clone_to(device) (a copy of all {tensors} tensors, one launch each or more) and",
              "a per-tensor copy_ back into the simulator's buffers.  These copy whole tensors, cannot name environments, and keep the rings' phase."]
    report("sim_state_cost.txt", "\n".join(lines))
