"""GPU checks of terrain traversal (include/go1eval.h, fifth kernel family): the scripted buffers of the emulator test through
libgo1eval.so against the model of tests/terrain_ref.py bit for bit, the simulation's indifference to an armed measurement, the
four statuses through the real environment with the model replayed on the buffers read back after every step, the terrain sweep
end to end, and the recorded cost of an armed step.

Reports: with GO1_EVAL_REPORT_DIR set, the cost table is also written there (terrain_sweep_cost.txt: the source of
profiles/terrain_sweep_cost.txt); it is always printed."""
import numpy as np
import pytest
import torch

import terrain_ref as T
from test_gpu_response_trace import DEVICE, StandStill, report
from test_terrain_metrics import check_against_the_model, drive, scripted_groups, terrain_on

pytestmark = pytest.mark.gpu
# The smallest tile on which every generator of Terrain.make_terrain still lays what it is written to lay: its flat 3 m platform in
# the middle and at least one ring of features around it (a stair tread is 0.31 m: 3 + 2 * 0.31 = 3.62 m, the next multiple of the
# 0.1 m sample pitch that is a whole number of metres).  Smaller tiles are accepted too, and are platform only.
TILE = 4.0


def same_bits(a, b):
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


# ---- 1. the kernels on the scripted buffers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 300])                                 # one ragged block; a full block and a ragged one
def test_terrain_kernels_equal_the_model_bit_for_bit(N):
    groups = 4
    rng = np.random.default_rng(100 + N)                                 # the emulator test's script
    geo, snaps, kind = T.scripted_steps(rng, N)
    group = scripted_groups(rng, N, groups)
    ter, B = terrain_on(DEVICE, geo, N)
    res, acc = drive(ter, B, geo, snaps, group, groups)
    check_against_the_model(res, acc, geo, snaps, kind, group, groups, N)
    again = ter.read()                                                   # the reduction leaves what it reads as it is
    assert all(again[k].tobytes() == res[k].tobytes() for k in T.STATE + ["groups"])
    assert all(again["metrics"][m].tobytes() == res["metrics"][m].tobytes() for m in T.METRICS)


# ---- 2. the real environment --------------------------------------------------------------------------------------------------------------
def make_env(N, seed=3, rows=2, cols=2, tile=TILE):
    """the training configuration on a trimesh curriculum grid of rows x cols tiles with the height scan; the spawn height is the
    tile's centre patch, so that a robot on a pit-shaped tile is not dropped from the rim's height"""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    c = apply_train_config(make_cfg(), num_envs=N)
    t = c.terrain
    t.mesh_type, t.curriculum, t.center_robots, t.terrain_proportions = "trimesh", True, False, [0.1, 0.1, 0.35, 0.25, 0.2]
    t.num_rows, t.num_cols, t.terrain_length, t.terrain_width, t.border_size = rows, cols, tile, tile, 5.0
    t.min_init_terrain_level, t.max_init_terrain_level = 0, rows - 1
    t.origin_height_source = "centre_patch"
    t.measure_heights = True                                             # the terminal body height is then taken above the ground, not above z = 0
    torch.manual_seed(seed)
    np.random.seed(seed)
    return VelocityTrackingEasyEnv(sim_device=DEVICE, headless=True, cfg=c)


def test_arming_writes_nothing_of_the_simulators():
    N, STEPS = 16, 30
    plain, armed = make_env(N), make_env(N)
    for e in (plain, armed):
        e.reset()                                                        # the first episode begins: a measurement covers it alone
    assert armed.buffers.height_samples is not None and armed.sim_config.hf_wall_units > 0
    armed.start_terrain_metrics(torch.arange(N) % 4, warmup_steps=3)
    assert plain._traversal is None
    action = torch.zeros(N, 12, device=DEVICE)
    for step in range(STEPS):
        plain.step(action)
        armed.step(action)
        # episode_log is no state: the step kernel adds the finished episodes' sums to it with fp32 atomicAdd
        for name, t in plain.buffers.tensors.items():
            if isinstance(t, torch.Tensor) and name != "episode_log":
                assert same_bits(t, armed.buffers.tensors[name]), (step, name)
    assert torch.allclose(plain.buffers.episode_log, armed.buffers.episode_log, rtol=1e-5, atol=1e-6)
    armed.stop_terrain_metrics()
    res = armed.read_terrain_metrics()
    assert res["steps"].max() == STEPS and res["groups"][:, 0].tolist() == [4.0] * 4
    armed.step(action)                                                   # disarmed: no further launch
    assert armed.read_terrain_metrics()["steps"].max() == STEPS


def snapshot(env):
    """host copies of the buffers go1eval_terrain_accumulate reads, as they stand after a step"""
    return {k: getattr(env.buffers, k).cpu().numpy().copy() for k in T.INPUTS if k != "height_samples"}


def test_statuses_through_the_environment():
    N, BEFORE, AFTER, MOVED, TURNED = 16, 5, 30, 0, 5
    env = make_env(N)
    cells = torch.arange(N) % 4                                          # cell = level * 2 + type
    env.place_on_terrain(cells // 2, cells % 2)
    assert env.terrain_levels.tolist() == (cells // 2).tolist() and env.terrain_types.tolist() == (cells % 2).tolist()
    origins = env.cfg.terrain.terrain_origins[cells // 2, cells % 2].to(DEVICE)
    assert torch.equal(env.buffers.env_origins.t(), origins)
    assert (env.root_states[:, 0:2] - origins[:, 0:2]).abs().max() <= env.cfg.terrain.x_init_range + 1e-5      # respawned on the new tiles
    S = env.sim_config
    geo = T.geometry(hf_hscale=S.hf_hscale, hf_vscale=S.hf_vscale, hf_border=S.hf_border, tile_length=TILE, tile_width=TILE, dt=env.dt, warmup_steps=2,
                     penalised_body_mask=int(S.penalised_body_mask), height_samples=env.buffers.height_samples.cpu().numpy())
    env.start_terrain_metrics(cells, warmup_steps=geo.warmup_steps)
    action = torch.zeros(N, 12, device=DEVICE)
    snaps = []
    for step in range(BEFORE + AFTER):
        if step == BEFORE:
            moved = env.root_states[MOVED].clone()
            moved[0] += TILE                                             # one tile further along x: onto the level-1 tile behind it
            env.set_idx_pose([MOVED], None, moved.unsqueeze(0))
            turned = env.root_states[TURNED].clone()
            turned[3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0])             # half a turn about x: upside down
            env.set_idx_pose([TURNED], None, turned.unsqueeze(0))
        env.step(action)
        snaps.append(snapshot(env))
    env.stop_terrain_metrics()
    res = env.read_terrain_metrics()
    status, steps, end = res["status"], res["steps"], res["end_step"]
    print(f"\nstatuses {status.tolist()}, steps {steps.tolist()}, end steps {end.tolist()}")
    assert status[MOVED] == T.TRAVERSED and end[MOVED] == BEFORE + 1 == steps[MOVED]         # at the step after the move
    assert status[TURNED] == T.FELL and BEFORE + 1 <= end[TURNED] == steps[TURNED] + 1         # once its episode ended
    rest = np.array([e for e in range(N) if e not in (MOVED, TURNED)])
    assert (status[rest] == T.RUNNING).all() and (end[rest] == 0).all() and (steps[rest] == BEFORE + AFTER).all()
    for g in (2, 3):                                                     # cells with untouched robots only: nothing is decided
        assert res["outcomes"]["traversed"][g].tolist()[0] == 0.0 and np.isnan(res["outcomes"]["traversed"][g, 1:5]).all()
        assert res["outcomes"]["traversed"][g, 5] == 4.0 and res["groups"][g].tolist()[:5] == [4.0, 4.0, 0.0, 0.0, 0.0] and np.isnan(res["groups"][g, 5])
    assert res["groups"][0].tolist() == [4.0, 3.0, 1.0, 0.0, 0.0, 1.0] and res["groups"][1].tolist() == [4.0, 3.0, 0.0, 1.0, 0.0, 0.0]
    # the model on the buffers read back after each step: every accumulator, every state word and the table
    st = T.run(geo, snaps, N)
    for k, t in env._traversal.acc.items():
        assert t.cpu().numpy().view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    for k in T.STATE:
        assert res[k].view(getattr(st, k).dtype).tobytes() == getattr(st, k).tobytes(), k
    want = T.reduce(st, cells.numpy(), 4, geo.dt)
    for m, name in enumerate(T.METRICS):
        assert res["metrics"][name].tobytes() == want[:, m].tobytes(), name
    for o, name in enumerate(T.OUTCOMES):
        assert res["outcomes"][name].tobytes() == want[:, T.M + o].tobytes(), name
    assert res["groups"].tobytes() == want[:, -1].tobytes()
    quiet = int(rest[0])
    assert st.count[:, quiet].tolist()[0] == BEFORE + AFTER - geo.warmup_steps and st.count[T.STUMBLE, quiet] == st.count[T.BASE_HEIGHT, quiet]
    assert 0.1 < st.min[T.BASE_HEIGHT, quiet] <= st.max[T.BASE_HEIGHT, quiet] < 0.6         # a Go1 standing on the ground it is over


# ---- 3. the sweep end to end ------------------------------------------------------------------------------------------------------------------
def test_terrain_sweep_end_to_end(monkeypatch):
    from go1_gym_learn.eval_metrics import sweep, terrain
    built = []
    build = sweep.build_eval_env
    monkeypatch.setattr(sweep, "build_eval_env", lambda *a, **kw: built.append(build(*a, **kw)) or built[-1])
    N, WINDOW, WARMUP = 32, 40, 5
    res = terrain.run_terrain_sweep(StandStill(), "static_medium", vx=0.0, num_envs=N, window=WINDOW, warmup=WARMUP, seed=5, num_rows=2, num_cols=2,
                                    terrain_length=TILE, terrain_width=TILE)
    assert res["cells"] == [(0, 0), (0, 1), (1, 0), (1, 1)] and res["terrain_type"] == ["slope_down", "stairs_down"] * 2
    assert res["difficulty"] == [0.0, 0.0, 0.5, 0.5] and res["tile"] == (TILE, TILE)
    assert sorted(res["metrics"]) == sorted(T.METRICS) and sorted(res["outcomes"]) == sorted(T.OUTCOMES)
    assert all(res["metrics"][m].shape == (4, 6) for m in T.METRICS) and all(res["outcomes"][o].shape == (4, 6) for o in T.OUTCOMES)
    g = res["groups"]
    assert g.shape == (4, 6) and g[:, 0].tolist() == [8.0] * 4 and (g[:, 1:5].sum(axis=1) == g[:, 0]).all() and g[:, 0].sum() == N
    assert res["status"].shape == (N,) and (res["steps"] <= WINDOW).all() and (res["steps"][res["status"] == T.RUNNING] == WINDOW).all()
    print("\n" + terrain.terrain_markdown_grid(res))
    # the mean base_height_terrain between the two ends the configuration allows: a base lying on the tile's lowest ground while
    # the sample under it reads the tile's highest (below), and the spawn height, origin z + base_init_state z, over the tile's lowest
    # sample (above)
    env, cfg = built[0]
    t, field = cfg.terrain, env.env.terrain.heightsamples
    init_z = float(env.env.base_init_state[2])
    px = int(TILE / t.horizontal_scale)
    for cell, (level, kind) in enumerate(res["cells"]):
        tile = field[t.border + level * px:t.border + (level + 1) * px, t.border + kind * px:t.border + (kind + 1) * px].astype(np.float64) * t.vertical_scale
        low, high = tile.min() - tile.max(), float(t.env_origins[level, kind, 2]) + init_z - tile.min()
        row = res["metrics"]["base_height_terrain"][cell]
        print(f"cell {cell}: base_height_terrain mean {row[1]:.4f} (min {row[3]:.4f}, max {row[4]:.4f}) in [{low:.3f}, {high:.3f}], count {row[0]:.0f}")
        assert row[0] > 0 and low <= row[1] <= high, (cell, row.tolist(), low, high)    # (the mean: a reset also draws a base velocity of up to 0.5 m/s, so single steps may lie a centimetre above the spawn height)


# ---- 4. the cost ----------------------------------------------------------------------------------------------------------------------------
def test_terrain_cost_is_recorded():
    """no time is asserted: the two configurations are timed in alternation and the table is printed (and written where
    GO1_EVAL_REPORT_DIR says)"""
    ENVS, STEPS, REPS = 1024, 150, 2
    env = make_env(ENVS, seed=5, rows=4, cols=4, tile=8.0)
    group = torch.arange(ENVS, dtype=torch.int32) % 16
    action = torch.zeros(ENVS, 12, device=DEVICE)
    env.reset()

    def window(armed):
        if armed:
            env.start_terrain_metrics(group, warmup_steps=0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(STEPS):
            env.step(action)
        b.record()
        torch.cuda.synchronize()
        if armed:
            env.stop_terrain_metrics()
        return a.elapsed_time(b) * 1000.0 / STEPS

    def read():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = env.read_terrain_metrics()
        b.record()
        torch.cuda.synchronize()
        assert res["groups"][:, 0].sum() == ENVS and res["steps"].max() == STEPS      # robots were measured through the whole window
        return a.elapsed_time(b) * 1000.0
    window(False), window(True), read()                                  # warm: every kernel and every allocation size once
    rows = [[window(False), window(True), read()] for _ in range(REPS)]
    assert all(x > 0 for row in rows for x in row)
    names = ["nothing armed", "terrain armed", "read"]
    lines = [f"Cost of the terrain-traversal measurement, one MI355X, {ENVS} environments on a 4 x 4 grid of 8 m trimesh tiles, zero actions, {STEPS} steps",
             "per window, device events around the step loop, warm, the two windows in alternation.", "MEASURED; microseconds per step for the two windows,",
             "microseconds per call for the read.", "", f"{'rep':>4}" + "".join(f"{n:>18}" for n in names)]
    lines += [f"{r + 1:>4}" + "".join(f"{x:>18.1f}" for x in row) for r, row in enumerate(rows)]
    lines += ["", "nothing armed: env.step() alone.  terrain armed: the same loop after start_terrain_metrics(): one go1eval_terrain_accumulate launch",
              "more per step; its cost is the difference of the two columns.  read: read_terrain_metrics() (go1eval_terrain_reduce over 16 groups,",
              "the device-to-host copies of the table and the four state arrays), events around the call."]
    report("terrain_sweep_cost.txt", "\n".join(lines))
