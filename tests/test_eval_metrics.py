"""CPU checks of the policy-evaluation feature: the C-ABI surface and stamp of libgo1eval (include/go1eval.h,
walk-these-ways_amd/csrc/go1eval.hip), the reference's metric functions and DR presets against fixtures produced by executing
the reference (tests/golden/gen_eval_metrics.py), the fp64 model of the two kernels (tests/eval_ref.py) on hand-computable
cases, the kernel source itself under the SIMT emulator against that model, and the environment hooks where there is no GPU."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import eval_ref as E
from util import build_emu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(REPO, "include", "go1eval.h")
GOLDEN = os.path.join(REPO, "tests", "golden")


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(go1eval_\w+)\s*\(", src)))


def exported_symbols(path):
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


# ---- 1. the library ------------------------------------------------------------------------------------------------------------
def test_eval_library_exports_what_the_header_declares_with_the_source_stamp():
    import __graft_entry__ as g
    import go1eval_host
    path = g.build_eval_hip()
    assert path == go1eval_host.LIB_PATH
    assert declared_functions() == sorted(go1eval_host.EXPORTED_SYMBOLS)
    assert sorted(s for s in exported_symbols(path) if s.startswith("go1eval")) == declared_functions()
    want = g.source_hash(g.eval_sources(), g.EVAL_FLAGS)
    assert g.library_stamp(path) == want
    lib = go1eval_host.load_library()
    v = lib.go1eval_version()
    assert b"gfx950" in v and (g.STAMP + want.encode()) in v
    # argument validation happens before any launch: callable without a GPU
    cfg, buf = go1eval_host.Go1EvalConfig(), go1eval_host.Go1EvalBuffers()
    for fn in (lib.go1eval_clear, lib.go1eval_accumulate, lib.go1eval_reduce):
        assert fn(None, None, None) == -1
        assert fn(ctypes.byref(cfg), ctypes.byref(buf), None) == -1        # num_envs = 0
    cfg.num_envs = 8
    assert lib.go1eval_accumulate(ctypes.byref(cfg), ctypes.byref(buf), None) == -2     # no accumulators


def test_eval_library_is_separate_from_the_other_libraries():
    import __graft_entry__ as g
    names = {os.path.basename(f) for f in g.sim_sources() + g.ppo_sources() + g.render_sources()}
    assert not names & {"go1eval.hip", "go1eval.h", "go1_tables.h"}
    assert {os.path.basename(f) for f in g.eval_sources()} == {"go1eval.hip", "go1eval.h", "go1_tables.h"}


def test_missing_eval_library_fails_loudly(tmp_path):
    import go1eval_host
    with pytest.raises(go1eval_host.Go1EvalLibraryMissing, match="no CPU fallback"):
        go1eval_host.load_library(str(tmp_path / "missing.so"))


def test_host_mirror_matches_the_header():
    import go1eval_host as G
    src = open(HEADER).read()
    assert f"#define GO1EVAL_NUM_METRICS {G.NUM_METRICS}" in src and f"#define GO1EVAL_NUM_FIELDS {G.NUM_FIELDS}" in src
    assert f"#define GO1EVAL_REDUCE_THREADS {G.REDUCE_THREADS}" in src and G.REDUCE_THREADS == E.REDUCE_THREADS
    body = src[src.index("typedef struct Go1EvalBuffers"):src.index("} Go1EvalBuffers;")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in G.Go1EvalBuffers._fields_]
    body = src[src.index("typedef struct Go1EvalConfig"):src.index("} Go1EvalConfig;")]
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in G.Go1EvalConfig._fields_]
    enum = src[src.index("enum Go1EvalMetric"):src.index("};", src.index("enum Go1EvalMetric"))]
    order = [n for n, _ in sorted(re.findall(r"GO1EVAL_(\w+) = (\d+)", enum), key=lambda p: int(p[1]))]
    assert [n.lower() for n in order] == [n.lower() for n in G.METRIC_NAMES] == [n.lower() for n in E.METRICS]
    assert G.FIELD_NAMES == E.FIELDS and G.GROUP_FIELD_NAMES == E.GROUP_FIELDS
    from go1_gym_learn.eval_metrics.metrics import SCALAR_METRICS
    from go1_gym.envs.base.legged_robot import LeggedRobot
    assert SCALAR_METRICS == G.METRIC_NAMES and G.DEFAULT_BODY_MASS == LeggedRobot.default_body_mass


# ---- 2. the reference's metric functions ---------------------------------------------------------------------------------------
def _fixture_env(z, seed):
    env = types.SimpleNamespace(default_body_mass=4.801)
    for k in ("base_lin_vel", "base_ang_vel", "commands", "root_states", "torques", "dof_vel", "payloads", "reset_buf", "time_out_buf",
              "episode_length_buf"):
        setattr(env, k, torch.from_numpy(z[f"s{seed}_in_{k}"]))
    key = f"s{seed}_in_measured_heights"
    env.measured_heights = torch.from_numpy(z[key]) if key in z.files else 0
    return env


def test_metric_names_are_the_references():
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS
    with open(os.path.join(GOLDEN, "eval_metric_names.json")) as f:
        names = json.load(f)
    assert len(names) == 14 and sorted(METRICS_FNS) == names


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scalar_metrics_equal_the_references_bit_for_bit(seed):
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS, SCALAR_METRICS
    z = np.load(os.path.join(GOLDEN, "eval_metrics.npz"))
    env = _fixture_env(z, seed)
    assert isinstance(env.measured_heights, int) == (seed == 1)
    nonfinite = 0
    for name in SCALAR_METRICS:
        got = METRICS_FNS[name](env, None, None)
        want = z[f"s{seed}_out_{name}"]
        assert got.shape == (256,) and got.numpy().dtype == want.dtype == (np.bool_ if name == "termination" else np.float32), name
        assert got.numpy().tobytes() == want.tobytes(), name          # bits: infinities and NaNs included
        nonfinite += int((~np.isfinite(want.astype(np.float64))).sum())
    assert nonfinite > 0                                              # the fixture holds robots that stand still


def test_network_metrics_go_through_the_policy_modules():
    from go1_gym_learn.eval_metrics.metrics import METRICS_FNS
    torch.manual_seed(0)
    ac = types.SimpleNamespace(adaptation_module=torch.nn.Linear(6, 3), env_factor_encoder=torch.nn.Linear(4, 3))
    obs = {"obs_history": torch.randn(5, 6), "privileged_obs": torch.randn(5, 4)}
    with torch.no_grad():
        want = ((ac.adaptation_module(obs["obs_history"]) - ac.env_factor_encoder(obs["privileged_obs"])) ** 2).mean(dim=1)
        assert torch.equal(METRICS_FNS["adaptation_loss"](None, ac, obs), want)
        assert np.array_equal(METRICS_FNS["latents"](None, ac, obs), ac.env_factor_encoder(obs["privileged_obs"]).numpy())
    assert METRICS_FNS["adaptation_loss"](None, object(), obs) is None
    assert np.array_equal(METRICS_FNS["privileged_obs"](None, None, obs), obs["privileged_obs"].numpy())
    # the reference returns after the first reward term
    env = types.SimpleNamespace(reward_names=["a", "b"], reward_scales={"a": 2.0, "b": 3.0},
                                reward_functions=[lambda: torch.ones(4), lambda: torch.ones(4)])
    r = METRICS_FNS["auxiliary_rewards"](env, None, None)
    assert list(r) == ["a"] and torch.equal(r["a"], 2.0 * torch.ones(4))


# ---- 3. the DR presets -----------------------------------------------------------------------------------------------------------
def _leaves(cfg):
    import inspect
    out = {}
    for sec in dir(cfg):
        node = getattr(cfg, sec)
        if sec.startswith("_") or not inspect.isclass(node):
            continue
        for k in dir(node):
            v = getattr(node, k)
            if k.startswith("_") or callable(v):
                continue
            out[f"{sec}.{k}"] = list(v) if isinstance(v, tuple) else v
    return out


@pytest.mark.parametrize("name", ["base_set", "rand_regular", "rand_large", "static_low", "static_medium", "static_high", "only_base_mass"])
def test_presets_write_the_references_fields(name):
    import go1sim_host as H
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym_learn.eval_metrics import domain_randomization as DR
    from scripts.train_config import apply_train_config
    with open(os.path.join(GOLDEN, "eval_dr_settings.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(["base_set"] + list(DR.DR_SETTINGS))
    fn = DR.base_set if name == "base_set" else DR.DR_SETTINGS[name]
    cfg = make_cfg()
    before = _leaves(cfg)
    fn(cfg)
    after = _leaves(cfg)
    changed = {k: v for k, v in after.items() if k not in before or before[k] != v}
    assert changed == want[name]
    if name == "static_low":
        assert cfg.domain_rand.motor_strength_range == [0.9, -0.99]          # the reference's value, kept
    # the simulator's host accepts the configuration a sweep builds from it, and the ranges reach the device configuration
    cfg = apply_train_config(make_cfg(), num_envs=64)
    DR.base_set(cfg)
    if name != "base_set":
        fn(cfg)
    S, _ = H.build_sim_config(cfg, seed=1)
    assert int(S.teleport_robots) == 1 and int(S.use_terminal_body_height) == 1
    for field in ("friction_range", "restitution_range", "added_mass_range", "com_displacement_range", "motor_strength_range"):
        assert np.allclose(list(getattr(S, field))[:2], getattr(cfg.domain_rand, field)), field


def test_presets_default_to_the_module_level_cfg():
    from go1_gym.envs.base import legged_robot_config as LC
    from go1_gym_learn.eval_metrics import domain_randomization as DR
    saved = {k: getattr(LC.Cfg.domain_rand, k) for k in dir(LC.Cfg.domain_rand) if not k.startswith("_")}
    had = hasattr(LC.Cfg.domain_rand, "restitution")
    try:
        DR.rand_large()
        assert LC.Cfg.domain_rand.friction_range == [0.04, 6.0] and LC.Cfg.domain_rand.added_mass_range == [-1.5, 4.]
    finally:
        for k, v in saved.items():
            setattr(LC.Cfg.domain_rand, k, v)
        if not had:
            delattr(LC.Cfg.domain_rand, "restitution")


# ---- 4. the fp64 model on hand-computable cases ------------------------------------------------------------------------------------
def _vals(N, v):
    return np.full((E.M, N), float(v))


def test_model_constant_metric():
    N = 6
    acc = E.Accumulators(N)
    z = np.zeros(N, np.int64)
    for _ in range(5):
        E.accumulate(acc, _vals(N, 2.0), z, z, z + 10, warmup_steps=0)
    t = E.reduce(acc, np.zeros(N, np.int64), 1)
    for m in range(E.M):
        v = 0.0 if m == E.TERMINATION else 2.0
        assert t[0, m].tolist() == [30.0, v, 0.0, v, v, 0.0]
    assert t[0, E.M].tolist() == [6.0, 30.0, 0.0, 0.0, 0.0, 0.0]


def test_model_one_nonfinite_value():
    N = 4
    acc = E.Accumulators(N)
    z = np.zeros(N, np.int64)
    v = _vals(N, 1.0)
    E.accumulate(acc, v, z, z, z + 5, 0)
    v2 = v.copy()
    v2[7, 2] = np.inf                      # CoT of environment 2
    v2[7, 3] = np.nan
    E.accumulate(acc, v2, z, z, z + 6, 0)
    assert acc.nonfinite[7].tolist() == [0, 0, 1, 1] and acc.count[7].tolist() == [2, 2, 1, 1]
    assert acc.sum[7].tolist() == [2.0, 2.0, 1.0, 1.0] and acc.max[7].tolist() == [1.0] * 4
    t = E.reduce(acc, np.zeros(N, np.int64), 1)
    assert t[0, 7].tolist() == [6.0, 1.0, 0.0, 1.0, 1.0, 2.0]
    assert t[0, 6].tolist() == [8.0, 1.0, 0.0, 1.0, 1.0, 0.0]


def test_model_reset_step_and_warmup_boundary():
    N = 5
    acc = E.Accumulators(N)
    #          terminated  timed out  warm-up (== W)  first counted (W + 1)  long running
    reset = np.array([1, 1, 0, 0, 0])
    tout = np.array([0, 1, 0, 0, 0])
    elb = np.array([0, 0, 3, 4, 50])
    E.accumulate(acc, _vals(N, 7.0), reset, tout, elb, warmup_steps=3)
    assert acc.steps.tolist() == [1] * 5
    assert acc.episodes_terminated.tolist() == [1, 0, 0, 0, 0] and acc.episodes_timed_out.tolist() == [0, 1, 0, 0, 0]
    assert acc.warmup_excluded == 1
    for m in range(E.M):
        if m == E.TERMINATION:
            assert acc.count[m].tolist() == [1, 1, 0, 1, 1] and acc.sum[m].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
        else:
            assert acc.count[m].tolist() == [0, 0, 0, 1, 1] and acc.sum[m].tolist() == [0.0, 0.0, 0.0, 7.0, 7.0]
            assert acc.min[m].tolist() == [np.inf, np.inf, np.inf, 7.0, 7.0]
    t = E.reduce(acc, np.zeros(N, np.int64), 1)
    assert t[0, E.TERMINATION].tolist() == [4.0, 0.5, 0.5, 0.0, 1.0, 0.0]
    assert t[0, E.M].tolist() == [5.0, 5.0, 1.0, 1.0, 0.2, 0.0]


def test_model_groups_empty_group_and_unevaluated_environments():
    N = 8
    acc = E.Accumulators(N)
    z = np.zeros(N, np.int64)
    v = np.tile(np.arange(N, dtype=np.float64), (E.M, 1))
    E.accumulate(acc, v, z, z, z + 9, 0)
    group = np.array([0, 0, 2, 2, 2, -1, -1, 7])          # group 1 is empty; -1 and 7 (outside the table) are not evaluated
    t = E.reduce(acc, group, 3)
    assert t[0, 0].tolist() == [2.0, 0.5, 0.5, 0.0, 1.0, 0.0]
    assert t[2, 0].tolist() == [3.0, 3.0, np.sqrt(29.0 / 3.0 - 9.0), 2.0, 4.0, 0.0]      # Q / n - mean^2 = 29/3 - 9
    assert t[1, 0, 0] == 0.0 and np.isnan(t[1, 0, 1:5]).all() and t[1, 0, 5] == 0.0
    assert t[1, E.M, 0] == 0.0 and np.isnan(t[1, E.M, 4])
    assert t[:, E.M, 0].sum() == 5.0


def test_model_metric_values_by_hand():
    snap = dict(base_lin_vel=np.array([[3.0], [4.0], [9.0]]), base_ang_vel=np.array([[0.0], [0.0], [-0.5]]),
                commands=np.array([[1.0], [0.0], [0.25]]), root_states=np.array([[0.0]] * 2 + [[0.5]] + [[0.0]] * 10),
                measured_heights=np.array([[0.1], [0.3]]), torques=np.array([[2.0], [-6.0]] + [[0.0]] * 10),
                dof_vel=np.array([[1.5], [0.5]] + [[1.0]] * 10), payloads=np.array([1.0]))
    v = E.metric_values(snap, default_body_mass=4.0)[:, 0]
    assert np.allclose(v[:7], [2.0, 0.75, 3.0, -0.5, 0.3, 6.0, 0.0]) and np.isclose(v[8], 9.0 / 2.94)
    snap["torques"][0, 0] = 4.0
    v = E.metric_values(snap, default_body_mass=4.0)[:, 0]
    assert np.isclose(v[6], 3.0) and np.isclose(v[7], 3.0 / (5.0 * 9.8 * 5.0))
    snap["measured_heights"] = None
    assert E.metric_values(snap)[4, 0] == 0.5


# ---- the kernel source under the SIMT emulator against the model ---------------------------------------------------------------------
def eval_emu():
    """go1eval.hip under the SIMT emulator (util.build_emu): the one emulator library of every family of libgo1eval"""
    import __graft_entry__ as g
    return build_emu(g.eval_sources(), "libgo1eval_emu.so")


def random_snapshot(rng, N, P, step):
    s = dict(base_lin_vel=rng.standard_normal((3, N)), base_ang_vel=rng.standard_normal((3, N)), commands=rng.standard_normal((15, N)),
             root_states=rng.standard_normal((13, N)), measured_heights=None if P == 0 else 0.1 * rng.standard_normal((P, N)),
             torques=20 * rng.standard_normal((12, N)), dof_vel=8 * rng.standard_normal((12, N)), payloads=rng.uniform(-1, 3, N))
    s = {k: (None if v is None else v.astype(np.float32)) for k, v in s.items()}
    s["base_lin_vel"][0:2, rng.random(N) < 0.05] = 0.0                    # robots that stand still
    s["reset_buf"] = (rng.random(N) < 0.1).astype(np.uint8)
    s["time_out_buf"] = (s["reset_buf"] & (rng.random(N) < 0.5)).astype(np.uint8)
    s["episode_length_buf"] = np.where(s["reset_buf"] > 0, 0, rng.integers(1, 8, N)).astype(np.int32)
    return s


@pytest.mark.parametrize("N,P", [(300, 17), (64, 0)])
def test_emulated_kernels_follow_the_model(N, P):
    import go1eval_host as G
    lib = ctypes.CDLL(eval_emu())
    rng = np.random.default_rng(5 + N)
    W, groups = 2, 3
    group = rng.integers(-1, groups + 1, N).astype(np.int32)           # includes -1 and an id outside the table
    group[group == 1] = 0                                               # group 1 stays empty
    dt = dict(count=np.uint32, sum=np.float64, sumsq=np.float64, min=np.float32, max=np.float32, nonfinite=np.uint32)
    acc = {k: np.full((E.M, N), 99, d) for k, d in dt.items()}          # (garbage: go1eval_clear has to initialise)
    per = {k: np.full(N, 99, np.uint32) for k in ("steps", "episodes_terminated", "episodes_timed_out")}
    table = np.full((groups, E.M + 1, 6), -1.0)
    cfg, buf = G.Go1EvalConfig(), G.Go1EvalBuffers()
    cfg.num_envs, cfg.num_height_points, cfg.warmup_steps, cfg.num_groups, cfg.default_body_mass = N, P, W, groups, 4.801
    for k, a in list(acc.items()) + list(per.items()):
        setattr(buf, k, a.ctypes.data)
    buf.group, buf.results = group.ctypes.data, table.ctypes.data
    assert lib.go1eval_clear(ctypes.byref(cfg), ctypes.byref(buf), None) == 0
    model = E.Accumulators(N)
    for step in range(12):
        s = random_snapshot(rng, N, P, step)
        for k, a in s.items():
            setattr(buf, k, None if a is None else a.ctypes.data)
        assert lib.go1eval_accumulate(ctypes.byref(cfg), ctypes.byref(buf), None) == 0
        E.accumulate_snapshot(model, s, W)
    assert lib.go1eval_reduce(ctypes.byref(cfg), ctypes.byref(buf), None) == 0
    assert model.warmup_excluded > 0 and model.nonfinite[7].sum() > 0 and model.episodes_terminated.sum() > 0 and model.episodes_timed_out.sum() > 0
    for k in ("count", "nonfinite"):
        assert np.array_equal(acc[k], getattr(model, k)), k
    for k in per:
        assert np.array_equal(per[k], getattr(model, k)), k
    for m in (2, 3, 5, 9):                                              # pure selections of fp32 inputs: equal
        assert np.array_equal(acc["min"][m], model.min[m]) and np.array_equal(acc["max"][m], model.max[m])
        assert np.array_equal(acc["sum"][m], model.sum[m])
    for m in range(E.M):                                                # fp32 arithmetic against fp64: a few roundings of the largest term
        scale = max(1.0, np.abs(model.sum[m]).max())
        if m == 7:                                                      # CoT: relative to each environment's own sum of |terms|
            assert np.allclose(acc["sum"][m], model.sum[m], rtol=2e-4, atol=1e-6 * scale)
        else:
            assert np.abs(acc["sum"][m] - model.sum[m]).max() <= 2e-6 * scale, (m, np.abs(acc["sum"][m] - model.sum[m]).max(), scale)
    want = E.reduce(model, group, groups)
    assert np.array_equal(table[:, :, 0], want[:, :, 0]) and np.array_equal(table[:, :, 5], want[:, :, 5])
    assert np.array_equal(table[:, E.M], want[:, E.M], equal_nan=True)
    assert np.array_equal(np.isnan(table), np.isnan(want)) and np.isnan(table[1, :E.M, 1:5]).all()
    assert np.allclose(table, want, rtol=2e-4, atol=1e-5, equal_nan=True)
    # the reduction of the kernel's own accumulators in the model's fixed order: the same bits
    own = E.Accumulators(N)
    for k in dt:
        setattr(own, k, acc[k].astype(np.float64 if dt[k] != np.uint32 else np.int64))
    for k in per:
        setattr(own, k, per[k].astype(np.int64))
    assert np.array_equal(table, E.reduce(own, group, groups), equal_nan=True)


# ---- 5. the environment hooks without a GPU --------------------------------------------------------------------------------------------
def test_metrics_hooks_on_cpu_buffers(monkeypatch):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    monkeypatch.delitem(sys.modules, "go1eval_host", raising=False)
    cfg = apply_train_config(make_cfg(), num_envs=16)
    cfg.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    env = VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=cfg)
    for _ in range(3):
        env.step(torch.zeros(16, 12))
    assert "go1eval_host" not in sys.modules                       # an environment that never armed metrics never imports the library
    for call in (lambda: env.start_metrics(torch.zeros(16, dtype=torch.int32)), env.stop_metrics, env.read_metrics):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    assert "go1eval_host" not in sys.modules
    env.step(torch.zeros(16, 12))                                   # and stepping goes on


# ---- the sweep's host pieces ---------------------------------------------------------------------------------------------------------------
def test_sweep_grid_commands_and_tables(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    from go1_gym_learn.eval_metrics import sweep
    from go1_gym_learn.ppo_cse.actor_critic import ActorCritic
    grid = dict(vx=[0.5, 1.5], yaw=[0.0, 0.5], gait=[sweep.GAITS["trotting"], sweep.GAITS["pacing"]])
    cells = sweep.grid_cells(grid)
    assert len(cells) == 8 and cells[0] == (0.5, 0.0, (0.5, 0.0, 0.0)) and cells[-1] == (1.5, 0.5, (0.0, 0.0, 0.5))
    cmd = sweep.command_table(cells, 15, "cpu")
    assert cmd.shape == (8, 15) and cmd[:, 0].tolist() == [0.5] * 4 + [1.5] * 4 and cmd[:, 2].tolist() == [0.0, 0.0, 0.5, 0.5] * 2
    assert cmd[1, 5:8].tolist() == [0.0, 0.0, 0.5] and cmd[:, 4].tolist() == [3.0] * 8 and torch.allclose(cmd[:, 13], torch.full((8,), 0.40))
    res = dict(preset="static_medium", cells=cells, num_envs=1024, steps=150, warmup_steps=10, seed=5,
               metrics={n: np.arange(48, dtype=np.float64).reshape(8, 6) for n in E.METRICS}, groups=np.ones((8, 5)))
    md = sweep.markdown_table(res).splitlines()
    assert len(md) == 10 and md[0].startswith("| vx | yaw | gait | envs | fall rate | lin_vel_rmsd") and "| 1.5 | 0.5 | 0/0/0.5 | 1 | 1.000 | 43 ± 44" in md[-1]
    js = json.loads(json.dumps(eval_sweep.to_json(res)))
    assert js["cells"][7] == dict(vx=1.5, yaw=0.5, gait=[0.0, 0.0, 0.5]) and js["metrics"]["CoT"][7][1] == 43.0 and js["fields"] == E.FIELDS
    # both checkpoint forms give the same deterministic actions
    torch.manual_seed(0)
    ac = ActorCritic(7, 2, 21, 12)
    torch.save(ac.state_dict(), str(tmp_path / "ac_weights_last.pt"))
    loaded = eval_sweep.load_policy(str(tmp_path), "cpu")
    obs = {"obs_history": torch.randn(5, 21)}
    with torch.inference_mode():
        want = ac.act_inference(obs)
        assert torch.equal(sweep.deterministic_action(loaded, obs), want)
        jit = tmp_path / "jit"
        jit.mkdir()
        torch.jit.script(ac.adaptation_module).save(str(jit / "adaptation_module_latest.jit"))
        torch.jit.script(ac.actor_body).save(str(jit / "body_latest.jit"))
        scripted = eval_sweep.load_policy(str(jit), "cpu")
        assert torch.allclose(sweep.deterministic_action(scripted, obs), want, atol=1e-6) and torch.equal(scripted.act_inference(obs), sweep.deterministic_action(scripted, obs))
    with pytest.raises(FileNotFoundError):
        eval_sweep.load_policy(str(tmp_path / "nothing"), "cpu")


def test_sweep_keeps_the_cells_commands_through_resets(monkeypatch):
    """an episode reset draws new commands inside the step (resampling_time = 1e9 ends the periodic resampling only): the sweep
    writes the grid's commands before every step, so a respawned robot keeps counting towards the cell it is measured for"""
    import fake_sim
    from go1_gym_learn.eval_metrics import sweep
    fake_sim.install(monkeypatch)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    cells = sweep.grid_cells(dict(vx=[0.5, 1.5], yaw=[0.0], gait=[sweep.GAITS["trotting"]]))
    env, cfg = sweep.build_eval_env("static_medium", 32, seed=2, terrain="plane")
    assert cfg.commands.resampling_time == 1e9
    obs, group, commands = sweep.prepare(env, cells)
    base = env.env
    assert group.tolist() == [0, 1] * 16 and torch.equal(base.commands, commands) and commands[:, 0].tolist() == [0.5, 1.5] * 16
    g = torch.Generator().manual_seed(0)
    thrash = types.SimpleNamespace(act_inference=lambda o: 4.0 * torch.randn(32, 12, generator=g))       # robots that fall
    fell = torch.zeros(32, dtype=torch.bool)
    with torch.inference_mode():
        # write-once is not enough: after the first falls the respawned environments carry other commands
        for _ in range(60):
            obs, _, _, _ = env.step(sweep.deterministic_action(thrash, obs))
            fell |= base.reset_buf.bool() & ~base.time_out_buf
        assert int(fell.sum()) >= 4
        assert not sweep.commands_held(env, commands) and not torch.equal(base.commands[fell], commands[fell])
        assert torch.equal(base.commands[~fell], commands[~fell])
        # the sweep's own step: every environment that the last step did not reset carries its cell's commands again
        for _ in range(60):
            obs = sweep.policy_step(env, thrash, obs, commands)
            fell |= base.reset_buf.bool() & ~base.time_out_buf
            assert sweep.commands_held(env, commands)
    assert int(fell.sum()) >= 8
    keep = ~base.reset_buf.bool()
    assert torch.equal(base.commands[keep], commands[keep]) and int(keep.sum()) > 0
    obs = sweep.rollout(env, thrash, obs, 5, commands)
    assert sweep.commands_held(env, commands)
