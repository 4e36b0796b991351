"""CPU checks of how the measurement families are wired through the three host layers above the libraries: the order in which
`LeggedRobot.step()` calls the armed families, the state-family list and what `load_state` says about it, the public hooks' signatures and
their laziness, the call sequence and the result keys of the seven `run_*_sweep` functions on a recording environment, and which mode
flags `tools/eval_sweep.py` accepts together, with every mode's own options and defaults.  None of it runs device code: these tests pin
the behaviour of the wiring itself."""
import inspect
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HOST_MODULES = ("go1eval_host", "go1feet_host", "go1trunk_host", "go1gait_host", "go1spectrum_host", "go1place_host", "go1reward_host", "go1episode_host",
                "go1sens_host", "go1obs_host", "go1state_host")
# (attribute, per-step method) in launch order
STEPPED = [("_metrics", "accumulate"), ("_behaviour", "accumulate"), ("_trace", "record"), ("_traversal", "accumulate"), ("_joints", "accumulate"),
           ("_feet", "accumulate"), ("_trunk", "accumulate"), ("_gait", "accumulate"), ("_spectrum", "accumulate"), ("_place", "accumulate"),
           ("_reward", "accumulate"), ("_episodes", "accumulate"), ("_sens", "accumulate"), ("_obs", "accumulate")]
STATE_FAMILIES = (("metrics", "_metrics"), ("behaviour", "_behaviour"), ("trace", "_trace"), ("terrain", "_traversal"), ("joints", "_joints"),
                  ("feet", "_feet"), ("trunk", "_trunk"), ("gait", "_gait"), ("spectrum", "_spectrum"), ("placement", "_place"), ("rewards", "_reward"),
                  ("episodes", "_episodes"), ("sensitivity", "_sens"), ("observations", "_obs"))
# the whole table: name, attribute, host module, class, per-step method (the behaviour table has none: it is folded beside the scalar one)
FAMILIES = (("metrics", "_metrics", "go1eval_host", "Go1Eval", "accumulate"),
            ("behaviour", "_behaviour", "go1eval_host", "Go1Behaviour", None),
            ("trace", "_trace", "go1eval_host", "Go1Trace", "record"),
            ("terrain", "_traversal", "go1eval_host", "Go1Terrain", "accumulate"),
            ("joints", "_joints", "go1eval_host", "Go1Joints", "accumulate"),
            ("feet", "_feet", "go1feet_host", "Go1Feet", "accumulate"),
            ("trunk", "_trunk", "go1trunk_host", "Go1Trunk", "accumulate"),
            ("gait", "_gait", "go1gait_host", "Go1Gait", "accumulate"),
            ("spectrum", "_spectrum", "go1spectrum_host", "Go1Spectrum", "accumulate"),
            ("placement", "_place", "go1place_host", "Go1Place", "accumulate"),
            ("rewards", "_reward", "go1reward_host", "Go1Reward", "accumulate"),
            ("episodes", "_episodes", "go1episode_host", "Go1Episodes", "accumulate"),
            ("sensitivity", "_sens", "go1sens_host", "Go1Sensitivity", "accumulate"),
            ("observations", "_obs", "go1obs_host", "Go1Observations", "accumulate"))
REWARD = STEPPED.index(("_reward", "accumulate"))


def plane_env(monkeypatch, num_envs=16):
    import fake_sim
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    fake_sim.install(monkeypatch)
    for module in HOST_MODULES:
        monkeypatch.delitem(sys.modules, module, raising=False)
    c = apply_train_config(make_cfg(), num_envs=num_envs)
    c.terrain.mesh_type = "plane"
    torch.manual_seed(0)
    return VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=c)


class Stub:
    """stands in for a family object: notes every per-step call in the shared log"""

    def __init__(self, attr, log, armed=True):
        self.attr, self.log, self.armed = attr, log, armed

    def accumulate(self, *args):
        self.log.append((self.attr, "accumulate", args))

    def record(self, *args):
        self.log.append((self.attr, "record", args))

    def snapshot(self, *args):                                                # (reset_idx tells the sensitivity family; not a per-step call)
        pass

    def note_reset(self, *args):                                              # (reset_idx tells the observation family; not a per-step call)
        pass


def put_stubs(env, log, armed=True, stepped=STEPPED):
    for attr, _ in stepped:
        setattr(env, attr, Stub(attr, log, armed))


# ---- 1. the per-step dispatch ------------------------------------------------------------------------------------------------------------------
def test_step_calls_the_armed_families_in_launch_order(monkeypatch):
    import go1sim_host as H
    env = plane_env(monkeypatch)
    zero = torch.zeros(16, 12)
    assert all(getattr(env, attr) is None for attr, _ in STEPPED) and env._push is None and env._state is None
    env.step(zero)                                                            # nothing was ever started: nothing to call, nothing imported
    log = []
    put_stubs(env, log)
    counter = env.common_step_counter
    env.step(zero)
    assert env.common_step_counter == counter + 1
    assert [(attr, method) for attr, method, _ in log] == STEPPED
    assert all(args == () for k, (_, _, args) in enumerate(log) if k != REWARD)      # the reward stub alone receives an argument
    (gravity,) = log[REWARD][2]                                               # the gravity of the step just taken: the counter before its increment
    assert np.array_equal(gravity, H.gravity_at(env.sim_config, counter)) and gravity.shape == (3,)
    # the behaviour table is folded only beside the scalar one
    del log[:]
    env._metrics.armed = False
    env.step(zero)
    assert [(attr, method) for attr, method, _ in log] == STEPPED[2:]
    del log[:]
    env._metrics.armed, env._behaviour.armed = True, False
    env.step(zero)
    assert [(attr, method) for attr, method, _ in log] == STEPPED[:1] + STEPPED[2:]
    # a disarmed family is never called, whichever it is
    for k, (attr, _) in enumerate(STEPPED[2:], start=2):
        put_stubs(env, log)
        getattr(env, attr).armed = False
        del log[:]
        env.step(zero)
        assert [(a, m) for a, m, _ in log] == STEPPED[:k] + STEPPED[k + 1:], attr
    put_stubs(env, log, armed=False)
    del log[:]
    env.step(zero)
    assert log == []
    for attr, _ in STEPPED:
        setattr(env, attr, None)
    env.step(zero)
    assert log == [] and all(m not in sys.modules for m in HOST_MODULES)


# ---- 2. the state families -----------------------------------------------------------------------------------------------------------------------
def test_state_families_and_the_refusal_of_load_state(monkeypatch):
    from go1_gym.envs.base.legged_robot import LeggedRobot
    env = plane_env(monkeypatch)
    assert env._STATE_FAMILIES == STATE_FAMILIES and isinstance(env._STATE_FAMILIES, tuple)
    # the one table, whole: fourteen rows of five columns, and everything else made of it
    assert LeggedRobot._FAMILIES == FAMILIES and len(FAMILIES) == 14 and all(len(row) == 5 for row in LeggedRobot._FAMILIES)
    assert LeggedRobot._STEPPED == tuple(pair for pair in STEPPED if pair[0] != "_behaviour")
    assert list(LeggedRobot._HOST) == [row[1] for row in FAMILIES] + ["_push"] and len(LeggedRobot._HOST) == 15 and list(LeggedRobot._HOST)[-2:] == ["_obs", "_push"]
    assert all(LeggedRobot._HOST[attr] == (module, cls) for _, attr, module, cls, _ in FAMILIES) and LeggedRobot._HOST["_push"] == ("go1eval_host", "Go1Push")
    assert not [name for name in dir(LeggedRobot) if "LATER" in name or "MORE_" in name or "FURTHER" in name]      # no table beside the table
    restored = []
    env._state = types.SimpleNamespace(restore=lambda *a, **k: restored.append((a, k)))       # the state library is never reached by a refusal
    put_stubs(env, [])
    with pytest.raises(RuntimeError) as e:
        env.load_state(None)
    assert "load_state(): refused while metrics, behaviour, trace, terrain, joints, feet, trunk, gait, spectrum, placement, rewards, episodes, sensitivity, observations are armed: stop them first" in str(e.value)
    put_stubs(env, [], armed=False)
    env._place.armed = True
    with pytest.raises(RuntimeError, match=r"refused while placement is armed: stop it first"):
        env.load_state(None)
    assert restored == []
    env._place = None
    state = types.SimpleNamespace(whole=False, counter=0)
    env.load_state(state, env_ids=[1])                                        # disarmed or never made: not refused
    assert len(restored) == 1 and restored[0][0][0] is state


# ---- 3. the public hooks -------------------------------------------------------------------------------------------------------------------------
REQUIRED = "required"
HOOKS = dict(
    start_metrics=dict(groups=REQUIRED, warmup_steps=0, behaviour=False), stop_metrics={}, read_metrics={},
    start_trace=dict(env_ids=None, capacity=None), stop_trace={}, read_trace={},
    trace_response=dict(signals=REQUIRED, switch_row=REQUIRED, pre=REQUIRED, smooth=REQUIRED, band=REQUIRED, hold=REQUIRED, tail=REQUIRED, groups=REQUIRED, dt=None),
    push_robots=dict(push=REQUIRED, env_ids=None),
    trace_recovery=dict(push_row=REQUIRED, pre=REQUIRED, smooth=REQUIRED, band=REQUIRED, hold=REQUIRED, groups=REQUIRED, dt=None),
    start_terrain_metrics=dict(groups=REQUIRED, warmup_steps=0), stop_terrain_metrics={}, read_terrain_metrics={},
    start_joint_metrics=dict(groups=REQUIRED, warmup_steps=0), stop_joint_metrics={}, read_joint_metrics={},
    start_foot_metrics=dict(groups=REQUIRED, warmup_steps=0), stop_foot_metrics={}, read_foot_metrics={},
    start_trunk_metrics=dict(groups=REQUIRED, warmup_steps=0, segment_steps=50, tilt_limit=0.25), stop_trunk_metrics={}, read_trunk_metrics={},
    start_gait_metrics=dict(groups=REQUIRED, warmup_steps=0, min_stride_steps=1, max_stride_steps=100), stop_gait_metrics={}, read_gait_metrics={},
    start_spectrum_metrics=dict(groups=REQUIRED, warmup_steps=0, segment_steps=100, high_freq=10.0, taper="hann"), stop_spectrum_metrics={}, read_spectrum_metrics={},
    start_placement_metrics=dict(groups=REQUIRED, warmup_steps=0, map_cell=0.03), stop_placement_metrics={}, read_placement_metrics={},
    start_reward_metrics=dict(groups=REQUIRED, warmup_steps=0), stop_reward_metrics={}, read_reward_metrics={},
    last_reward_terms={})


def test_hook_signatures_docstrings_and_laziness(monkeypatch):
    from go1_gym.envs.base.legged_robot import LeggedRobot
    env = plane_env(monkeypatch)
    env.step(torch.zeros(16, 12))
    for name, wanted in HOOKS.items():
        parameters = inspect.signature(getattr(env, name)).parameters
        found = {k: (REQUIRED if p.default is inspect.Parameter.empty else p.default) for k, p in parameters.items()}
        assert found == wanted and list(found) == list(wanted), name
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in parameters.values()), name
        assert (getattr(LeggedRobot, name).__doc__ or "").strip(), name       # the docstrings are the user documentation
    assert sum(name.startswith(("stop_", "read_")) for name in HOOKS) == 20
    assert isinstance(LeggedRobot.reward_functions, property) and LeggedRobot.reward_functions.__doc__.strip()
    assert not hasattr(env, "reward_functions")                               # it exists only while the reward family has accumulated a step
    # without a GPU every hook says so, makes nothing and imports nothing
    groups = torch.zeros(16, dtype=torch.int32)
    arguments = dict(trace_response=(["lin_vel_x"], 5, 2, 1, 0.1, 3, 4, groups), trace_recovery=(5, 2, 1, 0.1, 3, groups), push_robots=(np.zeros((16, 4), np.float32),))
    for name, wanted in HOOKS.items():
        args = arguments.get(name, (groups,) if "groups" in wanted else ())
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            getattr(env, name)(*args)
    for call in (env.save_state, lambda: env.load_state(None)):
        with pytest.raises(NotImplementedError, match="this simulator's buffers are not on a GPU"):
            call()
    env.step(torch.zeros(16, 12))
    assert all(m not in sys.modules for m in HOST_MODULES)
    assert all(getattr(env, attr) is None for attr, _ in STEPPED) and env._push is None and env._state is None


# ---- 4. the sweeps' skeleton ---------------------------------------------------------------------------------------------------------------------
N, NUM_COMMANDS, STEPS, WARMUP = 12, 15, 3, 2
COMMON_KEYS = ["preset", "cells", "metrics", "groups", "num_envs", "steps", "warmup_steps", "seed", "dt"]
# (module, sweep function, the family's hook stem, its start keywords beyond the warm-up, the cell's wording in the error, what the result holds beside COMMON_KEYS)
SWEEPS = [
    ("joints", "run_joint_sweep", "joint", {}, "grid cell's",
     ["joints", "joint_groups", "hist", "tau_edges", "vel_edges", "torque_limit", "vel_limit", "soft_torque_limit", "soft_vel_limit", "dof_names"]),
    ("feet", "run_foot_sweep", "foot", {}, "grid cell's",
     ["feet", "feet_groups", "profile", "profile_count", "phase_edges", "body_weight", "terrain_friction", "max_contact_force", "foot_names"]),
    ("trunk", "run_trunk_sweep", "trunk", dict(segment_steps=40, tilt_limit=0.5), "grid cell's",
     ["trunk", "trunk_groups", "tilt_hist", "tilt_edges", "segment_steps", "tilt_limit"]),
    ("gait", "run_gait_sweep", "gait", dict(min_stride_steps=3, max_stride_steps=60), "grid cell's",
     ["gait", "gait_groups", "support_hist", "phase_hist", "phase_centres", "support_patterns", "min_stride_steps", "max_stride_steps"]),
    ("spectrum", "run_spectrum_sweep", "spectrum", dict(segment_steps=64, high_freq=8.0, taper="boxcar"), "grid cell's",
     ["step_freq", "spectrum", "spectrum_groups", "psd", "psd_segments", "freq", "signals", "high_bin", "segment_steps", "high_freq", "taper"]),
    ("rewards", "run_reward_sweep", "reward", {}, "grid cell's",
     ["names", "scales", "terms", "share", "reward_groups", "sum", "positive", "negative", "total"]),
    ("placement", "run_placement_sweep", "placement", dict(map_cell=0.05), "cell's",
     ["commands", "placement", "placement_groups", "map", "map_edges", "foot_counts", "map_cell"]),
]
TABLE_KEYS = dict(joint=("joints", "joint_groups"), foot=("feet", "feet_groups"), trunk=("trunk", "trunk_groups"), gait=("gait", "gait_groups"),
                  spectrum=("spectrum", "spectrum_groups"), placement=("placement", "placement_groups"))


def canned(stem, cells):
    """what read_<stem>_metrics returns: the keys the sweep reads, each a distinct object"""
    table, groups = {"m": np.full((cells, 6), 0.5)}, np.ones((cells, 6))
    counts = lambda k: (np.arange(4 * N, dtype=np.int32).reshape(4, N) + k)
    return dict(
        joint=dict(metrics=table, groups=groups, hist=np.zeros((cells, 12, 8, 8)), tau_edges=np.zeros((12, 9)), vel_edges=np.ones((12, 9))),
        foot=dict(metrics=table, groups=groups, profile=np.zeros((cells, 4, 16)), profile_count=np.ones((cells, 4, 16)), phase_edges=np.linspace(0, 1, 17)),
        trunk=dict(metrics=table, groups=groups, tilt_hist=np.zeros((cells, 16)), tilt_edges=np.linspace(0, 1, 17)),
        gait=dict(metrics=table, groups=groups, support_hist=np.zeros((cells, 16)), phase_hist=np.zeros((cells, 3, 16)), phase_centres=np.arange(16) / 16,
                  support_patterns=[str(k) for k in range(16)]),
        spectrum=dict(metrics=table, groups=groups, psd=np.zeros((cells, 40, 33)), psd_segments=np.zeros((cells, 40)), freq=np.arange(33.0), signals=["s"] * 40,
                      high_bin=np.int64(11)),
        reward=dict(names=["a", "b"], scales=np.ones(2), terms={"a": np.zeros((cells, 6))}, share={"a": np.zeros(cells)}, groups=groups,
                    sum=np.zeros((cells, 6)), positive=np.ones((cells, 6)), negative=-np.ones((cells, 6)), total=np.full((cells, 6), 2.0)),
        placement=dict(metrics=table, groups=groups, map=np.zeros((cells, 4, 8, 8)), map_edges=np.linspace(-0.12, 0.12, 9), touchdowns=counts(0),
                       strides=counts(1), map_outside=counts(2)))[stem]


class RecordingBase:
    """the part of LeggedRobot a sweep touches: every start_*, stop_* and read_* call is noted with its arguments"""
    num_envs, device, dt = N, "cpu", 0.02

    def __init__(self, stem, cells, spoil):
        self.log, self.stem, self.cells, self.spoil = [], stem, cells, spoil
        self.commands = torch.full((N, NUM_COMMANDS), -7.0)
        self.reset_buf = torch.zeros(N, dtype=torch.int32)
        self.dof_names = [f"joint{j}" for j in range(12)]
        self.payloads = torch.full((N,), 2.0)
        self._joints = types.SimpleNamespace(cfg=types.SimpleNamespace(torque_limit=[33.5] * 12, vel_limit=[50.0, 28.0, 28.0] * 4, soft_torque_limit=0.9, soft_vel_limit=0.8))
        self._feet = types.SimpleNamespace(cfg=types.SimpleNamespace(terrain_friction=1.0, max_contact_force=100.0))
        self.family = canned(stem, cells)

    def __getattr__(self, name):
        if not name.startswith(("start_", "stop_", "read_")):
            raise AttributeError(name)

        def hook(*args, **kwargs):
            self.log.append((name, args, kwargs))
            if name == "read_metrics":
                return dict(lin_vel_rmsd=np.zeros((self.cells, 6)), groups=np.full((self.cells, 5), 3.0))
            if name.startswith("read_"):
                return self.family
        return hook


class RecordingEnv:
    """the wrapper a sweep steps.  A step notes whether every environment carries the commands the sweep first wrote, then respawns
    environment 0 as a reset does (new commands, reset_buf set); with `spoil` the last step also moves a command of environment 1 without
    a reset"""

    def __init__(self, stem, cells, spoil=False):
        self.env = RecordingBase(stem, cells, spoil)
        self.first, self.steps = None, 0

    def reset(self):
        return self.get_observations()

    def get_observations(self):
        return dict(obs=torch.zeros(N, 4), obs_history=torch.zeros(N, 8))

    def step(self, actions):
        base = self.env
        assert actions.shape == (N, 12) and not actions.any()
        if self.first is None:
            self.first = base.commands.clone()
        base.log.append(("step", bool(torch.equal(base.commands, self.first)), {}))
        self.steps += 1
        base.commands[0] = 9.0
        base.reset_buf[:] = 0
        base.reset_buf[0] = 1
        if base.spoil and self.steps == STEPS:
            base.commands[1, 0] += 0.25
        return self.get_observations(), None, None, None


class ZeroPolicy:
    evaluated = 0

    def eval(self):
        self.evaluated += 1

    def act_inference(self, obs):
        return torch.zeros(N, 12)


@pytest.mark.parametrize("module, function, stem, options, wording, keys", SWEEPS, ids=[s[0] for s in SWEEPS])
def test_sweeps_share_one_call_sequence(monkeypatch, module, function, stem, options, wording, keys):
    import importlib
    from go1_gym_learn.eval_metrics import behaviour, sweep
    run = getattr(importlib.import_module("go1_gym_learn.eval_metrics." + module), function)
    if module == "placement":
        cells_in = dict(stance_width=[0.1, 0.3], vx=[0.5, 1.0])
        cells = behaviour.behaviour_cells(cells_in)
        table = behaviour.behaviour_command_table(cells, NUM_COMMANDS, "cpu")
    else:
        cells_in = dict(vx=[0.5, 1.0], yaw=[0.0, 0.5], gait=[sweep.GAITS["trotting"]])
        cells = sweep.grid_cells(cells_in)
        table = sweep.command_table(cells, NUM_COMMANDS, "cpu")
    assert len(cells) == 4
    built = []

    def build(preset, num_envs, seed, terrain=None, configure=None):
        built.append((preset, num_envs, seed, terrain, configure))
        return built_env, None
    monkeypatch.setattr(sweep, "build_eval_env", build)
    built_env, policy = RecordingEnv(stem, len(cells)), ZeroPolicy()
    res = run(policy, "static_medium", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5, terrain="plane", **options)
    base = built_env.env
    assert built == [("static_medium", N, 5, "plane", None)] and policy.evaluated == 1
    group = torch.arange(N) % len(cells)
    assert torch.equal(built_env.first, table[group])                        # environment i carries cell i % cells
    names = [entry[0] for entry in base.log]
    assert names == ["start_metrics", f"start_{stem}_metrics", "step", "step", "step", "stop_metrics", f"stop_{stem}_metrics", "read_metrics", f"read_{stem}_metrics"]
    (_, scalar_args, scalar_kw), (_, family_args, family_kw) = base.log[0], base.log[1]
    assert len(scalar_args) == 1 and scalar_args[0] is family_args[0] and len(family_args) == 1
    assert scalar_args[0].dtype == torch.int32 and torch.equal(scalar_args[0], group.to(torch.int32))
    assert scalar_kw == dict(warmup_steps=WARMUP) and family_kw == dict(warmup_steps=WARMUP, **options)
    assert [entry[1] for entry in base.log[2:5]] == [True, True, True]       # the commands are written again before every step
    assert all(args == () and kw == {} for _, args, kw in base.log[5:])
    assert sorted(res) == sorted(COMMON_KEYS + keys) and len(res) == len(COMMON_KEYS) + len(keys)
    assert (res["preset"], res["cells"], res["num_envs"], res["steps"], res["warmup_steps"], res["seed"], res["dt"]) == ("static_medium", cells, N, STEPS, WARMUP, 5, 0.02)
    assert list(res["metrics"]) == ["lin_vel_rmsd"] and res["groups"].shape == (4, 5) and (res["groups"] == 3.0).all()
    assert all(res[k] == v for k, v in options.items())
    family = base.family
    if stem == "reward":
        assert res["reward_groups"] is family["groups"] and all(res[k] is family[k] for k in ("names", "scales", "terms", "share", "sum", "positive", "negative", "total"))
    else:
        table_key, groups_key = TABLE_KEYS[stem]
        assert res[table_key] is family["metrics"] and res[groups_key] is family["groups"]
    if stem == "joint":
        assert (res["torque_limit"], res["vel_limit"][:3], res["soft_torque_limit"], res["soft_vel_limit"]) == ([33.5] * 12, [50.0, 28.0, 28.0], 0.9, 0.8)
        assert res["dof_names"] == base.dof_names and res["hist"] is family["hist"]
    if stem == "foot":
        from go1_gym_learn.eval_metrics import feet
        assert res["body_weight"] == (feet.total_mass() + 2.0) * feet.GRAVITY and (res["terrain_friction"], res["max_contact_force"]) == (1.0, 100.0)
        assert res["foot_names"] == ["FL", "FR", "RL", "RR"] and res["profile"] is family["profile"]
    if stem == "spectrum":
        assert res["step_freq"] == [3.0] * 4 and res["high_bin"] == 11 and type(res["high_bin"]) is int and res["psd"] is family["psd"]
    if stem == "placement":
        assert np.array_equal(res["commands"], table.numpy())
        member = group.numpy()
        for k, name in enumerate(("touchdowns", "strides", "map_outside")):
            wanted = np.stack([family[name][:, member == g].sum(axis=1) for g in range(4)]).astype(np.float64)
            assert res["foot_counts"][name].dtype == np.float64 and np.array_equal(res["foot_counts"][name], wanted)
        assert list(res["foot_counts"]) == ["touchdowns", "strides", "map_outside"]
    # an environment that left its cell's commands without a reset: the caller says so under its own name
    built_env = RecordingEnv(stem, len(cells), spoil=True)
    with pytest.raises(RuntimeError) as e:
        run(ZeroPolicy(), "static_medium", cells_in, num_envs=N, steps=STEPS, warmup_steps=WARMUP, seed=5, **options)
    assert str(e.value) == f"{function}: an environment left its {wording} commands during the rollout"
    assert [entry[0] for entry in built_env.env.log][-2:] == ["stop_metrics", f"stop_{stem}_metrics"]       # nothing is read after the refusal


# ---- 5. the tool's modes -------------------------------------------------------------------------------------------------------------------------
MODES = dict(terrain=["--terrain"], response=["--response", "--switch", "vx", "0", "1"], behaviour=["--behaviour", "--axis", "stance_width", "0.1"],
             push=["--push", "--magnitude", "1", "--direction", "0"], joints=["--joints"], feet=["--feet"], trunk=["--trunk"], rewards=["--rewards"],
             coordination=["--coordination"], spectrum=["--spectrum"], placement=["--placement", "--axis", "stance_width", "0.1"])
ACCEPTED_PAIRS = {frozenset(("response", "behaviour"))}                       # every other pair of modes excludes each other
# what a command line without a mode parses to, in the fields the modes define
NO_MODE = dict(tiles=False, terrain=None, response=False, behaviour=False, push=False, joints=False, feet=False, trunk=False, rewards=False, coordination=False,
               spectrum=False, placement=False, vx=[0.5, 1.0, 1.5], rows=None, cols=None, window=None, mesh=None, proportions=None, switch=None, axis=None,
               trace_envs=None, magnitude=None, direction=None, paired=False, segment_steps=None, tilt_limit=None, min_stride_steps=None, max_stride_steps=None,
               high_freq=None, taper=None, map_cell=None)
ALONE = dict(terrain=dict(tiles=True, terrain=None, rows=4, cols=5, window=500, mesh="trimesh", vx=[1.0]),
             response=dict(response=True, switch=["vx", "0", "1"]),
             behaviour=dict(behaviour=True, axis=[["stance_width", "0.1"]]),
             push=dict(push=True, magnitude=[1.0], direction=[0.0]),
             joints=dict(joints=True), feet=dict(feet=True), rewards=dict(rewards=True),
             trunk=dict(trunk=True, segment_steps=50, tilt_limit=0.25),
             coordination=dict(coordination=True, min_stride_steps=1, max_stride_steps=100),
             spectrum=dict(spectrum=True, segment_steps=100, high_freq=10.0, taper="hann"),
             placement=dict(placement=True, axis=[["stance_width", "0.1"]], map_cell=0.03))
DEPENDENT = [["--min-stride-steps", "3"], ["--max-stride-steps", "50"], ["--trunk", "--min-stride-steps", "3"], ["--spectrum", "--max-stride-steps", "50"],
             ["--map-cell", "0.05"], ["--coordination", "--map-cell", "0.05"], ["--high-freq", "5"], ["--taper", "boxcar"], ["--trunk", "--high-freq", "5"],
             ["--trunk", "--taper", "boxcar"], ["--segment-steps", "40"], ["--tilt-limit", "0.3"], ["--joints", "--segment-steps", "40"],
             ["--spectrum", "--tilt-limit", "0.3"], ["--rows", "3"], ["--cols", "3"], ["--window", "100"], ["--mesh", "trimesh"], ["--proportions", "1", "0"],
             ["--terrain", "plane", "--rows", "3"], ["--switch", "vx", "0", "1"], ["--trace-envs", "0"], ["--joints", "--trace-envs", "0"], ["--magnitude", "1"],
             ["--direction", "0"], ["--paired"], ["--response", "--paired", "--switch", "vx", "0", "1"]]
OUT_OF_RANGE = [["--coordination", "--min-stride-steps", "0"], ["--coordination", "--min-stride-steps", "5", "--max-stride-steps", "4"],
                ["--spectrum", "--segment-steps", "63"], ["--spectrum", "--segment-steps", "6"], ["--spectrum", "--segment-steps", "130"],
                ["--spectrum", "--high-freq", "0"], ["--spectrum", "--high-freq", "inf"], ["--spectrum", "--taper", "hamming"], ["--placement", "--map-cell", "0"],
                ["--placement", "--map-cell", "inf"], ["--trunk", "--segment-steps", "0"], ["--trunk", "--tilt-limit", "-0.1"], ["--trunk", "--tilt-limit", "inf"],
                ["--terrain", "--rows", "0"], ["--terrain", "--vx", "0.5", "1.0"], ["--push", "--magnitude", "-1", "--direction", "0"], ["--push", "--magnitude", "1"],
                ["--response"], ["--response", "--switch", "vx", "0"]]


def test_tool_modes_exclusions_defaults_and_dependent_options():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import eval_sweep
    base = ["--checkpoint", "c", "--out", "o"]
    assert set(MODES) == set(ALONE) and len(MODES) == 11
    for first, second in itertools.permutations(MODES, 2):
        argv = base + MODES[first] + MODES[second]
        if frozenset((first, second)) in ACCEPTED_PAIRS:
            a = eval_sweep.parse_args(argv)
            assert a.response and a.behaviour and a.switch == ["vx", "0", "1"]
        else:
            with pytest.raises(SystemExit) as e:
                eval_sweep.parse_args(argv)
            assert e.value.code == 2, (first, second)
    fields = lambda a: {k: getattr(a, k) for k in NO_MODE}
    assert fields(eval_sweep.parse_args(base)) == NO_MODE
    for mode, own in ALONE.items():
        assert fields(eval_sweep.parse_args(base + MODES[mode])) == dict(NO_MODE, **own), mode
    # a mode's options given: they arrive; the segment length means the trunk's or the spectrum's
    given = eval_sweep.parse_args(base + ["--trunk", "--segment-steps", "33", "--tilt-limit", "0.4"])
    assert (given.segment_steps, given.tilt_limit) == (33, 0.4)
    given = eval_sweep.parse_args(base + ["--spectrum", "--segment-steps", "64", "--high-freq", "8", "--taper", "boxcar"])
    assert (given.segment_steps, given.high_freq, given.taper) == (64, 8.0, "boxcar")
    given = eval_sweep.parse_args(base + ["--coordination", "--min-stride-steps", "3", "--max-stride-steps", "60"])
    assert (given.min_stride_steps, given.max_stride_steps) == (3, 60)
    assert eval_sweep.parse_args(base + ["--placement", "--map-cell", "0.05"]).map_cell == 0.05
    given = eval_sweep.parse_args(base + ["--terrain", "--rows", "2", "--cols", "3", "--window", "50", "--mesh", "heightfield", "--proportions", "1", "0", "--vx", "0.7"])
    assert (given.rows, given.cols, given.window, given.mesh, given.proportions, given.vx, given.tiles, given.terrain) == (2, 3, 50, "heightfield", [1.0, 0.0], [0.7], True, None)
    for mode in ("joints", "feet", "trunk", "rewards", "coordination", "spectrum", "placement", "behaviour", "response", "push"):
        a = eval_sweep.parse_args(base + MODES[mode] + ["--terrain", "heightfield"])      # with a value it is the mesh type of any sweep
        assert a.terrain == "heightfield" and not a.tiles
    for bad in DEPENDENT + OUT_OF_RANGE:
        with pytest.raises(SystemExit) as e:
            eval_sweep.parse_args(base + bad)
        assert e.value.code == 2, bad
    # the seven table-driven modes stay callables of (a, policy, grid)
    for name in ("run_joints", "run_feet", "run_trunk", "run_gait", "run_spectrum", "run_rewards", "run_placement"):
        assert callable(getattr(eval_sweep, name)) and len(inspect.signature(getattr(eval_sweep, name)).parameters) == 3
    assert all(callable(getattr(eval_sweep, name)) for name in ("run_response", "run_push", "run_terrain", "to_json", "load_policy", "response_switch", "behaviour_axes"))
