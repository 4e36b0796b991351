"""`run_sweep`: measure a policy over a grid of commands under one domain-randomisation preset, without a host read inside
the step loop.

The environment is built from the training configuration with `base_set()` and the preset applied to a fresh `make_cfg()`;
environment i gets cell `i % cells` of the command grid, which is also its group in the result table.  The presets set
`commands.resampling_time = 1e9`, which ends the periodic resampling only: an episode reset still draws new commands inside
the step kernel, so the grid's commands are written again on the device before every step (one copy, no host read; what
tools/play_eval.py does), and after the loop `run_sweep` checks once that every environment still carries its cell's
commands.  `start_metrics` arms libgo1eval (include/go1eval.h), the deterministic policy is stepped `steps` times, and
`read_metrics` reduces per group.
"""
import itertools

import numpy as np
import torch

from . import domain_randomization as DR

# gait (phase, offset, bound) triples of the command vector (commands 5, 6, 7): the four gaits the reference's play script names
GAITS = {"trotting": (0.5, 0.0, 0.0), "pronking": (0.0, 0.0, 0.0), "bounding": (0.0, 0.5, 0.0), "pacing": (0.0, 0.0, 0.5)}
DEFAULT_GRID = dict(vx=[0.5, 1.0, 1.5], yaw=[0.0], gait=[GAITS["trotting"]])


def grid_cells(grid):
    """[(vx, yaw rate, (phase, offset, bound)), ...] in row-major order of (vx, yaw, gait)"""
    return [(float(vx), float(yaw), tuple(float(x) for x in gait))
            for vx, yaw, gait in itertools.product(grid["vx"], grid["yaw"], grid["gait"])]


def command_table(cells, num_commands, device):
    """(cells, num_commands) commands: the cell's velocity and gait, everything else as tools/play_eval.py holds it
    (step frequency 3 Hz, duty 0.5, foot swing 0.08 m, stance width 0.25 m, stance length 0.40 m)"""
    cmd = torch.zeros(len(cells), num_commands)
    for i, (vx, yaw, (phase, offset, bound)) in enumerate(cells):
        cmd[i, 0], cmd[i, 2] = vx, yaw
        cmd[i, 4], cmd[i, 5], cmd[i, 6], cmd[i, 7], cmd[i, 8], cmd[i, 9], cmd[i, 12] = 3.0, phase, offset, bound, 0.5, 0.08, 0.25
        if num_commands > 13:
            cmd[i, 13] = 0.40
    return cmd.to(device)


def build_eval_env(preset, num_envs, seed, terrain=None, configure=None):
    """(HistoryWrapper env, cfg): the training configuration with base_set() and the preset on a fresh configuration tree.
    terrain: None keeps the training terrain; "plane" | "heightfield" | "trimesh" replaces its mesh type.  configure(cfg), if given,
    edits the finished configuration before the environment is built (the terrain sweep lays out its tile grid there)."""
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from go1_gym.envs.wrappers.history_wrapper import HistoryWrapper
    from scripts.train_config import apply_train_config
    cfg = apply_train_config(make_cfg(), num_envs=num_envs)
    DR.base_set(cfg)
    DR.DR_SETTINGS[preset](cfg)
    cfg.seed = seed
    if terrain is not None:
        cfg.terrain.mesh_type = terrain
    if configure is not None:
        configure(cfg)
    torch.manual_seed(seed)              # the terrain and the environments' first draws come from the global generators
    np.random.seed(seed)
    env = VelocityTrackingEasyEnv(sim_device=f"cuda:{torch.cuda.current_device()}", headless=True, cfg=cfg)
    return HistoryWrapper(env), cfg


def deterministic_action(policy, obs):
    """`policy.act_inference(obs)` (the actor's mean on the adaptation module's latent).  The ActorCritic's own act_inference
    also copies the latent to the host for `policy_info` on every call; where the policy exposes the two halves they are called
    directly, which computes the same actions and leaves the stream alone."""
    if hasattr(policy, "_latent") and hasattr(policy, "_actor"):
        h = obs["obs_history"]
        return policy._actor(h, policy._latent(h))
    return policy.act_inference(obs)


def prepare(env, cells):
    """reset, write the grid's commands, and return (first observations, group id per environment, (N, num_commands) commands
    of every environment's cell)"""
    base = env.env
    obs = env.reset()
    group = torch.arange(base.num_envs, device=base.device) % len(cells)
    commands = command_table(cells, base.commands.shape[1], base.device)[group]
    base.commands[:] = commands
    return env.get_observations(), group.to(torch.int32), commands


def policy_step(env, policy, obs, commands):
    """one step of the sweep: the cells' commands written again (a reset inside the last step drew new ones for the environments
    it respawned), then the deterministic action.  No host read."""
    env.env.commands[:] = commands
    obs, _, _, _ = env.step(deterministic_action(policy, obs))
    return obs


def rollout(env, policy, obs, steps, commands):
    """`steps` policy steps; nothing in here reads from the device"""
    with torch.inference_mode():
        for _ in range(steps):
            obs = policy_step(env, policy, obs, commands)
    return obs


def commands_held(env, commands):
    """after a rollout: every environment carries its cell's commands, except those the LAST step reset (they are rewritten before
    the next step; a reset step folds no tracking metric).  One host read."""
    base = env.env
    same = (base.commands == commands).all(dim=1) | base.reset_buf.bool()
    return bool(same.all())


def run_beside_scalar(caller, family, policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain, start_kwargs=None, prepare_cells=None,
                      cell="grid cell"):
    """The rollout every sweep with a table of its own shares: one environment for `preset`, environment i on cell i % cells (written by
    prepare_cells(env, cells), default `prepare`), the scalar table and the table of `family` ("joint", "foot", ...: the stem of the
    environment's start_ / stop_ / read_<family>_metrics hooks, the start taking `start_kwargs`) armed with the same groups and warm-up,
    `steps` policy steps, both stopped, the commands checked (the RuntimeError names `caller` and the `cell`), both read.  Returns (the
    base environment, group per environment, the scalar table without its "groups", those groups, what read_<family>_metrics gave)."""
    env, _ = build_eval_env(preset, num_envs, seed, terrain)
    if hasattr(policy, "eval"):
        policy.eval()
    base = env.env
    obs, group, commands = (prepare_cells or prepare)(env, cells)
    base.start_metrics(group, warmup_steps=warmup_steps)
    getattr(base, f"start_{family}_metrics")(group, warmup_steps=warmup_steps, **(start_kwargs or {}))
    rollout(env, policy, obs, steps, commands)
    base.stop_metrics()
    getattr(base, f"stop_{family}_metrics")()
    if not commands_held(env, commands):
        raise RuntimeError(f"{caller}: an environment left its {cell}'s commands during the rollout")
    scalar = base.read_metrics()
    groups = scalar.pop("groups")
    return base, group, scalar, groups, getattr(base, f"read_{family}_metrics")()


def run_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None):
    """One table for one preset: {"preset", "cells": [(vx, yaw, gait)], "metrics": {name: (cells, 6) array of count, mean, std,
    min, max, nonfinite}, "groups": (cells, 5) array of envs, steps, episodes_terminated, episodes_timed_out, fall_rate}."""
    cells = grid_cells(grid or DEFAULT_GRID)
    env, _ = build_eval_env(preset, num_envs, seed, terrain)
    if hasattr(policy, "eval"):
        policy.eval()
    obs, group, commands = prepare(env, cells)
    env.env.start_metrics(group, warmup_steps=warmup_steps)
    rollout(env, policy, obs, steps, commands)
    env.env.stop_metrics()
    if not commands_held(env, commands):
        raise RuntimeError("run_sweep: an environment left its grid cell's commands during the rollout")
    res = env.env.read_metrics()
    groups = res.pop("groups")
    return dict(preset=preset, cells=cells, metrics=res, groups=groups, num_envs=num_envs, steps=steps, warmup_steps=warmup_steps, seed=seed)


# ---- what every sweep's table and JSON share
FIELDS = ["count", "mean", "std", "min", "max", "nonfinite"]                  # the columns of a metric table's row


def number(x, fmt):
    """x in the format `fmt`, a dash for a NaN or an infinity"""
    return format(x, fmt) if np.isfinite(x) else "–"


def mean_std(row):
    """mean +- std of a metric table's row, a dash for a row that counted nothing"""
    return f"{row[1]:.3g} ± {row[2]:.2g}" if row[0] > 0 else "–"


def clean(a):
    """nested dicts, lists and tuples of numbers, bools and strings as JSON takes them: NaN and infinities as None, tuples as lists"""
    if isinstance(a, dict):
        return {k: clean(v) for k, v in a.items()}
    if isinstance(a, (list, tuple)):
        return [clean(x) for x in a]
    if isinstance(a, (bool, str)):
        return a
    return a if np.isfinite(a) else None


def cells_to_json(cells, **more):
    """the grid's cells (vx, yaw, gait) as a list of dicts; `more` = {key: one value per cell} adds entries to them"""
    return [dict(vx=c[0], yaw=c[1], gait=list(c[2]), **{k: v[g] for k, v in more.items()}) for g, c in enumerate(cells)]


def markdown_table(result, metrics=("lin_vel_rmsd", "ang_vel_rmsd", "base_height", "max_torques", "power_consumption", "CoT", "froude_number")):
    """one row per grid cell: the cell, its fall rate, and mean +- std of the chosen metrics"""
    head = ["vx", "yaw", "gait", "envs", "fall rate"] + list(metrics)
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, (vx, yaw, gait) in enumerate(result["cells"]):
        row = [f"{vx:g}", f"{yaw:g}", "/".join(f"{x:g}" for x in gait), f"{int(result['groups'][g, 0])}", f"{result['groups'][g, 4]:.3f}"]
        row += [f"{result['metrics'][m][g, 1]:.4g} ± {result['metrics'][m][g, 2]:.3g}" for m in metrics]
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)
