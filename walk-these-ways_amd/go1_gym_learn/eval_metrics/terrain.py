"""Terrain traversal: which terrain type and difficulty does a policy cross, where does it fall, how often does it stumble, how
high do its feet swing above the ground they are over?

`run_terrain_sweep` builds the training configuration on a small curriculum tile grid (the row is the difficulty, the column the
terrain type: go1_gym/utils/terrain.py), places environment i on tile `i % cells`, commands every robot forward and runs one
window with libgo1eval's fifth kernel family armed (include/go1eval.h): per tile, whether the robots left it (the criterion of
legged_gym-style curricula), fell or timed out first, and their height, foot clearance, stumbles and collisions on the way.  An
environment is measured for its first episode on its tile only.  No host read in the step loop; the host reads one small table.
"""
import numpy as np
import torch

from . import sweep
from .sweep import number

# the generator a tile of column choice `c` gets, in the order of the thresholds of go1_gym.utils.terrain.Terrain.make_terrain
# (cumulative terrain_proportions p[0], p[1], ...): below p[0] / 2, below p[0], below p[1], ...
TYPE_NAMES = ["slope_down", "slope_up", "rough_slope", "stairs_down", "stairs_up", "discrete_obstacles", "stepping_stones", "flat", "flat",
              "noise", "half_rough"]


# the configuration tree's own mix of slopes, rough slopes, stairs down, stairs up and discrete obstacles (legged_robot_config); the
# training configuration narrows it to flat ground with noise, on which every column would be the same tile
DEFAULT_PROPORTIONS = (0.1, 0.1, 0.35, 0.25, 0.2)


def terrain_cells(num_rows, num_cols):
    """[(level, type), ...] in row-major order: every tile of the grid once, the difficulty (row) outermost"""
    return [(level, kind) for level in range(int(num_rows)) for kind in range(int(num_cols))]


def terrain_type_name(kind, num_cols, terrain_proportions):
    """the generator of column `kind` of a curriculum grid: make_terrain's choice = kind / num_cols + 0.001 against the cumulative
    proportions, which make_terrain pads with infinity: the generator after the last proportion takes every remaining column"""
    choice = kind / num_cols + 0.001
    p = [float(np.sum(terrain_proportions[:i + 1])) for i in range(len(terrain_proportions))] + [np.inf] * 10
    for name, bound in zip(TYPE_NAMES, [p[0] / 2] + p):
        if choice < bound:
            return name
    return "flat"


def cell_difficulty(level, num_rows, difficulty_scale=1.0):
    """Terrain.curriculum's difficulty of row `level`"""
    return level / num_rows * difficulty_scale


def run_terrain_sweep(policy, preset, vx=1.0, num_envs=4096, window=500, warmup=25, seed=1, num_rows=4, num_cols=5, terrain_length=None,
                      terrain_width=None, mesh_type="trimesh", terrain_proportions=None):
    """One traversal table for one preset on a curriculum grid of num_rows difficulties x num_cols terrain types: environment i is
    placed on tile i % cells (its group), every robot is commanded `vx` m/s forward with zero yaw rate as a trot, and `window`
    steps are measured; steps with episode_length_buf <= warmup fold no metric.  terrain_length / terrain_width = None keep the
    training configuration's tile size; terrain_proportions = None is DEFAULT_PROPORTIONS.  Returns {"preset", "cells": [(level, type)], "terrain_type": [name per cell],
    "difficulty": [per cell], "metrics": {name: (cells, 6)}, "outcomes": {name: (cells, 6)}, "groups": (cells, 6) array of envs,
    running, traversed, fell, timed_out, success_rate, "status", "steps", "end_step", "max_dist": per environment, ...}."""
    def configure(cfg):
        t = cfg.terrain
        t.mesh_type, t.curriculum, t.selected, t.center_robots = mesh_type, True, False, False
        t.num_rows, t.num_cols = int(num_rows), int(num_cols)
        t.min_init_terrain_level, t.max_init_terrain_level = 0, int(num_rows) - 1
        t.measure_heights = True                             # the presets' terminal body height is then taken above the ground, not above z = 0
        if terrain_length is not None:
            t.terrain_length = float(terrain_length)
        if terrain_width is not None:
            t.terrain_width = float(terrain_width)
        t.terrain_proportions = list(DEFAULT_PROPORTIONS if terrain_proportions is None else terrain_proportions)
    cells = terrain_cells(num_rows, num_cols)
    env, cfg = sweep.build_eval_env(preset, num_envs, seed, configure=configure)
    if hasattr(policy, "eval"):
        policy.eval()
    base = env.env
    group = torch.arange(base.num_envs, device=base.device) % len(cells)
    table = torch.tensor(cells, dtype=torch.long)[group.cpu()]
    base.place_on_terrain(table[:, 0], table[:, 1])
    env.reset()                                              # every robot respawns on its tile, with an empty observation history
    commands = sweep.command_table([(float(vx), 0.0, sweep.GAITS["trotting"])], base.commands.shape[1], base.device).repeat(base.num_envs, 1)
    base.commands[:] = commands
    obs = env.get_observations()
    base.start_terrain_metrics(group.to(torch.int32), warmup_steps=warmup)
    sweep.rollout(env, policy, obs, window, commands)
    base.stop_terrain_metrics()
    if not sweep.commands_held(env, commands):
        raise RuntimeError("run_terrain_sweep: an environment left its commands during the rollout")
    res = base.read_terrain_metrics()
    t = cfg.terrain
    return dict(res, preset=preset, cells=cells, terrain_type=[terrain_type_name(k, t.num_cols, t.terrain_proportions) for _, k in cells],
                difficulty=[cell_difficulty(lv, t.num_rows, getattr(t, "difficulty_scale", 1.0)) for lv, _ in cells], vx=float(vx), num_envs=num_envs,
                window=window, warmup=warmup, seed=seed, num_rows=int(num_rows), num_cols=int(num_cols), mesh_type=mesh_type,
                tile=(float(t.terrain_length), float(t.terrain_width)), dt=float(base.dt))


def terrain_markdown_grid(result):
    """rows = difficulty, columns = terrain type; a cell reads success rate / stumble rate / mean swing foot height [m] / fall rate:
    traversed over the decided environments, the share of measured steps with a stumble, the mean height of the swinging feet's
    soles above the ground under them, and fell over the decided environments (– where nothing was measured)"""
    rows, cols = result["num_rows"], result["num_cols"]
    index = {cell: g for g, cell in enumerate(result["cells"])}
    head = ["difficulty"] + [f"{k}: {result['terrain_type'][index[(0, k)]]}" for k in range(cols)]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for level in range(rows):
        row = [f"{result['difficulty'][index[(level, 0)]]:.2f}"]
        for k in range(cols):
            g = index[(level, k)]
            row.append(" / ".join([number(result["groups"][g, 5], ".2f"), number(result["metrics"]["stumble"][g, 1], ".3f"),
                                   number(result["metrics"]["swing_foot_height"][g, 1], ".3f"), number(result["outcomes"]["fell"][g, 1], ".2f")]))
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def terrain_to_json(result):
    """the JSON form of a run_terrain_sweep result (without the per-environment arrays)"""
    keep = ("preset", "vx", "num_envs", "window", "warmup", "seed", "num_rows", "num_cols", "mesh_type", "dt")
    out = {k: result[k] for k in keep}
    out.update(tile=list(result["tile"]), fields=list(sweep.FIELDS),
               group_fields=["envs", "running", "traversed", "fell", "timed_out", "success_rate"],
               cells=[dict(level=lv, type=k, terrain_type=name, difficulty=d)
                      for (lv, k), name, d in zip(result["cells"], result["terrain_type"], result["difficulty"])],
               metrics={m: t.tolist() for m, t in result["metrics"].items()}, outcomes={m: t.tolist() for m, t in result["outcomes"].items()},
               groups=result["groups"].tolist(), status_counts=[int((result["status"] == k).sum()) for k in (0, 1, 2, 3)])
    return out
