"""Disturbance recovery: shove the robot while it trots.  Does it fall, how far does it leave its command, how long until it is
back?

`run_push_sweep` holds one command for every environment, pushes environment i with cell `i % cells` of a grid of push
magnitudes and directions, and records the trace of libgo1eval (include/go1eval.h) around the push.  The push is one launch of
the library's fourth kernel family between two policy steps (a velocity step ADDED to the base velocity in the robot's heading
frame; the reference's training-time push replaces the velocity with a random draw and is switched off in every evaluation
preset), and the analysis (fall, peak velocity error, recovery time, height drop, yaw-rate deviation, integrated excess error
per environment, reduced per cell) runs on the device as well.  No host read in the step loop; the host reads one small table.
"""
import math

import numpy as np
import torch

from . import response, sweep


def push_cells(magnitudes, directions_deg):
    """[(magnitude in m/s, direction in degrees), ...] in row-major order of (magnitude, direction).  The direction is where the
    push drives the robot in its heading frame, counter-clockwise from forward seen from above: 0 is a shove from behind (a
    forward push), 90 a push to the left, 180 a shove from the front.  A magnitude of 0 is the control cell: nothing is pushed."""
    return [(float(m), float(d)) for m in magnitudes for d in directions_deg]


def push_table(cells, num_envs):
    """(num_envs, 4) float32 table for push_robots: environment i gets cell i % cells as a planar velocity step (forward, left),
    no vertical and no yaw-rate step.  The cosine and sine are taken here: the device does no trigonometry."""
    rows = np.zeros((len(cells), 4), np.float64)
    for i, (magnitude, direction) in enumerate(cells):
        a = math.radians(direction)
        rows[i, 0], rows[i, 1] = magnitude * math.cos(a), magnitude * math.sin(a)
    rows = np.round(rows, 12) + 0.0                          # cos(90 degrees) is 6e-17 in fp64: an exact zero, and no -0.0
    return rows[np.arange(num_envs) % len(cells)].astype(np.float32)


def run_push_sweep(policy, preset, magnitudes, directions, num_envs=4096, settle_steps=100, pre=25, window=150, smooth=None, band=0.1,
                   hold=10, seed=1, terrain=None, trace_envs=None, paired=False):
    """One recovery table for one preset: every environment holds response.BASE_CELL (a trot at 1 m/s) for settle_steps + pre
    steps, environment i is pushed once with cell i % cells, and `window` more steps follow; the trace covers the last
    pre + window steps and is analysed with push_row = pre.  smooth=None: one stride (response.stride_rows).  band: m/s of
    velocity error above the pre-push mean that counts as recovered; its default is a placeholder, not a measured figure.
    Returns {"preset", "cells": [(magnitude, direction)], "recovery": {metric: (cells, 6)}, "groups": (cells, 5) array of envs,
    ok, baseline reset, not held, fell, "values", "status", ...}; with trace_envs also "trace": read_trace() restricted to those
    environments.
    paired=True: the same robots, at the same instant, pushed once with every cell.  The first num_envs // cells environments are
    the sources; after settle_steps their state is saved (LeggedRobot.save_state) and loaded into all environments, environment i
    getting source i // cells and cell i % cells (the remainder beyond sources * cells is left unpushed, in group -1).  The
    result gains "source" ((num_envs,), -1 for the remainder) and, if the grid holds a magnitude-0 cell, "paired_excess": (cells, 3)
    mean, std and count of peak_vel_err(cell) - peak_vel_err(control) over the sources whose control and pushed environments both
    have status 0 (the control is the first magnitude-0 cell).  A copy keeps its own index: with observation noise or
    randomisation on the cadence enabled in the preset its draws after the load are its own."""
    cells = push_cells(magnitudes, directions)
    env, _ = sweep.build_eval_env(preset, num_envs, seed, terrain)
    if hasattr(policy, "eval"):
        policy.eval()
    base = env.env
    env.reset()
    group = torch.arange(base.num_envs, device=base.device) % len(cells)
    commands = sweep.command_table([response.BASE_CELL], base.commands.shape[1], base.device).repeat(base.num_envs, 1)
    w = response.stride_rows(commands[:1], base.dt) if smooth is None else int(smooth)
    if not 1 <= w <= pre + 1:
        raise ValueError(f"run_push_sweep: the filter of {w} rows needs pre >= {w - 1}")
    table = push_table(cells, base.num_envs)                 # on the host: push_robots checks it there and uploads it once
    base.commands[:] = commands
    obs = env.get_observations()
    obs = sweep.rollout(env, policy, obs, settle_steps, commands)
    source = None
    if paired:
        sources = base.num_envs // len(cells)
        if sources < 1:
            raise ValueError(f"run_push_sweep: paired needs at least one environment per cell ({len(cells)}), got {base.num_envs}")
        used = np.arange(sources * len(cells))
        source = np.where(np.arange(base.num_envs) < used.size, np.arange(base.num_envs) // len(cells), -1)
        group = torch.from_numpy(np.where(source >= 0, np.arange(base.num_envs) % len(cells), -1)).to(base.device)
        # (the observations `obs` are views of the simulator's buffers, and the rings keep their positions: they show the loaded state)
        base.load_state(base.save_state(np.arange(sources)), env_ids=used, rows=used // len(cells))
    base.start_trace(capacity=pre + window)
    obs = sweep.rollout(env, policy, obs, pre, commands)
    if source is None or used.size == base.num_envs:
        base.push_robots(table)
    else:
        base.push_robots(table[:used.size], used)
    sweep.rollout(env, policy, obs, window, commands)
    base.stop_trace()
    if not sweep.commands_held(env, commands):
        raise RuntimeError("run_push_sweep: an environment left its commands during the rollout")
    res = base.trace_recovery(push_row=pre, pre=pre, smooth=w, band=band, hold=hold, groups=group.to(torch.int32))
    out = dict(preset=preset, cells=cells, recovery={k: v for k, v in res.items() if k not in ("groups", "values", "status")},
               groups=res["groups"], values=res["values"], status=res["status"], num_envs=num_envs, settle_steps=settle_steps, pre=pre,
               window=window, smooth=w, band=band, hold=hold, dt=float(base.dt), seed=seed)
    if source is not None:
        out["source"] = source
        excess = paired_excess(cells, source, res["values"]["peak_vel_err"], res["status"])
        if excess is not None:
            out["paired_excess"] = excess
    if trace_envs is not None:
        out["trace"] = response.select_envs(base.read_trace(), trace_envs)
    return out


def paired_excess(cells, source, peak, status):
    """(cells, 3) float64 mean, std, count of peak[cell's environment] - peak[control's environment] over the sources of a paired sweep whose
    two environments both have status 0; None without a magnitude-0 cell.  Environment source * cells + g is source's copy for cell g."""
    control = next((g for g, (magnitude, _) in enumerate(cells) if magnitude == 0.0), None)
    if control is None:
        return None
    sources = int(source.max()) + 1
    peak = np.asarray(peak, dtype=np.float64)[:sources * len(cells)].reshape(sources, len(cells))
    good = (np.asarray(status)[:sources * len(cells)] == 0).reshape(sources, len(cells))
    out = np.full((len(cells), 3), np.nan)
    for g in range(len(cells)):
        both = good[:, g] & good[:, control]
        diff = peak[both, g] - peak[both, control]
        out[g] = [diff.mean() if diff.size else np.nan, diff.std() if diff.size else np.nan, diff.size]
    return out


def recovery_markdown_table(result):
    """one row per cell: ok / fell / baseline reset / not held, the fall rate fell / (ok + fell), then over the environments with
    status 0 mean +- std of the peak velocity error and of the recovery time (over those that recovered) and the recovered share"""
    r = result["recovery"]
    head = ["push [m/s]", "direction [deg]", "ok / fell / baseline reset / not held", "fall rate", "peak velocity error [m/s]",
            "recovery time [s]", "recovered"]
    excess = result.get("paired_excess")
    if excess is not None:
        head.append("paired excess peak error [m/s]")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, (magnitude, direction) in enumerate(result["cells"]):
        ok, spoiled, moved, fell = (int(x) for x in result["groups"][g, 1:5])
        row = [f"{magnitude:g}", f"{direction:g}", f"{ok} / {fell} / {spoiled} / {moved}", f"{fell / (ok + fell):.3f}" if ok + fell > 0 else "–"]
        row += [sweep.mean_std(r["peak_vel_err"][g]), sweep.mean_std(r["recovery_time"][g]), f"{r['recovered'][g, 1]:.3f}" if r["recovered"][g, 0] > 0 else "–"]
        if excess is not None:
            row.append(f"{excess[g][0]:.3g} ± {excess[g][1]:.2g} ({int(excess[g][2])})" if excess[g][2] > 0 else "–")
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def recovery_to_json(result):
    """the JSON form of a run_push_sweep result (without the per-environment values and the trace)"""
    keep = ("preset", "num_envs", "settle_steps", "pre", "window", "smooth", "band", "hold", "dt", "seed")
    out = {k: result[k] for k in keep}
    out.update(cells=[dict(magnitude=m, direction_deg=d) for m, d in result["cells"]], fields=list(sweep.FIELDS),
               group_fields=["envs", "ok", "baseline_reset", "not_held", "fell"],
               recovery={m: t.tolist() for m, t in result["recovery"].items()}, groups=result["groups"].tolist(),
               status_counts=[int((result["status"] == k).sum()) for k in (0, 1, 2, 3)])
    if "source" in result:
        out["paired"] = True
        out["source"] = np.asarray(result["source"]).tolist()
    if "paired_excess" in result:
        out["paired_excess_fields"] = ["mean", "std", "count"]
        out["paired_excess"] = [[None if np.isnan(v) else float(v) for v in row] for row in np.asarray(result["paired_excess"])]
    return out
