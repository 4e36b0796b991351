"""Whole episodes: what return a policy collects, how long it stays up, how far it gets, how well it tracks its command over an episode,
and its survival curve.

`run_episode_sweep` arms the device-side tables (include/go1episode.h, libgo1episode.so) beside the scalar table over a command grid,
BEFORE the reset that starts the rollout, so that every environment's first episode is seen from its first step, and reads them once at
the end.  A sweep window is usually shorter than an episode, so most episodes are still open at its end: the device bins them by their
age, and `kaplan_meier` takes them as right-censored observations beside the episodes that fell and those that timed out (a time-out
is a censoring too: the robot was taken away standing).
"""
import math

import numpy as np

from . import sweep
from .sweep import clean, mean_std, number

EPISODE_METRICS = ["step_reward", "length", "fell", "length_fell", "return", "reward_rate", "lin_vel_err", "yaw_vel_err", "discounted_return",
                   "displacement", "path_length"]
EPISODE_GROUP_FIELDS = ["envs", "steps", "closed", "fell", "timed_out", "open", "cut", "unseen", "open_steps"]
BINS = 16


def kaplan_meier(fall, timeout, open):
    """The product-limit estimate of survival per length bin, in fp64.  fall, timeout, open: (..., bins) episodes per bin that fell, that
    timed out, and that were still open (by their age).  At risk in bin k is everything in the bins >= k of all three; S_k = the product
    over j <= k of (1 - fall_j / n_j), taken in ascending order; NaN from the first bin in which nobody is at risk.  S_k estimates the
    share of episodes that outlast bin k."""
    fall, timeout, open = (np.asarray(a, np.float64) for a in (fall, timeout, open))
    total = fall + timeout + open
    at_risk = np.cumsum(total[..., ::-1], axis=-1)[..., ::-1]
    out = np.full(fall.shape, np.nan)
    flat_fall, flat_risk, flat_out = fall.reshape(-1, fall.shape[-1]), at_risk.reshape(-1, fall.shape[-1]), out.reshape(-1, fall.shape[-1])
    for row in range(flat_fall.shape[0]):
        s = 1.0
        for k in range(flat_fall.shape[1]):
            if not flat_risk[row, k] > 0:
                break
            s = s * (1.0 - flat_fall[row, k] / flat_risk[row, k])
            flat_out[row, k] = s
    return flat_out.reshape(fall.shape)


def run_episode_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None, gamma=0.99, bin_steps=0):
    """One episode table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the scalar
    table armed beside it with the same groups and warm-up.  bin_steps = 0 means ceil(steps / 16): the sixteen bins span the window.
    Both tables are started before sweep.prepare()'s reset, so every environment's first episode is whole (which is why this sweep
    spells the rollout out instead of calling sweep.run_beside_scalar, which starts them after it).  Returns {"preset", "cells",
    "episodes": {name: (cells, 6)}, "episode_groups": (cells, 9) array of EPISODE_GROUP_FIELDS, "fall_hist", "timeout_hist", "open_hist":
    (cells, 16), "bin_edges": (17,) in steps, "survival": (cells, 16) kaplan_meier of the three, "gamma", "bin_steps", "metrics": the
    scalar table {name: (cells, 6)}, "groups": (cells, 5), ...}."""
    import torch
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    bin_steps = int(bin_steps) if bin_steps else max(1, int(math.ceil(steps / BINS)))
    env, _ = sweep.build_eval_env(preset, num_envs, seed, terrain)
    if hasattr(policy, "eval"):
        policy.eval()
    base = env.env
    group = (torch.arange(base.num_envs, device=base.device) % len(cells)).to(torch.int32)          # prepare()'s groups, known before it
    base.start_metrics(group, warmup_steps=warmup_steps)
    base.start_episode_metrics(group, warmup_steps=warmup_steps, gamma=gamma, bin_steps=bin_steps)
    obs, prepared, commands = sweep.prepare(env, cells)
    assert torch.equal(prepared.cpu(), group.cpu())
    sweep.rollout(env, policy, obs, steps, commands)
    base.stop_metrics()
    base.stop_episode_metrics()
    if not sweep.commands_held(env, commands):
        raise RuntimeError("run_episode_sweep: an environment left its grid cell's commands during the rollout")
    scalar = base.read_metrics()
    groups = scalar.pop("groups")
    res = base.read_episode_metrics()
    return dict(preset=preset, cells=cells, episodes=res["metrics"], episode_groups=res["groups"], fall_hist=res["fall_hist"],
                timeout_hist=res["timeout_hist"], open_hist=res["open_hist"], bin_edges=res["bin_edges"],
                survival=kaplan_meier(res["fall_hist"], res["timeout_hist"], res["open_hist"]), gamma=float(gamma), bin_steps=bin_steps,
                metrics=scalar, groups=groups, num_envs=num_envs, steps=steps, warmup_steps=warmup_steps, seed=seed, dt=float(base.dt))


def cell_summary(result, g):
    """what the table and the JSON say about cell g: {"closed", "open", "cut", "unseen", "fall_share": falls among the closed episodes,
    "time_to_fall_s": the mean length of the episodes that fell, in seconds, "survival_quarter", "survival_half", "survival_end": the
    Kaplan-Meier estimate after bins 3, 7 and 15, "steps_per_fall": env-steps per fall (NaN without one)}"""
    groups = dict(zip(EPISODE_GROUP_FIELDS, (float(x) for x in result["episode_groups"][g])))
    t = result["episodes"]
    s = np.asarray(result["survival"][g], np.float64)
    return dict(closed=groups["closed"], open=groups["open"], cut=groups["cut"], unseen=groups["unseen"],
                fall_share=float(t["fell"][g][1]), time_to_fall_s=float(t["length_fell"][g][1]) * float(result["dt"]),
                survival_quarter=float(s[BINS // 4 - 1]), survival_half=float(s[BINS // 2 - 1]), survival_end=float(s[BINS - 1]),
                steps_per_fall=groups["steps"] / groups["fell"] if groups["fell"] > 0 else float("nan"))


def episode_markdown_table(result):
    """one row per cell: the episodes closed / open / cut, the share of falls among the closed, return, length in steps, time to a fall
    in seconds, reward per step, discounted return, displacement and path length in metres, the two tracking errors (each mean +- std
    over the cell's closed episodes), the survival estimate after a quarter, a half and all of the binned range, and the env-steps
    per fall"""
    head = ["vx", "yaw", "gait", "closed / open / cut", "fall share", "return", "length", "time to fall [s]", "reward / step", "discounted return",
            "displacement [m]", "path [m]", "lin vel err", "yaw vel err", "S(1/4)", "S(1/2)", "S(end)", "env-steps / fall"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    t = result["episodes"]
    for g, (vx, yaw, gait) in enumerate(result["cells"]):
        s = cell_summary(result, g)
        row = [f"{vx:g}", f"{yaw:g}", "/".join(f"{x:g}" for x in gait), f"{s['closed']:.0f} / {s['open']:.0f} / {s['cut']:.0f}", number(s["fall_share"], ".3f"),
               mean_std(t["return"][g]), mean_std(t["length"][g]), number(s["time_to_fall_s"], ".2f")]
        row += [mean_std(t[m][g]) for m in ("reward_rate", "discounted_return", "displacement", "path_length", "lin_vel_err", "yaw_vel_err")]
        row += [number(s[k], ".3f") for k in ("survival_quarter", "survival_half", "survival_end")] + [number(s["steps_per_fall"], ".0f")]
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def episode_to_json(result):
    """the JSON form of a run_episode_sweep result (NaN and infinities as null)"""
    keep = ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "gamma", "bin_steps")
    out = {k: result[k] for k in keep}
    out.update(cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS), group_fields=list(EPISODE_GROUP_FIELDS),
               episodes={m: clean(np.asarray(t).tolist()) for m, t in result["episodes"].items()},
               episode_groups=np.asarray(result["episode_groups"]).tolist(), fall_hist=np.asarray(result["fall_hist"]).tolist(),
               timeout_hist=np.asarray(result["timeout_hist"]).tolist(), open_hist=np.asarray(result["open_hist"]).tolist(),
               bin_edges=clean(np.asarray(result["bin_edges"]).tolist()), survival=clean(np.asarray(result["survival"]).tolist()),
               summary=[clean(cell_summary(result, g)) for g in range(len(result["cells"]))])
    return out


def plot_survival(result, path):
    """The survival figure as a PNG: one Kaplan-Meier step curve per cell over the episode's age in seconds (1 at age 0, then the
    estimate after every bin, drawn to the bin's upper edge; the open-ended last bin is drawn one bin wide)."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    dt, width = float(result["dt"]), float(result["bin_steps"])
    edges = np.arange(BINS + 1) * width * dt
    figure, axes = plt.subplots(figsize=(7, 4), constrained_layout=True)
    for g, (vx, yaw, gait) in enumerate(result["cells"]):
        s = np.asarray(result["survival"][g], np.float64)
        axes.step(edges, np.concatenate([[1.0], s]), where="post", label=f"vx {vx:g}, yaw {yaw:g}, gait {'/'.join(f'{x:g}' for x in gait)}")
    axes.set(xlabel="age of the episode [s]", ylabel="share of episodes still up", ylim=(0.0, 1.05), xlim=(0.0, float(edges[-1])),
             title=f"{result['preset']}: Kaplan-Meier survival, open episodes censored")
    axes.grid(True, linewidth=0.3)
    axes.legend(fontsize=7)
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
