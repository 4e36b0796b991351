"""The step reward taken apart: per command cell, which reward terms pay, which cost, what share of the total each carries, and how
much negative reward the clip (`only_positive_rewards`, or the ji22 rule) forgives.

The step kernel evaluates the terms, adds them to `episode_sums` and stores the clipped total; libgo1reward (include/go1reward.h)
evaluates the terms of every step once more with the step kernel's own device functions and folds them per environment.
`run_reward_sweep` arms that table beside the scalar one over the velocity grid of `sweep.run_sweep` and reads both once at the end;
nothing in the step loop reads from the device.
"""
import numpy as np

from . import sweep
from .sweep import clean, number

EXTRA_ROWS = ("sum", "positive", "negative", "total")
GROUP_FIELDS = ["envs", "measured", "reset", "teleported"]


def run_reward_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None):
    """One reward table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the
    scalar table armed beside it with the same groups and warm-up.  Returns {"preset", "cells", "names": [K], "scales": (K,),
    "terms": {name: (cells, 6)}, "sum" / "positive" / "negative" / "total": (cells, 6), "share": {name: (cells,)}, "reward_groups":
    (cells, 4) array of envs, measured, reset, teleported env-steps, "metrics": the scalar table, "groups": (cells, 5), ...}."""
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_reward_sweep", "reward", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain)
    out = dict(preset=preset, cells=cells, names=res["names"], scales=res["scales"], terms=res["terms"], share=res["share"],
               reward_groups=res["groups"], metrics=scalar, groups=groups, num_envs=num_envs, steps=steps, warmup_steps=warmup_steps, seed=seed,
               dt=float(base.dt))
    out.update({row: res[row] for row in EXTRA_ROWS})
    return out


def forgiven(result):
    """(cells,) mean of total minus mean of sum: what the clip forgave per measured step (both rows count the same steps)"""
    return np.asarray(result["total"], np.float64)[:, 1] - np.asarray(result["sum"], np.float64)[:, 1]


def reward_table(result):
    """Markdown: one row per term and one column per cell, each cell the mean scaled reward per step and its share (mean_k over the sum
    of the |mean_j|); below the terms the rows sum, positive, negative, total, forgiven by the clip, and the measured / reset /
    teleported env-steps"""
    cells = result["cells"]
    head = ["term", "scale"] + [f"vx {c[0]:g}, yaw {c[1]:g}" for c in cells]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for k, name in enumerate(result["names"]):
        row = [name, f"{float(result['scales'][k]):.3g}"]
        for g in range(len(cells)):
            share = result["share"][name][g]
            row.append(f"{number(result['terms'][name][g][1], '.4g')} ({number(100.0 * share, '+.1f')} %)")
        lines.append("| " + " | ".join(row) + " |")
    for name in EXTRA_ROWS:
        lines.append("| " + " | ".join([f"**{name}**", ""] + [number(result[name][g][1], ".4g") for g in range(len(cells))]) + " |")
    gone = forgiven(result)
    lines.append("| " + " | ".join(["**forgiven by the clip**", ""] + [number(gone[g], ".4g") for g in range(len(cells))]) + " |")
    for f, name in enumerate(GROUP_FIELDS[1:], start=1):
        lines.append("| " + " | ".join([f"{name} env-steps", ""] + [f"{result['reward_groups'][g][f]:.0f}" for g in range(len(cells))]) + " |")
    return "\n".join(lines)


def reward_to_json(result):
    """the JSON form of a run_reward_sweep result (NaN and infinities as null)"""
    table = lambda t: clean(np.asarray(t, np.float64).tolist())
    out = {k: result[k] for k in ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt")}
    out.update(cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS), group_fields=list(GROUP_FIELDS), names=list(result["names"]), scales=table(result["scales"]),
               terms={n: table(t) for n, t in result["terms"].items()}, share={n: table(t) for n, t in result["share"].items()},
               reward_groups=table(result["reward_groups"]), forgiven=table(forgiven(result)))
    out.update({row: table(result[row]) for row in EXTRA_ROWS})
    return out


def plot_reward_shares(result, path):
    """One stacked bar per cell as a PNG: the terms' mean scaled rewards per step, positive terms upwards and negative ones downwards
    from 0, and the (clipped) total as a marker."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    cells, names = result["cells"], list(result["names"])
    means = np.nan_to_num(np.array([[result["terms"][n][g][1] for n in names] for g in range(len(cells))], np.float64))
    figure, ax = plt.subplots(figsize=(max(6.0, 1.6 * len(cells) + 4.0), 5.0), constrained_layout=True)
    colours = plt.get_cmap("tab20")(np.arange(len(names)) % 20)
    x = np.arange(len(cells))
    up, down = np.zeros(len(cells)), np.zeros(len(cells))
    for k, name in enumerate(names):
        v = means[:, k]
        bottom = np.where(v >= 0, up, down)
        ax.bar(x, v, bottom=bottom, color=colours[k], edgecolor="black", linewidth=0.3, label=name)
        up, down = up + np.where(v >= 0, v, 0.0), down + np.where(v < 0, v, 0.0)
    total = np.array([result["total"][g][1] for g in range(len(cells))], np.float64)
    ax.plot(x, total, linestyle="none", marker="D", color="black", markersize=7, label="total (after the clip)")
    ax.axhline(0.0, color="black", linewidth=0.6)
    ax.set(xticks=x, xticklabels=[f"vx {c[0]:g}\nyaw {c[1]:g}" for c in cells], ylabel="mean scaled reward per step", title=f"{result['preset']}: reward by term")
    ax.grid(True, axis="y", linewidth=0.3)
    ax.legend(fontsize=7, ncol=2, loc="center left", bbox_to_anchor=(1.0, 0.5))
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
