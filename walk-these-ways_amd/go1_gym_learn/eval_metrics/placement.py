"""Foot placement and stride geometry: where does every foot land against its nominal stance point and the Raibert heuristic's target,
how far does it sweep under the body in stance, and what stride length and track width does the robot realise under the commanded stance
width and length, speed and step frequency?

`placement_errors` is the host-side definition of the per-foot error libgo1place evaluates in fp32 (include/go1place.h): the feet minus
where `behaviour.raibert_heuristic` wants them, with the same torch operations, so its squares summed over feet and axes are that
metric's value bit for bit.  `run_placement_sweep` measures the placement table on the device over a product of command values
(`behaviour.behaviour_cells`), beside the scalar table, without a host read in the step loop; it does not call the host definition.
`placement_table`, `placement_to_json` and `plot_footprints` turn a result into the Markdown table, the JSON and the footprint figure.
"""
import numpy as np
import torch

from go1_gym.utils.math_utils import quat_apply_yaw, quat_conjugate

from . import behaviour, sweep
from .sweep import clean, number

FEET = ["FL", "FR", "RL", "RR"]
PLACEMENT_METRICS = ["stance_err_x", "stance_err_y", "swing_err_x", "swing_err_y", "touchdown_x", "touchdown_y", "touchdown_err_x", "touchdown_err_y",
                     "track_width_err", "stride_length", "stride_length_err", "liftoff_x", "liftoff_y", "stance_sweep"]     # enum Go1PlaceMetric
PLACEMENT_GROUP_FIELDS = ["envs", "steps", "resets", "touchdowns", "strides", "map_outside"]
DEFAULT_MAP_CELL = 0.03        # m: a placeholder, nothing measured stands behind it
X_SIGN, Y_SIGN = (1.0, 1.0, -1.0, -1.0), (1.0, -1.0, 1.0, -1.0)


def placement_errors(env):
    """(N, 4, 2) fp32: the feet in the yaw-aligned body frame minus where the Raibert heuristic puts them for the commanded stance width
    and length, velocity and step frequency (realised minus commanded), by the torch operations of behaviour.raibert_heuristic"""
    cmd = env.commands
    offset = env.foot_positions - env.root_states[:, 0:3].unsqueeze(1)
    inverse = quat_conjugate(env.root_states[:, 3:7])
    feet = torch.stack([quat_apply_yaw(inverse, offset[:, f, :]) for f in range(4)], dim=1)
    y_sign = torch.tensor(Y_SIGN, device=cmd.device)
    x_sign = torch.tensor(X_SIGN, device=cmd.device)
    num_commands = env.cfg.commands.num_commands
    if num_commands >= 13:
        width = cmd[:, 12:13]
        ys = torch.cat([width / 2, -width / 2, width / 2, -width / 2], dim=1)
    else:
        width = behaviour.DEFAULT_STANCE_WIDTH
        ys = (y_sign * (width / 2)).unsqueeze(0)
    if num_commands >= 14:
        length = cmd[:, 13:14]
        xs = torch.cat([length / 2, length / 2, -length / 2, -length / 2], dim=1)
    else:
        length = behaviour.DEFAULT_STANCE_LENGTH
        xs = (x_sign * (length / 2)).unsqueeze(0)
    phase = torch.abs(1.0 - env.foot_indices * 2.0) * 1.0 - 0.5
    half_period = 0.5 / cmd[:, 4].unsqueeze(1)
    y_offset = phase * (cmd[:, 2:3] * length / 2) * half_period
    y_offset[:, 2:4] *= -1
    x_offset = phase * cmd[:, 0:1] * half_period
    wanted = torch.stack((xs + x_offset, ys + y_offset), dim=2)
    return (feet[:, :, 0:2] - wanted).cpu()


def run_placement_sweep(policy, preset, axes, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None, map_cell=DEFAULT_MAP_CELL):
    """The placement table for one preset over the product of `axes` = {command name: [values]} (behaviour.behaviour_cells: stance_width,
    stance_length, vx, frequency, ...; environment i gets cell i % cells, its group), the scalar table armed beside it with the same
    groups and warm-up.  Returns {"preset", "cells": [{name: value}], "commands": (cells, num_commands) the cells' command vectors,
    "placement": {name: (cells, 4, 6)}, "placement_groups": (cells, 6) array of envs, steps, resets, touchdowns, strides, map_outside,
    "map": (cells, 4, 8, 8), "map_edges": (9,), "foot_counts": {"touchdowns", "strides", "map_outside": (cells, 4)}, "metrics": the scalar
    table {name: (cells, 6)}, "groups": (cells, 5), "map_cell", ...}."""
    cells = behaviour.behaviour_cells(axes)
    base, group, scalar, groups, res = sweep.run_beside_scalar("run_placement_sweep", "placement", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain,
                                                               dict(map_cell=map_cell), prepare_cells=behaviour.prepare, cell="cell")
    member = group.cpu().numpy()
    per_foot = lambda name: np.stack([res[name].view(np.uint32)[:, member == g].sum(axis=1).astype(np.float64) for g in range(len(cells))])
    table = behaviour.behaviour_command_table(cells, base.commands.shape[1], "cpu").numpy()
    return dict(preset=preset, cells=cells, commands=table, placement=res["metrics"], placement_groups=res["groups"], map=res["map"],
                map_edges=res["map_edges"], foot_counts={k: per_foot(k) for k in ("touchdowns", "strides", "map_outside")}, metrics=scalar,
                groups=groups, map_cell=float(map_cell), num_envs=num_envs, steps=steps, warmup_steps=warmup_steps, seed=seed, dt=float(base.dt))


def commanded(result, g):
    """what cell g asks for: {"width", "length", "stride_length" = |v| / f} from its command vector (the defaults where it is too short)"""
    cmd = np.asarray(result["commands"][g], np.float64)
    width = float(cmd[12]) if cmd.size >= 13 else behaviour.DEFAULT_STANCE_WIDTH
    length = float(cmd[13]) if cmd.size >= 14 else behaviour.DEFAULT_STANCE_LENGTH
    with np.errstate(all="ignore"):
        stride = float(np.hypot(cmd[0], cmd[1]) / cmd[4])
    return dict(width=width, length=length, stride_length=stride)


def _mean_std(row, fmt="+.3f"):
    return number(row[1], fmt) + " ± " + number(row[2], ".3f")


def placement_table(result):
    """the Markdown table: one row per cell and foot with the cell's command values, the commanded width / length, the touchdown point
    against the nominal stance point (x and y, mean +- std), the touchdown error against the heuristic's target, the mean stance and swing
    error per axis, the stance sweep, the stride length realised / commanded, the track width realised (width + track_width_err) /
    commanded, and the touchdowns, strides and the share of touchdowns outside the map"""
    names = list(result["cells"][0]) if result["cells"] else []
    head = names + ["foot", "width / length", "touchdown x", "touchdown y", "touchdown err x / y", "stance err x / y", "swing err x / y", "stance sweep",
                    "stride real / cmd", "track real / cmd", "touchdowns", "strides", "outside map"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    t = result["placement"]
    for g, cell in enumerate(result["cells"]):
        want = commanded(result, g)
        for f, foot in enumerate(FEET):
            row = lambda name: np.asarray(t[name][g][f], np.float64)
            touchdowns, strides, outside = (float(result["foot_counts"][k][g][f]) for k in ("touchdowns", "strides", "map_outside"))
            line = [f"{cell[n]:g}" for n in names] + [foot, f"{want['width']:.3f} / {want['length']:.3f}", _mean_std(row("touchdown_x")), _mean_std(row("touchdown_y")),
                    number(row("touchdown_err_x")[1], "+.3f") + " / " + number(row("touchdown_err_y")[1], "+.3f"),
                    number(row("stance_err_x")[1], "+.3f") + " / " + number(row("stance_err_y")[1], "+.3f"),
                    number(row("swing_err_x")[1], "+.3f") + " / " + number(row("swing_err_y")[1], "+.3f"), _mean_std(row("stance_sweep")),
                    number(row("stride_length")[1], ".3f") + " / " + number(want["stride_length"], ".3f"),
                    number(want["width"] + row("track_width_err")[1], ".3f") + " / " + f"{want['width']:.3f}",
                    f"{touchdowns:.0f}", f"{strides:.0f}", number(outside / touchdowns if touchdowns > 0 else float("nan"), ".3f")]
            lines.append("| " + " | ".join(line) + " |")
    return "\n".join(lines)


def placement_to_json(result):
    """the JSON form of a run_placement_sweep result (NaN and infinities as null)"""
    out = {k: result[k] for k in ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "map_cell")}
    out.update(cells=result["cells"], commanded=[clean(commanded(result, g)) for g in range(len(result["cells"]))], feet=list(FEET),
               fields=list(sweep.FIELDS), group_fields=list(PLACEMENT_GROUP_FIELDS),
               placement={m: clean(np.asarray(t).tolist()) for m, t in result["placement"].items()},
               placement_groups=np.asarray(result["placement_groups"]).tolist(), map=np.asarray(result["map"]).tolist(),
               map_edges=np.asarray(result["map_edges"]).tolist(), foot_counts={k: np.asarray(v).tolist() for k, v in result["foot_counts"].items()},
               metrics={k: clean(np.asarray(v).tolist()) for k, v in result["metrics"].items()}, groups=clean(np.asarray(result["groups"]).tolist()))
    return out


def plot_footprints(result, path):
    """The footprint figure as a PNG: one panel per cell in the body frame (x forward, y to the left), the four feet's 8 x 8 maps drawn at
    their nominal stance points with logarithmic counts, the nominal point as a cross and the mean touchdown as a dot."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import colors, pyplot as plt
    cells = result["cells"]
    edges = np.asarray(result["map_edges"], np.float64)
    columns = min(len(cells), 3) or 1
    rows = (len(cells) + columns - 1) // columns or 1
    figure, axes = plt.subplots(rows, columns, figsize=(4.2 * columns, 4.2 * rows), squeeze=False, constrained_layout=True)
    top = max(float(np.asarray(result["map"]).max()), 1.0)
    for g, cell in enumerate(cells):
        ax = axes[g // columns][g % columns]
        want = commanded(result, g)
        for f, foot in enumerate(FEET):
            x0, y0 = X_SIGN[f] * want["length"] / 2, Y_SIGN[f] * want["width"] / 2
            counts = np.asarray(result["map"][g][f], np.float64)              # [v][u]: v along y, u along x
            # the body frame drawn with x up and y to the left: the horizontal axis is -y
            ax.pcolormesh(-(y0 + edges), x0 + edges, np.ma.masked_equal(counts.T, 0.0), norm=colors.LogNorm(vmin=0.5, vmax=max(top, 1.0)), cmap="viridis")
            ax.plot([-y0], [x0], marker="+", color="black", markersize=10)
            tx, ty = result["placement"]["touchdown_x"][g][f][1], result["placement"]["touchdown_y"][g][f][1]
            if np.isfinite(tx) and np.isfinite(ty):
                ax.plot([-(y0 + ty)], [x0 + tx], marker="o", color="tab:red", markersize=4)
            ax.annotate(foot, (-y0, x0), textcoords="offset points", xytext=(8, 8), fontsize=7)
        ax.set_aspect("equal")
        ax.set(xlabel="-y [m] (right of the body ->)", ylabel="x [m] (forward)", title=", ".join(f"{k} {v:g}" for k, v in cell.items()))
        ax.title.set_fontsize(8)
        ax.grid(True, linewidth=0.3)
    for k in range(len(cells), rows * columns):
        axes[k // columns][k % columns].axis("off")
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
