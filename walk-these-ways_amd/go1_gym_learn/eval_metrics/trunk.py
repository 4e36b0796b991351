"""Trunk motion: how far the trunk rolls and pitches and how fast, what acceleration an IMU or a payload on it would see, whether the
base is over the polygon of the supporting feet and how close to its edge, and whether the robot walks the straight line it is commanded.

`trunk_terms` is the host-side definition of the stateless per-step values libgo1trunk folds (include/go1trunk.h), as `[N]` tensors
on the environment's views, written the way the reference writes its terms.  Three of them are the reference's reward terms
`_reward_orientation`, `_reward_lin_vel_z` and `_reward_ang_vel_xy`; tests/golden/trunk_metrics.npz pins them bit for bit.  The
accelerations, the support rows and the drift segments need per-environment state or the feet and have no form here.  A sweep does not
call it per step: `run_trunk_sweep` arms the device-side tables instead and reads them once at the end.
"""
import numpy as np
import torch

from . import sweep
from .sweep import clean, number

TRUNK_TERMS = ["roll_sin", "pitch_sin", "tilt", "roll_rate", "pitch_rate", "vertical_vel", "orientation", "lin_vel_z", "ang_vel_xy"]
TRUNK_METRICS = ["roll_sin", "pitch_sin", "tilt", "tilt_exceeded", "roll_rate", "pitch_rate", "vertical_vel", "accel_horizontal", "accel_vertical",
                 "ang_accel", "support_feet", "support_margin", "margin_negative", "support_line_dist", "lateral_drift", "heading_drift",
                 "progress_err"]
GRAVITY = 9.81


def trunk_terms(env):
    """{name: (N,) float32 tensor} of TRUNK_TERMS from env.projected_gravity, env.base_lin_vel and env.base_ang_vel ((N, 3)).  The last
    three are the reference's reward terms: orientation = tilt squared before the root is taken, lin_vel_z = vertical_vel squared,
    ang_vel_xy = roll_rate squared + pitch_rate squared"""
    orientation = torch.sum(torch.square(env.projected_gravity[:, :2]), dim=1)
    lin_vel_z = torch.square(env.base_lin_vel[:, 2])
    ang_vel_xy = torch.sum(torch.square(env.base_ang_vel[:, :2]), dim=1)
    return dict(roll_sin=env.projected_gravity[:, 1], pitch_sin=env.projected_gravity[:, 0], tilt=torch.sqrt(orientation),
                roll_rate=env.base_ang_vel[:, 0], pitch_rate=env.base_ang_vel[:, 1], vertical_vel=env.base_lin_vel[:, 2],
                orientation=orientation, lin_vel_z=lin_vel_z, ang_vel_xy=ang_vel_xy)


def run_trunk_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None, segment_steps=50, tilt_limit=0.25):
    """One trunk table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the scalar
    table armed beside it with the same groups and warm-up.  Returns {"preset", "cells", "trunk": {name: (cells, 6)}, "trunk_groups":
    (cells, 4) array of envs, steps, resets, segments_dropped, "tilt_hist": (cells, 16), "tilt_edges": (17,), "metrics": the scalar table
    {name: (cells, 6)}, "groups": (cells, 5), "segment_steps", "tilt_limit", ...}."""
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_trunk_sweep", "trunk", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain,
                                                           dict(segment_steps=segment_steps, tilt_limit=tilt_limit))
    return dict(preset=preset, cells=cells, trunk=res["metrics"], trunk_groups=res["groups"], tilt_hist=res["tilt_hist"], tilt_edges=res["tilt_edges"],
                metrics=scalar, groups=groups, segment_steps=int(segment_steps), tilt_limit=float(tilt_limit), num_envs=num_envs, steps=steps,
                warmup_steps=warmup_steps, seed=seed, dt=float(base.dt))


def _rms(row):
    """the root mean square of a metric row (count, mean, std, ...): sqrt(std^2 + mean^2)"""
    return float(np.sqrt(row[2] * row[2] + row[1] * row[1]))


def _degrees(sine):
    """the angle of a sine in degrees, for display (a sine beyond 1 by rounding is clipped)"""
    return float(np.degrees(np.arcsin(np.clip(sine, -1.0, 1.0)))) if np.isfinite(sine) else float("nan")


def trunk_markdown_table(result):
    """one row per cell: mean and max tilt [deg], the share of steps beyond the limit, rms roll and pitch rate [rad/s], rms vertical
    velocity [m/s], rms and peak horizontal and vertical acceleration [g], the mean number of supporting feet, the mean margin [m] and
    the share of negative margins, the mean line distance [m], and per segment the lateral drift [m], the heading drift [deg] and the
    progress error [m] with the segments folded and dropped"""
    t = result["trunk"]
    head = ["vx", "yaw", "mean tilt [deg]", "max tilt [deg]", "beyond limit", "rms roll rate", "rms pitch rate", "rms vz", "rms a_h [g]", "peak a_h [g]",
            "rms a_v [g]", "peak a_v [g]", "feet", "mean margin [m]", "margin < 0", "mean line dist [m]", "lateral drift [m]", "heading drift [deg]",
            "progress err [m]", "segments", "dropped"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, cell in enumerate(result["cells"]):
        at = lambda name: np.asarray(t[name][g], np.float64)
        peak_v = max(abs(at("accel_vertical")[3]), abs(at("accel_vertical")[4])) if at("accel_vertical")[0] > 0 else float("nan")
        row = [f"{cell[0]:g}", f"{cell[1]:g}", number(_degrees(at("tilt")[1]), ".2f"), number(_degrees(at("tilt")[4]), ".2f"),
               number(at("tilt_exceeded")[1], ".4f"), number(_rms(at("roll_rate")), ".3f"), number(_rms(at("pitch_rate")), ".3f"),
               number(_rms(at("vertical_vel")), ".3f"), number(_rms(at("accel_horizontal")) / GRAVITY, ".3f"),
               number(at("accel_horizontal")[4] / GRAVITY, ".3f"), number(_rms(at("accel_vertical")) / GRAVITY, ".3f"), number(peak_v / GRAVITY, ".3f"),
               number(at("support_feet")[1], ".2f"), number(at("support_margin")[1], ".4f"), number(at("margin_negative")[1], ".4f"),
               number(at("support_line_dist")[1], ".4f"), number(at("lateral_drift")[1], ".4f"), number(_degrees(at("heading_drift")[1]), ".2f"),
               number(at("progress_err")[1], ".4f"), f"{at('lateral_drift')[0] + at('lateral_drift')[5]:.0f}", f"{result['trunk_groups'][g][3]:.0f}"]
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def trunk_to_json(result):
    """the JSON form of a run_trunk_sweep result (NaN and infinities as null)"""
    keep = ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "segment_steps", "tilt_limit")
    out = {k: result[k] for k in keep}
    out.update(cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS), group_fields=["envs", "steps", "resets", "segments_dropped"], trunk={m: clean(np.asarray(t).tolist()) for m, t in result["trunk"].items()},
               trunk_groups=np.asarray(result["trunk_groups"]).tolist(), tilt_hist=np.asarray(result["tilt_hist"]).tolist(),
               tilt_edges=clean(np.asarray(result["tilt_edges"]).tolist()))
    return out


def plot_tilt(result, path):
    """The tilt histogram as a PNG: one panel per cell, the count of steps per tilt bin (the bins are sines; the axis is labelled in
    degrees) on a logarithmic scale, the limit drawn."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    hist = np.asarray(result["tilt_hist"], np.float64)
    edges = np.asarray(result["tilt_edges"], np.float64).copy()
    width = edges[1] - edges[0]
    edges[-1] = edges[-2] + width                                            # the open last bin is drawn one bin wide
    angle = np.degrees(np.arcsin(np.clip(edges, 0.0, 1.0)))
    cells = result["cells"]
    figure, axes = plt.subplots(ncols=len(cells), figsize=(4 * len(cells), 3.5), constrained_layout=True, squeeze=False, sharey=True)
    for g, (ax, cell) in enumerate(zip(axes[0], cells)):
        ax.bar(angle[:-1], np.maximum(hist[g], 0.5), width=np.diff(angle), align="edge", edgecolor="black", linewidth=0.3)
        ax.axvline(_degrees(result["tilt_limit"]), color="red", linewidth=1.0, label="tilt limit")
        ax.set(title=f"vx {cell[0]:g} m/s, yaw {cell[1]:g} rad/s", xlabel="tilt [degrees]; the last bin is open", yscale="log",
               ylabel="steps" if g == 0 else "")
        ax.grid(True, linewidth=0.3)
    axes[0][0].legend()
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
