"""Per-joint actuator usage: which joints sit on the torque clip or on the URDF's speed limit and how often, where in the
torque-speed plane each motor operates, how much of its power is braking, which joints lean on their soft position limits.

`joint_terms` is the host-side definition of the ten values libgo1eval's sixth kernel family folds per joint and step
(include/go1eval.h, the order of `enum Go1JointMetric`), as `[N, 12]` tensors on the environment's views: the analogue of
`metrics.SCALAR_METRICS`' functions.  Four of them summed over the joints are the reference's reward terms `_reward_torques`,
`_reward_dof_vel`, `_reward_dof_acc` and `_reward_dof_pos_limits`; tests/golden/joint_metrics.npz pins those sums bit for bit.  A sweep
does not call it per step: `run_joint_sweep` arms the device-side tables instead and reads them once at the end.
"""
import numpy as np
import torch

from . import sweep
from .sweep import number

JOINT_TERMS = ["torque_abs", "torque_sq", "vel_abs", "vel_sq", "acc_sq", "power_pos", "power_neg", "pos_limit_excess", "torque_saturated",
               "vel_saturated"]
DOF_VELOCITY = [50.0, 28.0, 28.0] * 4        # rad/s: the Go1 URDF's speed limits (go1sim_host._DOF_VELOCITY)
JOINT_TYPES = ["hip", "thigh", "calf"]       # joint j is JOINT_TYPES[j % 3] of leg j // 3


def joint_terms(env, prev_dof_vel=None, vel_limit=None, soft_torque_limit=1.0, soft_vel_limit=1.0):
    """{name: (N, 12) float32 tensor} of JOINT_TERMS from env.torques, env.dof_vel, env.dof_pos, env.dof_pos_limits ((12, 2): lower,
    upper), env.torque_limits and env.dt.  prev_dof_vel: the joint velocities one policy step earlier (default env.last_dof_vel, the
    reference's operand; the simulator here has already rolled it forward after a step, the device-side family keeps its own copy)."""
    tau, qd, q = env.torques, env.dof_vel, env.dof_pos
    prev = env.last_dof_vel if prev_dof_vel is None else prev_dof_vel
    speed = torch.as_tensor(DOF_VELOCITY if vel_limit is None else vel_limit, dtype=torch.float32, device=tau.device)
    power = tau * qd
    zero = torch.zeros_like(power)
    excess = -(q - env.dof_pos_limits[:, 0]).clip(max=0.)
    excess = excess + (q - env.dof_pos_limits[:, 1]).clip(min=0.)
    return dict(torque_abs=tau.abs(), torque_sq=torch.square(tau), vel_abs=qd.abs(), vel_sq=torch.square(qd),
                acc_sq=torch.square((prev - qd) / env.dt), power_pos=torch.where(power > 0, power, zero), power_neg=torch.where(power < 0, -power, zero),
                pos_limit_excess=excess, torque_saturated=(tau.abs() >= soft_torque_limit * env.torque_limits).float(),
                vel_saturated=(qd.abs() >= soft_vel_limit * speed).float())


def run_joint_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None):
    """One joint table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group), the
    scalar table armed beside it with the same groups and warm-up.  Returns {"preset", "cells", "joints": {name: (cells, 12, 6)},
    "joint_groups": (cells, 3) array of envs, steps, resets, "hist": (cells, 12, 8, 8), "tau_edges", "vel_edges": (12, 9),
    "metrics": the scalar table {name: (cells, 6)}, "groups": (cells, 5), "torque_limit", "vel_limit", "soft_torque_limit",
    "soft_vel_limit", ...}."""
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_joint_sweep", "joint", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain)
    c = base._joints.cfg
    return dict(preset=preset, cells=cells, joints=res["metrics"], joint_groups=res["groups"], hist=res["hist"], tau_edges=res["tau_edges"],
                vel_edges=res["vel_edges"], metrics=scalar, groups=groups, torque_limit=list(c.torque_limit), vel_limit=list(c.vel_limit),
                soft_torque_limit=float(c.soft_torque_limit), soft_vel_limit=float(c.soft_vel_limit), dof_names=list(base.dof_names),
                num_envs=num_envs, steps=steps, warmup_steps=warmup_steps, seed=seed, dt=float(base.dt))


def pool_cells(table):
    """one row per joint from a (cells, 12, 6) metric table, over every cell: count, mean, std, min, max, nonfinite of the pooled
    steps (the cells' population moments combined; a cell without a folded step adds nothing)"""
    t = np.asarray(table, np.float64)
    n = t[:, :, 0]
    mean, std = np.where(n > 0, t[:, :, 1], 0.0), np.where(n > 0, t[:, :, 2], 0.0)
    total = n.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        pooled = (n * mean).sum(axis=0) / total
        square = (n * (std * std + mean * mean)).sum(axis=0) / total
        lowest = np.where(n > 0, t[:, :, 3], np.inf).min(axis=0)
        highest = np.where(n > 0, t[:, :, 4], -np.inf).max(axis=0)
    nan = np.full_like(total, np.nan)
    some = total > 0
    return np.stack([total, pooled, np.sqrt(np.maximum(square - pooled * pooled, 0.0)), np.where(some, lowest, nan), np.where(some, highest, nan),
                     t[:, :, 5].sum(axis=0)], axis=1)


def joint_markdown_table(result):
    """one row per joint over every cell of the sweep: mean and max of |tau| [N m], share of steps at the torque limit, max of |qd|
    [rad/s], share at the speed limit, mean driving and braking power [W], rms acceleration [rad/s^2], and mean and max of the excess
    beyond a soft position limit [rad].  (The ten rows keep the excess, not a count of the steps with one: the share of steps beyond
    a limit is not in the table; a max of 0 says the joint never left its limits.)"""
    pooled = {name: pool_cells(t) for name, t in result["joints"].items()}
    head = ["joint", "mean |tau|", "max |tau|", "at torque limit", "max |qd|", "at speed limit", "driving power", "braking power", "rms acc",
            "mean limit excess", "max limit excess"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for j, name in enumerate(result["dof_names"]):
        row = [name, number(pooled["torque_abs"][j, 1], ".2f"), number(pooled["torque_abs"][j, 4], ".2f"), number(pooled["torque_saturated"][j, 1], ".4f"),
               number(pooled["vel_abs"][j, 4], ".2f"), number(pooled["vel_saturated"][j, 1], ".4f"), number(pooled["power_pos"][j, 1], ".2f"),
               number(pooled["power_neg"][j, 1], ".2f"), number(np.sqrt(pooled["acc_sq"][j, 1]), ".1f"), number(pooled["pos_limit_excess"][j, 1], ".4f"),
               number(pooled["pos_limit_excess"][j, 4], ".4f")]
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def joint_to_json(result):
    """the JSON form of a run_joint_sweep result"""
    keep = ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "dof_names", "torque_limit", "vel_limit", "soft_torque_limit", "soft_vel_limit")
    out = {k: result[k] for k in keep}
    out.update(cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS), group_fields=["envs", "steps", "resets"], joints={m: np.asarray(t).tolist() for m, t in result["joints"].items()},
               joint_groups=np.asarray(result["joint_groups"]).tolist(), hist=np.asarray(result["hist"]).tolist(),
               tau_edges=np.asarray(result["tau_edges"]).tolist(), vel_edges=np.asarray(result["vel_edges"]).tolist())
    return out


def plot_envelope(hist, path, torque_limit=33.5, vel_limit=(50.0, 28.0, 28.0), soft_torque_limit=1.0, soft_vel_limit=1.0):
    """The torque-speed envelope as a PNG: one 8 x 8 heat map per joint type (hip, thigh, calf) with the four legs (and every leading
    axis of `hist`, (..., 12, 8, 8) [joint][torque bin][speed bin]) summed, a logarithmic colour scale, and the limits drawn: the frame
    is the simulator's torque clip and the URDF's speed limit (samples beyond them are counted in the outermost bins), the dashed
    lines the soft limits the saturation shares are measured against."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    from matplotlib.colors import LogNorm
    h = np.asarray(hist, np.float64)
    h = h.reshape(-1, 4, 3, h.shape[-2], h.shape[-1]).sum(axis=(0, 1))              # [type][torque bin][speed bin]
    top = max(float(h.max()), 1.0)
    figure, axes = plt.subplots(ncols=3, figsize=(12, 4), constrained_layout=True)
    image = None
    for k, (ax, name) in enumerate(zip(axes, JOINT_TYPES)):
        speed = float(vel_limit[k])
        image = ax.imshow(np.ma.masked_equal(h[k], 0.0), origin="lower", extent=(-speed, speed, -torque_limit, torque_limit), aspect="auto",
                          norm=LogNorm(vmin=1.0, vmax=max(top, 2.0)), cmap="viridis", interpolation="nearest")
        for x in (-soft_vel_limit * speed, soft_vel_limit * speed):
            ax.axvline(x, color="r", linestyle="--", linewidth=1.0)
        for y in (-soft_torque_limit * torque_limit, soft_torque_limit * torque_limit):
            ax.axhline(y, color="r", linestyle="--", linewidth=1.0)
        ax.axhline(0.0, color="k", linewidth=0.5)
        ax.axvline(0.0, color="k", linewidth=0.5)
        ax.set(title=f"{name} joints, {int(h[k].sum())} samples", xlabel="joint speed [rad/s]", ylabel="torque [N m]" if k == 0 else "")
    figure.colorbar(image, ax=axes, label="steps")
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
