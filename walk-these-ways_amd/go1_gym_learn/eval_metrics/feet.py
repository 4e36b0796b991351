"""Foot loading: how hard each foot lands, the peak vertical load of a stance, how much of the available friction the gait uses, how
far a loaded foot slides, how the load is shared between the feet, and the ground-reaction-force (GRF) curve over the gait cycle.

`foot_terms` is the host-side definition of the per-step values libgo1feet folds per foot (include/go1feet.h, the order of
`enum Go1FeetMetric`), as `[N, 4]` tensors on the environment's views, written the way the reference writes its terms.  Two of them
summed over the feet are the reference's reward terms `_reward_feet_contact_forces` and `_reward_feet_impact_vel`;
tests/golden/foot_metrics.npz pins those sums bit for bit.  The stance rows need the per-foot state and have no stateless form.  A
sweep does not call it per step: `run_foot_sweep` arms the device-side tables instead and reads them once at the end.
"""
import os
import re

import numpy as np
import torch

from . import sweep
from .sweep import number

FOOT_TERMS = ["contact", "force_normal", "force_tangent", "friction_use", "force_excess", "impact_vel_sq", "touchdown_speed", "touchdown_force"]
FEET_METRICS = FOOT_TERMS + ["stance_peak_force", "stance_impulse", "stance_slip", "stance_time"]
FOOT_NAMES = ["FL", "FR", "RL", "RR"]
GRAVITY = 9.81
_MODEL_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "csrc", "go1_model_data.h")


def total_mass(path=_MODEL_DATA):
    """kg: the sum of the model data's body masses (csrc/go1_model_data.h GO1_BODY_MASS), without payload"""
    text = open(path).read()
    body = re.search(r"GO1_BODY_MASS\[\d+\]\s*=\s*\{([^}]*)\}", text).group(1)
    return float(sum(float(v) for v in body.split(",")))


def foot_terms(env, terrain_friction=1.0, max_contact_force=None):
    """{name: (N, 4) float32 tensor} of FOOT_TERMS from env.contact_forces ((N, 17, 3)), env.feet_indices, env.foot_velocities,
    env.prev_foot_velocities ((N, 4, 3)) and env.friction_coeffs ((N, 4) or (N, 1)).  The rows folded only on some steps (the three
    gated by contact, the two of a touchdown) are given for every foot; "contact" says where the first three count.
    max_contact_force: default env.cfg.rewards.max_contact_force."""
    limit = env.cfg.rewards.max_contact_force if max_contact_force is None else max_contact_force
    forces = env.contact_forces[:, env.feet_indices, :]
    norm = torch.norm(forces, dim=-1)
    fz = forces[:, :, 2]
    tangent = torch.norm(forces[:, :, :2], dim=-1)
    pvz = env.prev_foot_velocities[:, :, 2].view(env.num_envs, -1)
    terms = dict(contact=(fz > 1.0).float(), force_normal=fz, force_tangent=tangent, force_excess=(norm - limit).clip(min=0.),
                 impact_vel_sq=(norm > 1.0) * torch.square(torch.clip(pvz, -100, 0)), touchdown_speed=(-pvz).clip(min=0.), touchdown_force=fz)
    friction = getattr(env, "friction_coeffs", None)
    if friction is not None:
        mu = 0.5 * (friction + terrain_friction)
        terms["friction_use"] = tangent / (mu * fz)
    return {name: terms[name] for name in FOOT_TERMS if name in terms}


def run_foot_sweep(policy, preset, grid=None, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None):
    """One foot-loading table for one preset over a command grid (as sweep.run_sweep; environment i gets cell i % cells, its group),
    the scalar table armed beside it with the same groups and warm-up.  Returns {"preset", "cells", "feet": {name: (cells, 4, 6)},
    "feet_groups": (cells, 3) array of envs, steps, resets, "profile", "profile_count": (cells, 4, 16), "phase_edges": (17,),
    "metrics": the scalar table {name: (cells, 6)}, "groups": (cells, 5), "body_weight": N, the model's total mass plus the mean
    payload times g, "terrain_friction", "max_contact_force", ...}."""
    cells = sweep.grid_cells(grid or sweep.DEFAULT_GRID)
    base, _, scalar, groups, res = sweep.run_beside_scalar("run_foot_sweep", "foot", policy, preset, cells, num_envs, steps, warmup_steps, seed, terrain)
    c = base._feet.cfg
    mass = total_mass() + float(base.payloads.mean())
    return dict(preset=preset, cells=cells, feet=res["metrics"], feet_groups=res["groups"], profile=res["profile"],
                profile_count=res["profile_count"], phase_edges=res["phase_edges"], metrics=scalar, groups=groups, body_weight=mass * GRAVITY,
                terrain_friction=float(c.terrain_friction), max_contact_force=float(c.max_contact_force), foot_names=list(FOOT_NAMES),
                num_envs=num_envs, steps=steps, warmup_steps=warmup_steps, seed=seed, dt=float(base.dt))


def load_shares(profile, profile_count):
    """(cells, 4) share of the total vertical load each foot carries: its mean force over every sampled step (the profile's sums over
    its counts, all bins together) over the four feet's sum; NaN for a cell that sampled nothing"""
    p, n = np.asarray(profile, np.float64), np.asarray(profile_count, np.float64)
    total = np.where(n > 0, p * n, 0.0).sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / n.sum(axis=2)
        return mean / mean.sum(axis=1, keepdims=True)


def foot_markdown_table(result):
    """one row per cell and foot: duty factor, mean and peak vertical force (over every loaded step) in N and in body weights, mean and
    max friction use, mean and max touchdown speed [m/s], impulse [N s] and slip [m] per stance, the foot's share of the total vertical
    load, and the front and the left feet's share of the cell (on the row of the cell's first foot)"""
    feet, weight = result["feet"], result["body_weight"]
    shares = load_shares(result["profile"], result["profile_count"])
    head = ["vx", "yaw", "foot", "duty", "mean Fz [N]", "mean Fz [BW]", "peak Fz [N]", "peak Fz [BW]", "mean friction use", "max friction use",
            "mean touchdown speed", "max touchdown speed", "impulse / stance", "slip / stance", "load share", "front", "left"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, cell in enumerate(result["cells"]):
        front, left = shares[g, 0] + shares[g, 1], shares[g, 0] + shares[g, 2]
        for f, foot in enumerate(result["foot_names"]):
            at = lambda name, field: feet[name][g][f][field]
            peak = at("force_normal", 4)
            row = [f"{cell[0]:g}", f"{cell[1]:g}", foot, number(at("contact", 1), ".3f"), number(at("force_normal", 1), ".1f"),
                   number(at("force_normal", 1) / weight, ".3f"), number(peak, ".1f"), number(peak / weight, ".3f"),
                   number(at("friction_use", 1), ".3f"), number(at("friction_use", 4), ".3f"), number(at("touchdown_speed", 1), ".3f"),
                   number(at("touchdown_speed", 4), ".3f"), number(at("stance_impulse", 1), ".2f"), number(at("stance_slip", 1), ".4f"),
                   number(shares[g, f], ".3f"), number(front, ".3f") if f == 0 else "", number(left, ".3f") if f == 0 else ""]
            lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def foot_to_json(result):
    """the JSON form of a run_foot_sweep result (NaN as null)"""
    clean = lambda a: [clean(x) for x in a] if isinstance(a, list) else (a if a == a else None)
    keep = ("preset", "num_envs", "steps", "warmup_steps", "seed", "dt", "foot_names", "body_weight", "terrain_friction", "max_contact_force")
    out = {k: result[k] for k in keep}
    out.update(cells=sweep.cells_to_json(result["cells"]), fields=list(sweep.FIELDS), group_fields=["envs", "steps", "resets"], feet={m: clean(np.asarray(t).tolist()) for m, t in result["feet"].items()},
               feet_groups=np.asarray(result["feet_groups"]).tolist(), profile=clean(np.asarray(result["profile"]).tolist()),
               profile_count=np.asarray(result["profile_count"]).tolist(), phase_edges=np.asarray(result["phase_edges"]).tolist(),
               load_share=clean(load_shares(result["profile"], result["profile_count"]).tolist()))
    return out


def plot_grf(result, path):
    """The GRF profile as a PNG: one panel per cell, the four feet's mean vertical force [body weights] over the phase of the commanded
    gait cycle (a foot in the air counts its 0)."""
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    profile = np.asarray(result["profile"], np.float64) / result["body_weight"]
    edges = np.asarray(result["phase_edges"], np.float64)
    centres = 0.5 * (edges[:-1] + edges[1:])
    cells = result["cells"]
    figure, axes = plt.subplots(ncols=len(cells), figsize=(4 * len(cells), 3.5), constrained_layout=True, squeeze=False, sharey=True)
    for g, (ax, cell) in enumerate(zip(axes[0], cells)):
        for f, foot in enumerate(result["foot_names"]):
            ax.plot(centres, profile[g, f], marker="o", markersize=3, label=foot)
        ax.set(title=f"vx {cell[0]:g} m/s, yaw {cell[1]:g} rad/s", xlabel="gait phase (foot_indices)", xlim=(0.0, 1.0),
               ylabel="mean vertical force [body weights]" if g == 0 else "")
        ax.grid(True, linewidth=0.3)
    axes[0][0].legend()
    figure.savefig(path, format="png", dpi=100)
    plt.close(figure)
