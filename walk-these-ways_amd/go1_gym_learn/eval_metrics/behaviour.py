"""Gait and behaviour tracking: does a policy do what the commands beyond the velocity ask (body height, step frequency, gait,
duty factor, foot-swing height, pitch and roll, stance width and length)?

`BEHAVIOUR_FNS` are the host-side definitions of the seven per-step values libgo1eval's behaviour kernel evaluates per
environment in fp32 (include/go1eval.h, the first seven of `enum Go1BehaviourMetric`), each `fn(env, actor_critic, obs)` on the
environment's `[N, k]` views as `metrics.METRICS_FNS`; six of them are the values of the reference's CoRLRewards terms, and
tests/golden/behaviour_metrics.npz pins them to what the reference's methods return.  `StrideTracker` restates the rules of the
three per-stride values.  `run_behaviour_sweep` measures both tables on the device over a product of command values, without
a host read in the step loop; it does not call the host definitions.
"""
import itertools

import numpy as np
import torch

from go1_gym.utils.math_utils import quat_apply_yaw, quat_conjugate, quat_from_angle_axis, quat_mul, quat_rotate_inverse

from . import sweep

CONTACT_FORCE = 1.0        # N: a foot is in contact when its F_z exceeds this
FOOT_RADIUS = 0.02         # m
DEFAULT_STANCE_WIDTH, DEFAULT_STANCE_LENGTH = 0.3, 0.45      # m, when the command vector is too short to carry them

# the order of include/go1eval.h `enum Go1BehaviourMetric`
PER_STEP = ["contact_match", "body_height_err", "orientation_err", "feet_clearance", "raibert_heuristic", "feet_slip", "action_rate"]
PER_STRIDE = ["step_frequency_err", "duty_factor_err", "swing_height_err"]
BEHAVIOUR_NAMES = PER_STEP + PER_STRIDE

# name -> column of the command vector
COMMAND_INDEX = dict(vx=0, vy=1, yaw=2, body_height=3, frequency=4, phase=5, offset=6, bound=7, duration=8, footswing_height=9,
                     pitch=10, roll=11, stance_width=12, stance_length=13)


def foot_contacts(env):
    """(N, 4) bool: F_z > 1 N"""
    return env.contact_forces[:, env.feet_indices, 2] > CONTACT_FORCE


def contact_match(env, actor_critic=None, obs=None):
    """share of the four feet whose measured contact equals the commanded contact schedule (tools/play_eval.py's figure)"""
    return (foot_contacts(env) == (env.desired_contact_states > 0.5)).float().mean(dim=1).cpu()


def body_height_err(env, actor_critic=None, obs=None):
    """base height above the mean measured terrain height, minus the commanded one (signed)"""
    height = (env.root_states[:, 2].unsqueeze(1) - env.measured_heights).mean(dim=1)
    return (height - (env.commands[:, 3] + env.cfg.rewards.base_height_target)).cpu()


def orientation_err(env, actor_critic=None, obs=None):
    """|xy difference| of the down vector seen from the base and seen from the commanded attitude (roll about x, then pitch
    about y, both negated: the reference's composition).  From the quaternion, so a randomised gravity is no attitude error."""
    N = env.commands.shape[0]
    down = torch.tensor([0.0, 0.0, -1.0], device=env.commands.device).repeat(N, 1)
    about_x = quat_from_angle_axis(-env.commands[:, 11], torch.tensor([1.0, 0.0, 0.0], device=down.device))
    about_y = quat_from_angle_axis(-env.commands[:, 10], torch.tensor([0.0, 1.0, 0.0], device=down.device))
    wanted = quat_rotate_inverse(quat_mul(about_x, about_y), down)
    seen = quat_rotate_inverse(env.root_states[:, 3:7], down)
    squared = torch.sum(torch.square(seen[:, :2] - wanted[:, :2]), dim=1)
    # the root is taken in fp64 and rounded to fp32 once: the correctly rounded fp32 root (which the kernel's sqrtf is), whatever
    # the host's vectorised fp32 root does in the last bit
    return squared.double().sqrt().float().cpu()


def feet_clearance(env, actor_critic=None, obs=None):
    """squared miss of the commanded swing height along the swing, feet in commanded stance excluded; world z: flat ground"""
    swing_phase = 1 - torch.abs(1.0 - torch.clip(env.foot_indices * 2.0 - 1.0, 0.0, 1.0) * 2.0)
    target = env.commands[:, 9].unsqueeze(1) * swing_phase + FOOT_RADIUS
    miss = torch.square(target - env.foot_positions[:, :, 2]) * (1 - env.desired_contact_states)
    return miss.sum(dim=1).cpu()


def raibert_heuristic(env, actor_critic=None, obs=None):
    """squared distance of the feet (yaw-aligned body frame) from where the Raibert heuristic puts them for the commanded
    stance width and length, velocity and step frequency"""
    N, cmd = env.commands.shape[0], env.commands
    offset = env.foot_positions - env.root_states[:, 0:3].unsqueeze(1)
    inverse = quat_conjugate(env.root_states[:, 3:7])
    feet = torch.stack([quat_apply_yaw(inverse, offset[:, f, :]) for f in range(4)], dim=1)
    y_sign = torch.tensor([1.0, -1.0, 1.0, -1.0], device=cmd.device)
    x_sign = torch.tensor([1.0, 1.0, -1.0, -1.0], device=cmd.device)
    num_commands = env.cfg.commands.num_commands
    if num_commands >= 13:
        width = cmd[:, 12:13]
        ys = torch.cat([width / 2, -width / 2, width / 2, -width / 2], dim=1)
    else:
        width = DEFAULT_STANCE_WIDTH
        ys = (y_sign * (width / 2)).unsqueeze(0)
    if num_commands >= 14:
        length = cmd[:, 13:14]
        xs = torch.cat([length / 2, length / 2, -length / 2, -length / 2], dim=1)
    else:
        length = DEFAULT_STANCE_LENGTH
        xs = (x_sign * (length / 2)).unsqueeze(0)
    phase = torch.abs(1.0 - env.foot_indices * 2.0) * 1.0 - 0.5
    half_period = 0.5 / cmd[:, 4].unsqueeze(1)
    y_offset = phase * (cmd[:, 2:3] * length / 2) * half_period
    y_offset[:, 2:4] *= -1
    x_offset = phase * cmd[:, 0:1] * half_period
    wanted = torch.stack((xs + x_offset, ys + y_offset), dim=2)
    return torch.square(torch.abs(wanted - feet[:, :, 0:2])).sum(dim=(1, 2)).cpu()


def feet_slip(env, actor_critic=None, obs=None):
    """squared planar speed of the feet in contact (the reference's term without its previous-step filter)"""
    speed_sq = torch.square(torch.norm(env.foot_velocities[:, :, 0:2], dim=2).view(env.commands.shape[0], -1))
    return torch.sum(foot_contacts(env) * speed_sq, dim=1).cpu()


def action_rate(env, actor_critic=None, obs=None):
    """squared change of the action from the previous step to this one"""
    return torch.sum(torch.square(env.last_actions - env.last_last_actions), dim=1).cpu()


BEHAVIOUR_FNS = {fn.__name__: fn for fn in (contact_match, body_height_err, orientation_err, feet_clearance, raibert_heuristic,
                                            feet_slip, action_rate)}
assert list(BEHAVIOUR_FNS) == PER_STEP


class StrideTracker:
    """The stride rules of include/go1eval.h on the host, for N environments x 4 feet.  `step()` takes one step's contacts
    (N, 4) bool, foot heights (N, 4), commands (N, >= 10) and the mask of environments that count (not reset, past the warm-up),
    and returns the strides that ended at this step as a list of (environment, foot, step_frequency_err, duty_factor_err,
    swing_height_err), environments ascending, feet 0..3 within one: the order the kernel folds them in.  `dtype` is the
    arithmetic's precision."""

    def __init__(self, num_envs, dt, dtype=np.float32):
        self.dt, self.dtype = dtype(np.float32(dt)), dtype          # (the kernel's configuration holds dt in fp32)
        self.prev_contact = np.full((num_envs, 4), 2, np.uint8)
        self.stride_steps = np.full((num_envs, 4), -1, np.int32)
        self.stance_steps = np.zeros((num_envs, 4), np.int32)
        self.swing_peak = np.full((num_envs, 4), -np.inf, dtype)

    def step(self, contact, foot_z, commands, counted):
        T = self.dtype
        contact, counted = np.asarray(contact, bool), np.asarray(counted, bool)
        foot_z, commands = np.asarray(foot_z, T), np.asarray(commands, T)
        self.prev_contact[~counted] = 2
        self.stride_steps[~counted] = -1
        touchdown = contact & (self.prev_contact == 0) & counted[:, None]
        events = []
        for e, f in zip(*np.nonzero(touchdown & (self.stride_steps >= 0))):
            L = T(self.stride_steps[e, f])
            with np.errstate(all="ignore"):
                events.append((int(e), int(f), T(1) / (L * self.dt) - commands[e, 4], T(self.stance_steps[e, f]) / L - commands[e, 8],
                               (self.swing_peak[e, f] - T(FOOT_RADIUS)) - commands[e, 9]))
        self.stride_steps[touchdown] = 0
        self.stance_steps[touchdown] = 0
        self.swing_peak[touchdown] = -np.inf
        live = counted[:, None]
        self.stride_steps += live & (self.stride_steps >= 0)
        self.stance_steps += live & contact
        self.swing_peak = np.where(live, np.maximum(self.swing_peak, foot_z), self.swing_peak)
        self.prev_contact = np.where(live, contact.astype(np.uint8), self.prev_contact)
        return events


def behaviour_cells(axes):
    """[{name: value}, ...]: the row-major product of `axes` = {command name: [values]}, names from COMMAND_INDEX"""
    for name in axes:
        if name not in COMMAND_INDEX:
            raise KeyError(f"behaviour_cells: unknown command {name!r}; one of {sorted(COMMAND_INDEX)}")
    names = list(axes)
    return [dict(zip(names, (float(v) for v in values))) for values in itertools.product(*(axes[n] for n in names))]


def behaviour_command_table(cells, num_commands, device, base_cell=(1.0, 0.0, sweep.GAITS["trotting"])):
    """(cells, num_commands) commands: the values `sweep.command_table` holds for `base_cell` = (vx, yaw rate, gait) (a trot at
    1 m/s, 3 Hz, duty 0.5, foot swing 0.08 m, stance 0.25 m x 0.40 m), with every cell's named columns overridden"""
    base = sweep.command_table([base_cell], num_commands, "cpu")
    cmd = base.repeat(len(cells), 1)
    for i, cell in enumerate(cells):
        for name, value in cell.items():
            if COMMAND_INDEX[name] >= num_commands:
                raise ValueError(f"behaviour_command_table: the command vector has {num_commands} entries, none for {name!r}")
            cmd[i, COMMAND_INDEX[name]] = value
    return cmd.to(device)


def prepare(env, cells):
    """as sweep.prepare, with the behaviour cells' commands"""
    base = env.env
    env.reset()
    group = torch.arange(base.num_envs, device=base.device) % len(cells)
    commands = behaviour_command_table(cells, base.commands.shape[1], base.device)[group]
    base.commands[:] = commands
    return env.get_observations(), group.to(torch.int32), commands


def run_behaviour_sweep(policy, preset, axes, num_envs=4096, steps=500, warmup_steps=25, seed=1, terrain=None):
    """Both tables for one preset over the product of `axes`: the dict of sweep.run_sweep ("cells" are dicts here) plus
    "behaviour": {behaviour metric name: (cells, 6) array of count, mean, std, min, max, nonfinite}."""
    cells = behaviour_cells(axes)
    env, _ = sweep.build_eval_env(preset, num_envs, seed, terrain)
    if hasattr(policy, "eval"):
        policy.eval()
    obs, group, commands = prepare(env, cells)
    env.env.start_metrics(group, warmup_steps=warmup_steps, behaviour=True)
    sweep.rollout(env, policy, obs, steps, commands)
    env.env.stop_metrics()
    if not sweep.commands_held(env, commands):
        raise RuntimeError("run_behaviour_sweep: an environment left its cell's commands during the rollout")
    res = env.env.read_metrics()
    groups, behaviour = res.pop("groups"), res.pop("behaviour")
    return dict(preset=preset, cells=cells, metrics=res, behaviour=behaviour, groups=groups, num_envs=num_envs, steps=steps,
                warmup_steps=warmup_steps, seed=seed)


def behaviour_markdown_table(result, metrics=tuple(BEHAVIOUR_NAMES)):
    """one row per cell: its command values, its fall rate, and mean +- std of the behaviour metrics (errors are realised minus
    commanded; the stride metrics also show how many strides they average)"""
    names = list(result["cells"][0]) if result["cells"] else []
    head = names + ["envs", "fall rate"] + list(metrics) + ["strides"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for g, cell in enumerate(result["cells"]):
        row = [f"{cell[n]:g}" for n in names] + [f"{int(result['groups'][g, 0])}", f"{result['groups'][g, 4]:.3f}"]
        row += [f"{result['behaviour'][m][g, 1]:.4g} ± {result['behaviour'][m][g, 2]:.3g}" for m in metrics]
        row.append(f"{int(result['behaviour']['step_frequency_err'][g, 0])}")
        lines.append("| " + " | ".join(row) + " |")
    return "\n".join(lines)


def behaviour_to_json(result):
    """the JSON form of a run_behaviour_sweep result"""
    return dict(preset=result["preset"], num_envs=result["num_envs"], steps=result["steps"], warmup_steps=result["warmup_steps"],
                seed=result["seed"], cells=result["cells"], fields=list(sweep.FIELDS),
                metrics={k: v.tolist() for k, v in result["metrics"].items()},
                behaviour={k: v.tolist() for k, v in result["behaviour"].items()},
                group_fields=["envs", "steps", "episodes_terminated", "episodes_timed_out", "fall_rate"], groups=result["groups"].tolist())
