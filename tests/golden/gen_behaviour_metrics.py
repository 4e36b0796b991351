#!/usr/bin/env python3
"""Generate the behaviour-metric fixture by executing six of the REFERENCE's CoRLRewards methods
(go1_gym/envs/rewards/corl_rewards.py) on the CPU, in the manner of gen_eval_metrics.py (make_golden.py's stubs for the
packages the reference imports are reused).  Runs only in the authoring container (needs the reference checkout make_golden.py
points at).  No reference code is copied; its methods are executed and only their inputs and outputs are written.

Output:
  behaviour_metrics.npz     per case (seed, number of commands): mock-environment tensors (N = 64, the reference's [N, ...]
                            layout; of root_states the pose columns 0..6, of contact_forces the four feet's rows) and what
                            _reward_jump, _reward_orientation_control, _reward_feet_clearance_cmd_linear,
                            _reward_raibert_heuristic, _reward_feet_slip (last_contacts all false) and _reward_action_rate
                            (actions / last_actions = this and the previous step's) return on them
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

N = 64
CASES = [(0, 15), (1, 13), (0, 12)]            # (seed, num_commands)
BASE_HEIGHT_TARGET = 0.30
INPUTS = ["commands", "base_pose", "foot_forces", "foot_positions", "foot_velocities", "desired_contact_states", "foot_indices",
          "actions_now", "actions_before"]
OUTPUTS = ["jump", "orientation_control", "feet_clearance_cmd_linear", "raibert_heuristic", "feet_slip", "action_rate"]


def mock_inputs(seed, num_commands):
    g = torch.Generator().manual_seed(100 + seed)
    rng = np.random.default_rng(100 + seed)
    x = {}
    cmd = torch.zeros(N, num_commands)
    cmd[:, 0:3] = torch.randn(N, 3, generator=g)
    cmd[:, 3] = 0.1 * torch.randn(N, generator=g)                       # body height
    cmd[:, 4] = 2.0 + 2.0 * torch.rand(N, generator=g)                  # step frequency
    cmd[0, 4] = 0.0                                                     # (one robot commanded to 0 Hz: the heuristic divides by it)
    cmd[:, 5:9] = torch.rand(N, 4, generator=g)
    cmd[:, 9] = 0.03 + 0.2 * torch.rand(N, generator=g)                 # foot-swing height
    cmd[:, 10:12] = 0.4 * torch.randn(N, 2, generator=g)                # pitch, roll
    if num_commands > 12:
        cmd[:, 12] = 0.1 + 0.35 * torch.rand(N, generator=g)            # stance width
    if num_commands > 13:
        cmd[:, 13] = 0.35 + 0.1 * torch.rand(N, generator=g)            # stance length
    x["commands"] = cmd
    root = torch.randn(N, 13, generator=g)
    root[:, 2] = 0.3 + 0.05 * torch.randn(N, generator=g)
    root[:, 3:7] = MG.rand_quat(rng, N)
    x["root_states"] = root
    x["base_pose"] = root[:, 0:7]                                       # (position and xyzw quaternion: all the six methods read)
    forces = 30.0 * torch.randn(N, 17, 3, generator=g)
    forces[:, :, 2] = forces[:, :, 2].abs() * (torch.rand(N, 17, generator=g) < 0.6)      # feet in the air carry no force
    forces[1, 4, 2], forces[2, 8, 2] = 1.0, 1.5                         # either side of the contact threshold
    x["contact_forces"] = forces
    x["foot_forces"] = forces[:, [4, 8, 12, 16], :]                     # (the six methods read no other body's)
    nominal = torch.tensor([[0.19, -0.15, -0.3], [0.19, 0.15, -0.3], [-0.19, -0.15, -0.3], [-0.19, 0.15, -0.3]])
    feet = root[:, None, 0:3] + nominal[None] + 0.05 * torch.randn(N, 4, 3, generator=g)
    feet[:, :, 2] = 0.02 + 0.12 * torch.rand(N, 4, generator=g)
    x["foot_positions"] = feet
    x["foot_velocities"] = torch.randn(N, 4, 3, generator=g)
    x["desired_contact_states"] = torch.rand(N, 4, generator=g)
    x["desired_contact_states"][::3] = (x["desired_contact_states"][::3] > 0.5).float()
    x["foot_indices"] = torch.rand(N, 4, generator=g)
    x["actions_now"] = torch.randn(N, 12, generator=g)
    x["actions_before"] = torch.randn(N, 12, generator=g)
    return x


def mock_env(x, num_commands, tu):
    env = types.SimpleNamespace(num_envs=N, device="cpu")
    env.cfg = types.SimpleNamespace(rewards=types.SimpleNamespace(base_height_target=BASE_HEIGHT_TARGET),
                                    commands=types.SimpleNamespace(num_commands=num_commands))
    env.commands, env.root_states = x["commands"], x["root_states"]
    env.base_pos, env.base_quat = x["root_states"][:, 0:3], x["root_states"][:, 3:7]
    env.gravity_vec = torch.tensor([0.0, 0.0, -1.0]).repeat(N, 1)
    env.projected_gravity = tu.quat_rotate_inverse(env.base_quat, env.gravity_vec)
    env.contact_forces, env.feet_indices = x["contact_forces"], torch.tensor([4, 8, 12, 16])
    env.foot_positions, env.foot_velocities = x["foot_positions"], x["foot_velocities"]
    env.desired_contact_states, env.foot_indices = x["desired_contact_states"], x["foot_indices"]
    env.last_contacts = torch.zeros(N, 4, dtype=torch.bool)
    env.actions, env.last_actions = x["actions_now"], x["actions_before"]
    return env


def main():
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    R = importlib.import_module("go1_gym.envs.rewards.corl_rewards")                       # the REFERENCE module
    tu = sys.modules["isaacgym.torch_utils"]
    out = {}
    for seed, num_commands in CASES:
        x = mock_inputs(seed, num_commands)
        rewards = R.CoRLRewards(mock_env(x, num_commands, tu))
        key = f"s{seed}_c{num_commands}"
        for k in INPUTS:
            out[f"{key}_in_{k}"] = x[k].numpy().copy()
        for name in OUTPUTS:
            r = getattr(rewards, "_reward_" + name)()
            assert r.shape == (N,) and r.dtype == torch.float32, (name, r.shape, r.dtype)
            out[f"{key}_out_{name}"] = r.numpy().copy()
    out["base_height_target"] = np.float32(BASE_HEIGHT_TARGET)
    np.savez_compressed(os.path.join(HERE, "behaviour_metrics.npz"), **out)
    print("behaviour fixture:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "behaviour_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
