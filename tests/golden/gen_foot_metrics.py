#!/usr/bin/env python3
"""Generate the foot-loading fixture by executing two of the REFERENCE's CoRLRewards methods
(go1_gym/envs/rewards/corl_rewards.py) on the CPU, in the manner of gen_joint_metrics.py (make_golden.py's stubs for the packages
the reference imports are reused).  Runs only in the authoring container (needs the reference checkout make_golden.py points at).
No reference code is copied; its methods are executed and only their inputs and outputs are written.

Output:
  foot_metrics.npz      per seed: mock-environment tensors (N = 64, the reference's layout: contact_forces [N, 17, 3],
                        prev_foot_velocities [N, 4, 3]; feet_indices; max_contact_force) and what _reward_feet_contact_forces and
                        _reward_feet_impact_vel return on them
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
SEEDS = [0, 1, 2]
MAX_CONTACT_FORCE = 100.0
FEET = [4, 8, 12, 16]
INPUTS = ["contact_forces", "prev_foot_velocities"]
OUTPUTS = ["feet_contact_forces", "feet_impact_vel"]


def mock_inputs(seed):
    g = torch.Generator().manual_seed(400 + seed)
    x = {}
    forces = 5.0 * torch.randn(N, 17, 3, generator=g)
    load = 120.0 * torch.rand(N, 4, generator=g)                          # vertical loads up to 120 N: a sixth beyond 100 N
    air = torch.rand(N, 4, generator=g) < 0.4                             # feet in the air: a force of a few tenths of a newton
    forces[:, FEET, 2] = load
    forces[:, FEET, :] = torch.where(air.unsqueeze(-1), 0.1 * forces[:, FEET, :], forces[:, FEET, :])
    forces[0, FEET, :] = 0.0                                              # a robot in flight
    forces[1, FEET, 2] = 250.0                                            # far beyond the limit
    x["contact_forces"] = forces
    vel = 1.5 * torch.randn(N, 4, 3, generator=g)                         # upward and downward
    vel[2, :, 2] = torch.tensor([-250.0, -100.0, -99.0, 100.0])           # beyond the clip, on it, inside, upward
    x["prev_foot_velocities"] = vel
    norm = torch.norm(forces[:, FEET, :], dim=-1)
    # the condition the test's bit-equality rests on: no norm within 1e-3 of the two thresholds
    assert ((norm - 1.0).abs() > 1e-3).all() and ((norm - MAX_CONTACT_FORCE).abs() > 1e-3).all()
    assert (norm > MAX_CONTACT_FORCE).any() and (norm < 1.0).any() and (vel[:, :, 2] > 0).any() and (vel[:, :, 2] < -100.0).any()
    return x


def mock_env(x):
    env = types.SimpleNamespace(num_envs=N, device="cpu", feet_indices=torch.tensor(FEET))
    env.cfg = types.SimpleNamespace(rewards=types.SimpleNamespace(max_contact_force=MAX_CONTACT_FORCE))
    env.contact_forces, env.prev_foot_velocities = (x[k] for k in INPUTS)
    return env


def main():
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    R = importlib.import_module("go1_gym.envs.rewards.corl_rewards")                       # the REFERENCE module
    out = {}
    for seed in SEEDS:
        x = mock_inputs(seed)
        rewards = R.CoRLRewards(mock_env(x))
        for k in INPUTS:
            out[f"s{seed}_in_{k}"] = x[k].numpy().copy()
        for name in OUTPUTS:
            r = getattr(rewards, "_reward_" + name)()
            assert r.shape == (N,) and r.dtype == torch.float32, (name, r.shape, r.dtype)
            out[f"s{seed}_out_{name}"] = r.numpy().copy()
    out["max_contact_force"] = np.float64(MAX_CONTACT_FORCE)
    out["feet_indices"] = np.array(FEET, np.int64)
    np.savez_compressed(os.path.join(HERE, "foot_metrics.npz"), **out)
    print("foot fixture:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "foot_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
