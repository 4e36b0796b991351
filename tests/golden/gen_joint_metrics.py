#!/usr/bin/env python3
"""Generate the joint-metric fixture by executing four of the REFERENCE's CoRLRewards methods
(go1_gym/envs/rewards/corl_rewards.py) on the CPU, in the manner of gen_behaviour_metrics.py (make_golden.py's stubs for the
packages the reference imports are reused).  Runs only in the authoring container (needs the reference checkout make_golden.py
points at).  No reference code is copied; its methods are executed and only their inputs and outputs are written.

Output:
  joint_metrics.npz     per seed: mock-environment tensors (N = 64, the reference's [N, 12] layout: torques, dof_vel, last_dof_vel,
                        dof_pos; dof_pos_limits [12, 2]; dt) and what _reward_torques, _reward_dof_vel, _reward_dof_acc and
                        _reward_dof_pos_limits return on them
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
DT = 0.02
INPUTS = ["torques", "dof_vel", "last_dof_vel", "dof_pos", "dof_pos_limits"]
OUTPUTS = ["torques", "dof_vel", "dof_acc", "dof_pos_limits"]
# the soft position limits of a Go1 at rewards.soft_dof_pos_limit = 0.9 (hip, thigh, calf), to three digits
LOWER, UPPER = [-0.723, -0.785, -2.608] * 4, [0.723, 3.927, -1.005] * 4


def mock_inputs(seed):
    g = torch.Generator().manual_seed(300 + seed)
    x = {}
    x["torques"] = (15.0 * torch.randn(N, 12, generator=g)).clamp(-33.5, 33.5)          # some sit on the clip
    x["dof_vel"] = 10.0 * torch.randn(N, 12, generator=g)
    x["last_dof_vel"] = x["dof_vel"] + 2.0 * torch.randn(N, 12, generator=g)
    x["last_dof_vel"][0] = 0.0                                                          # (a robot one step after its reset)
    limits = torch.tensor([LOWER, UPPER]).t().contiguous()
    x["dof_pos_limits"] = limits
    span = limits[:, 1] - limits[:, 0]
    x["dof_pos"] = limits[:, 0] + span * (1.2 * torch.rand(N, 12, generator=g) - 0.1)   # a sixth of them beyond a limit
    x["dof_pos"][1] = limits[:, 0]                                                      # exactly on the limits
    x["dof_pos"][2] = limits[:, 1]
    return x


def mock_env(x):
    env = types.SimpleNamespace(num_envs=N, device="cpu", dt=DT)
    env.torques, env.dof_vel, env.last_dof_vel, env.dof_pos, env.dof_pos_limits = (x[k] for k in INPUTS)
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
    out["dt"] = np.float64(DT)
    np.savez_compressed(os.path.join(HERE, "joint_metrics.npz"), **out)
    print("joint fixture:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "joint_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
