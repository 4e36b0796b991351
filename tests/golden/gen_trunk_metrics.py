#!/usr/bin/env python3
"""Generate the trunk-motion fixture by executing three of the REFERENCE's CoRLRewards methods
(go1_gym/envs/rewards/corl_rewards.py) on the CPU, in the manner of gen_foot_metrics.py (make_golden.py's stubs for the packages
the reference imports are reused).  Runs only in the authoring container (needs the reference checkout make_golden.py points at).
No reference code is copied; its methods are executed and only their inputs and outputs are written.

Output:
  trunk_metrics.npz     per seed: mock-environment tensors (N = 64, the reference's layout: projected_gravity, base_lin_vel,
                        base_ang_vel [N, 3]) and what _reward_orientation, _reward_lin_vel_z and _reward_ang_vel_xy return on them
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
INPUTS = ["projected_gravity", "base_lin_vel", "base_ang_vel"]
OUTPUTS = ["orientation", "lin_vel_z", "ang_vel_xy"]


def mock_inputs(seed):
    g = torch.Generator().manual_seed(500 + seed)
    x = {}
    gravity = torch.randn(N, 3, generator=g)
    gravity = gravity / gravity.norm(dim=1, keepdim=True)                 # unit vectors: every attitude, upside down included
    gravity[:N // 2, :2] *= 0.1                                           # half of them near upright
    gravity[0] = torch.tensor([0.0, 0.0, -1.0])                           # upright
    gravity[1] = torch.tensor([1.0, 0.0, 0.0])                            # on its nose
    x["projected_gravity"] = gravity
    x["base_lin_vel"] = 0.5 * torch.randn(N, 3, generator=g)
    x["base_ang_vel"] = 2.0 * torch.randn(N, 3, generator=g)
    x["base_lin_vel"][2, 2] = 0.0
    x["base_ang_vel"][3, :2] = 0.0
    return x


def mock_env(x):
    env = types.SimpleNamespace(num_envs=N, device="cpu")
    for k in INPUTS:
        setattr(env, k, x[k])
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
    np.savez_compressed(os.path.join(HERE, "trunk_metrics.npz"), **out)
    print("trunk fixture:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "trunk_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
