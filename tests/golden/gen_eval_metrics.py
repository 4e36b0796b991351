#!/usr/bin/env python3
"""Generate the evaluation fixtures by executing the REFERENCE's go1_gym_learn/eval_metrics/{metrics,domain_randomization}.py
on the CPU, in the manner of make_golden.py (whose stubs for the packages the reference imports are reused).  Runs only in
the authoring container (needs the reference checkout make_golden.py points at).  No reference code is copied; its functions are executed and only their
inputs and outputs are written.

Output:
  eval_metrics.npz          three seeds of mock-environment tensors (N = 256, the reference's [N, k] layout) and what the
                            reference's ten scalar metric functions return on them
  eval_metric_names.json    sorted keys of the reference's METRICS_FNS
  eval_dr_settings.json     for base_set and each of the six DR presets: the Cfg leaves that differ from a fresh Cfg after the call
"""
import importlib
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

N = 256
HEIGHT_POINTS = 17
SCALAR = ["lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "base_height", "max_torques", "power_consumption", "CoT",
          "froude_number", "termination"]


def mock_env(seed, with_heights):
    g = torch.Generator().manual_seed(seed)
    env = types.SimpleNamespace()
    env.base_lin_vel = 1.5 * torch.randn(N, 3, generator=g)
    env.base_lin_vel[::9, 0:2] = 0.0                       # robots that stand still: CoT divides by zero
    env.base_ang_vel = torch.randn(N, 3, generator=g)
    env.commands = torch.randn(N, 15, generator=g)
    env.root_states = torch.randn(N, 13, generator=g)
    env.root_states[:, 2] = 0.3 + 0.05 * torch.randn(N, generator=g)
    env.measured_heights = 0.1 * torch.randn(N, HEIGHT_POINTS, generator=g) if with_heights else 0
    env.torques = 20.0 * torch.randn(N, 12, generator=g)
    env.torques[::9] *= (torch.rand(N, 1, generator=g)[::9] > 0.5)   # some of the standing robots draw no power either: 0 / 0
    env.dof_vel = 8.0 * torch.randn(N, 12, generator=g)
    env.payloads = -1.0 + 4.0 * torch.rand(N, generator=g)
    env.default_body_mass = 4.801
    env.reset_buf = torch.rand(N, generator=g) < 0.15
    env.time_out_buf = env.reset_buf & (torch.rand(N, generator=g) < 0.5)
    env.episode_length_buf = torch.randint(0, 40, (N,), generator=g, dtype=torch.int32)
    env.episode_length_buf[env.reset_buf] = 0
    return env


def tree(node):
    out = {}
    for k in dir(node):
        if k.startswith("_"):
            continue
        v = getattr(node, k)
        if inspect.isclass(v):
            for kk, vv in tree(v).items():
                out[f"{k}.{kk}"] = vv
        elif callable(v):
            continue
        else:
            out[k] = list(v) if isinstance(v, tuple) else v
    return out


def main():
    MG.install_stubs()
    sys.path.insert(0, MG.REF)
    M = importlib.import_module("go1_gym_learn.eval_metrics.metrics")                      # the REFERENCE modules
    with open(os.path.join(HERE, "eval_metric_names.json"), "w") as f:
        json.dump(sorted(M.METRICS_FNS), f, indent=0)

    out = {}
    for seed, with_heights in ((0, True), (1, False), (2, True)):
        env = mock_env(seed, with_heights)
        for k in ("base_lin_vel", "base_ang_vel", "commands", "root_states", "torques", "dof_vel", "payloads", "reset_buf",
                  "time_out_buf", "episode_length_buf"):
            out[f"s{seed}_in_{k}"] = getattr(env, k).numpy()
        if with_heights:
            out[f"s{seed}_in_measured_heights"] = env.measured_heights.numpy()
        for name in SCALAR:
            r = M.METRICS_FNS[name](env, None, None)
            assert r.shape == (N,), (name, r.shape)
            out[f"s{seed}_out_{name}"] = r.numpy()
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)

    settings = {}
    cfg_mod = importlib.import_module("go1_gym.envs.base.legged_robot_config")
    dr_mod = importlib.import_module("go1_gym_learn.eval_metrics.domain_randomization")
    for name in ["base_set"] + sorted(dr_mod.DR_SETTINGS):
        cfg_mod = importlib.reload(cfg_mod)                 # a fresh Cfg
        dr_mod = importlib.reload(dr_mod)
        before = tree(cfg_mod.Cfg)
        getattr(dr_mod, name)()
        after = tree(cfg_mod.Cfg)
        settings[name] = {k: v for k, v in after.items() if k not in before or before[k] != v}
    with open(os.path.join(HERE, "eval_dr_settings.json"), "w") as f:
        json.dump(settings, f, indent=0, sort_keys=True)
    print("eval fixtures:", len(out), "arrays;", {k: len(v) for k, v in settings.items()})


if __name__ == "__main__":
    main()
