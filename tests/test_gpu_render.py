"""GPU tests of the renderer of recorded episodes (csrc/go1render.hip, include/go1render.h) through LeggedRobot's recording surface
(reference legged_robot.py start_recording / get_complete_frames / render, :1591-1673, recording boundaries :1003-1015):
the kernel's frames against the fp64 numpy renderer of tests/render_ref.py, the recording state machine, recording leaving the
simulation bit-identical, and the Runner writing videos end to end.  Not run under GO1_DRY_RUN_GPU_TESTS: the SIMT emulator has
no renderer."""
import os
import threading

import numpy as np
import pytest
import torch

import render_ref as R

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("GO1_DRY_RUN_GPU_TESTS")), reason="the emulated GPU has no renderer")]


def make_env(N=64, terrain="plane", episode_length_s=None, n_eval=0, seed=0):
    from go1_gym.envs.base.legged_robot_config import make_cfg
    from go1_gym.envs.go1.velocity_tracking import VelocityTrackingEasyEnv
    from scripts.train_config import apply_train_config
    cfgs = [apply_train_config(make_cfg(), num_envs=n) for n in ((N, n_eval) if n_eval else (N,))]
    for c in cfgs:
        t = c.terrain
        if terrain == "plane":
            t.mesh_type = "plane"
        else:                               # the train config's tile grid with rough slopes, stairs and obstacles
            t.mesh_type = terrain
            t.terrain_proportions, t.curriculum, t.center_robots = [0.1, 0.1, 0.35, 0.25, 0.2], True, False
            t.num_rows, t.num_cols, t.terrain_length, t.terrain_width, t.border_size = 4, 4, 8.0, 8.0, 5.0
            t.min_init_terrain_level, t.max_init_terrain_level = 0, 3
        if episode_length_s is not None:
            c.env.episode_length_s = episode_length_s
    torch.manual_seed(seed)
    np.random.seed(seed)
    return VelocityTrackingEasyEnv(sim_device="cuda:0", headless=True, cfg=cfgs[0], eval_cfg=cfgs[1] if n_eval else None)


def ref_terrain(env):
    S = env.sim_config
    if S.terrain_type == 0:
        return "plane"
    return R.HeightField(env.buffers.height_samples.cpu().numpy(), S.hf_hscale, S.hf_vscale, S.hf_border)


def compare(env, e=0, what=""):
    img = env._renderer().image(e).cpu().numpy()
    root = env.buffers.root_states[:, e].double().cpu().numpy()
    dof = env.buffers.dof_pos[:, e].double().cpu().numpy()
    ref, ids = R.render(root, dof, ref_terrain(env))
    assert img.shape == (240, 360, 4) and img.dtype == np.uint8 and (img[..., 3] == 255).all()
    diff = np.abs(img.astype(int) - ref.astype(int)).max(axis=-1)
    bad = diff > 2
    assert bad.mean() <= 0.01, (what, bad.mean())
    stray = bad & ~R.id_edges(ids)
    assert not stray.any(), (what, int(stray.sum()), np.argwhere(stray)[:5].tolist(), diff[stray][:5].tolist())
    kind = ids % 32
    assert (kind >= 3).sum() > 300, what                 # the robot is in the picture
    assert ((kind == 1) | (kind == 2)).sum() > 1000, what
    return img, ids


@pytest.mark.parametrize("terrain", ["plane", "heightfield", "trimesh"])
def test_kernel_frames_match_the_numpy_reference(terrain):
    env = make_env(terrain=terrain)
    S = env.sim_config
    if terrain == "plane":
        assert S.terrain_type == 0
    else:
        assert S.terrain_type == 1 and (S.hf_wall_units > 0) == (terrain == "trimesh")
    env.reset()
    B = env.buffers
    # standing: the default joint angles at the post-reset base pose
    B.dof_pos[:, 0] = env.default_dof_pos[0]
    compare(env, 0, "standing")
    # hand-posed: tilted body, legs folded
    q = torch.tensor([0.25, -0.2, 0.15, 0.93], device="cuda")
    B.root_states[3:7, 0] = q / q.norm()
    B.root_states[2, 0] += 0.1
    B.dof_pos[:, 0] = torch.tensor([0.4, 1.6, -2.6, -0.5, 1.3, -2.5, 0.3, 2.2, -1.0, -0.3, -0.6, -2.0], device="cuda")
    compare(env, 0, "tilted, folded")
    # free-running states after random actions, several envs (different places on the terrain)
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(50):
        env.step(0.6 * torch.randn(env.num_envs, 12, device="cuda", generator=g))
    for e in (0, 17, 42):
        compare(env, e, f"after 50 steps, env {e}")


def _step_and_watch(env, steps, cams, g):
    """step `steps` times; per step the reset flags of the recorded envs and a synchronous render of each (bit-exact reference)"""
    resets, images = {e: [] for e in cams}, {e: [] for e in cams}
    done = {e: None for e in cams}
    for k in range(steps):
        env.step(0.5 * torch.randn(env.num_envs, 12, device="cuda", generator=g))
        rb = env.reset_buf.cpu().numpy()
        for e, getter in cams.items():
            resets[e].append(bool(rb[e]))
            images[e].append(env._renderer().image(e).cpu().numpy().copy())
            frames = getter()
            r = [i for i, f in enumerate(resets[e]) if f]
            if len(r) < 2:
                assert frames == [], (e, k)
            elif done[e] is None:
                done[e] = frames
    return resets, images, done


def test_recording_follows_the_reference_rules_train_and_eval_cameras():
    NT = 64
    env = make_env(N=NT, episode_length_s=1.0, n_eval=16)
    assert 50 <= env.max_episode_length <= 51                # ceil(1 / dt) in floating point
    assert env.start_recording() is None and env.get_complete_frames() == []
    env.start_recording_eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    cams = {0: env.get_complete_frames, NT: env.get_complete_frames_eval}
    resets, images, done = _step_and_watch(env, 130, cams, g)
    for e in cams:
        r = [i for i, f in enumerate(resets[e]) if f]
        assert len(r) >= 2, (e, r)
        r1, r2 = r[0], r[1]
        frames = done[e]
        assert len(frames) == r2 - r1, (e, r1, r2, len(frames))
        for i, f in enumerate(frames):
            assert f.shape == (240, 360, 4) and f.dtype == np.uint8
            assert np.array_equal(f, images[e][r1 + i]), (e, i)
        # the complete recording stays until pause_recording()
        assert cams[e]() is frames or np.array_equal(np.stack(cams[e]()), np.stack(frames))
    env.pause_recording()
    env.pause_recording_eval()
    assert env.get_complete_frames() == [] and env.get_complete_frames_eval() == []
    assert not env._render.any_armed
    # a host reset of the recorded env is a boundary too: armed -> reset_idx starts the recording, the next one ends it
    env.start_recording()
    env.reset_idx(torch.arange(env.num_envs, device="cuda"))
    for _ in range(3):
        env.step(torch.zeros(env.num_envs, 12, device="cuda"))
    last = env.render()
    assert not bool(env.reset_buf[0]) and env.get_complete_frames() == []
    env.reset_idx(torch.tensor([5, 0, 9], device="cuda"))
    frames = env.get_complete_frames()
    assert len(frames) == 3 and np.array_equal(frames[-1], last)
    env.pause_recording()


def test_recording_leaves_the_simulation_bit_identical():
    envs = [make_env(N=64, episode_length_s=1.0, seed=3) for _ in range(2)]
    for name in ("obs_buf", "root_states", "dof_pos", "commands"):
        assert torch.equal(getattr(envs[0].buffers, name), getattr(envs[1].buffers, name)), name
    envs[1].start_recording()
    g = torch.Generator(device="cuda").manual_seed(2)
    for k in range(150):
        a = 0.5 * torch.randn(64, 12, device="cuda", generator=g)
        for e in envs:
            e.step(a)
        if k % 25 == 0:
            envs[1].get_complete_frames()
    torch.cuda.synchronize()
    assert envs[1]._render is not None and envs[0]._render is None
    for name in ("obs_buf", "rew_buf", "reset_buf", "root_states"):
        assert torch.equal(getattr(envs[0].buffers, name), getattr(envs[1].buffers, name)), name


def test_runner_writes_playable_videos(tmp_path, monkeypatch):
    from go1_gym.envs.wrappers.history_wrapper import HistoryWrapper
    from go1_gym_learn.ppo_cse import Runner, RunnerArgs
    from ml_logger import logger
    import test_render
    logger.configure("run", root=str(tmp_path))
    monkeypatch.setattr(logger, "print_summary", False)
    monkeypatch.setattr(RunnerArgs, "save_interval", 100)
    monkeypatch.setattr(RunnerArgs, "log_freq", 1)
    # (the Runner arms the camera when `it - last >= interval` BEFORE it collects, as the reference's log_video: interval 1 re-arms
    # every iteration, so the smallest interval that completes a recording is 2)
    monkeypatch.setattr(RunnerArgs, "save_video_interval", 2)
    saved = []
    real = logger.save_video
    monkeypatch.setattr(logger, "save_video", lambda frames, path, fps=30: saved.append((path, len(frames), fps)) or real(frames, path, fps))
    env = HistoryWrapper(make_env(N=64, episode_length_s=0.2))
    monkeypatch.chdir(tmp_path)
    runner = Runner(env, device="cuda:0")
    runner.learn(num_learning_iterations=8, init_at_random_ep_len=False)
    for t in threading.enumerate():
        if t.name == "save_video":
            t.join()
    assert saved, "no video written"
    for path, n, fps in saved:
        assert fps == pytest.approx(1 / env.dt)
        png = tmp_path / "run" / (os.path.splitext(path)[0] + ".png")
        assert png.exists(), png
        frames, delays, count = test_render.read_apng(str(png))
        assert count == len(frames) == n > 0
        assert delays[0] == pytest.approx(env.dt, abs=1e-9)
    assert any(p.startswith("videos/000") for p, _, _ in saved)
