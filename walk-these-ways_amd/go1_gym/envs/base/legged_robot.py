"""`LeggedRobot`: the vectorised Go1 environment on MI355X.

Same step / reset / get_observations surface, constructor and attribute names as the reference's
go1_gym/envs/base/legged_robot.py (`LeggedRobot` :19-58, `step` :60-88, `reset_idx` :150-239, buffers
:1123-1297), but nothing here computes per-environment arithmetic in Python: `step()` is one call into
libgo1sim (HIP, include/go1sim.h `go1sim_step`), which runs the torque model, the 4 physics substeps and
every tensor map of `post_physics_step` in a single kernel launch on the current torch stream, with no
host synchronisation.  This class owns the device buffers (torch tensors, SoA layout) and exposes them
under the reference's attribute names as (N, ...) views.
"""
import os
from collections.abc import Mapping

import numpy as np
import torch

import go1sim_host as H
from go1_gym.envs.base.base_task import BaseTask
from go1_gym.utils.terrain import Terrain


class _LazyMapping(Mapping):
    """Base of the `extras` entries that are evaluated on access.  Pickled (the reference Runner dumps
    `extras["curriculum/distribution"]` with `logger.save_pkl`, ppo_cse/__init__.py:200-208) and deep-copied as the plain dict
    of their current values — never as a reference to the environment."""

    def __reduce__(self):
        return (dict, (dict(self.items()),))


class _EpisodeStats(_LazyMapping):
    """`extras["train/episode"]` (reference legged_robot.py:181-227): means of the per-term episode sums over the
    environments that were reset, plus command-range statistics.  Evaluated lazily on access (device reductions,
    no work and no sync inside step()); the running sums are kept by the kernel in `episode_log`."""

    def __init__(self, env):
        self.env = env

    def _keys(self):
        e = self.env
        keys = ["rew_" + n for n in e.episode_sum_names]
        if e.cfg.commands.command_curriculum:
            for n in ("duration", "bound", "offset", "phase", "freq", "x_vel", "y_vel", "yaw_vel"):
                keys += [f"min_command_{n}", f"max_command_{n}"]
            if e.cfg.commands.num_commands > 9:
                keys += ["min_command_swing_height", "max_command_swing_height"]
            keys += [f"command_area_{c}" for c in e.category_names] + ["min_action", "max_action"]
        return keys

    def __iter__(self):
        return iter(self._keys())

    def __len__(self):
        return len(self._keys())

    def __getitem__(self, key):
        e = self.env
        log = e.buffers.episode_log
        if key.startswith("rew_"):
            i = e.episode_sum_names.index(key[4:])
            return log[i] / log[-1].clamp(min=1.0)
        col = {"duration": 8, "bound": 7, "offset": 6, "phase": 5, "freq": 4, "x_vel": 0, "y_vel": 1, "yaw_vel": 2,
               "swing_height": 9}
        if key.startswith("min_command_"):
            return e.buffers.commands[col[key[12:]]].min()
        if key.startswith("max_command_"):
            return e.buffers.commands[col[key[12:]]].max()
        if key.startswith("command_area_"):
            w = e.buffers.curriculum_weights[e.category_names.index(key[13:])]
            return w.sum() / w.numel()
        if key == "min_action":
            return e.buffers.actions.min()
        if key == "max_action":
            return e.buffers.actions.max()
        raise KeyError(key)

    def consume(self):
        """Snapshot the running means as floats and restart the accumulation (one host sync, used at log time)."""
        out = {k: float(v) for k, v in self.items()}
        self.env.buffers.episode_log.zero_()
        return out


class _CurriculumDistribution(_LazyMapping):
    """`extras["curriculum/distribution"]` (reference legged_robot.py:229-232)."""

    def __init__(self, env):
        self.env = env

    def __iter__(self):
        for c in self.env.category_names:
            yield f"weights_{c}"
            yield f"grid_{c}"

    def __len__(self):
        return 2 * len(self.env.category_names)

    def __getitem__(self, key):
        kind, cat = key.split("_", 1)
        i = self.env.category_names.index(cat)
        self.env.sync_curricula_from_device()
        return self.env.curricula[i].weights if kind == "weights" else self.env.curricula[i].grid


class _SimFaults(_LazyMapping):
    """`extras["sim_faults"]`: occurrences per fault site since the counters were last consumed (include/go1sim.h
    `Go1FaultBit`).  The reference has no such entry — PhysX never returns a non-finite state; here every containment
    of a failed environment is reported instead of hidden.  Lazy: device reads happen on access only."""

    def __init__(self, env):
        self.env = env

    def __iter__(self):
        return iter(H.FAULT_NAMES[b] for b in sorted(H.FAULT_NAMES))

    def __len__(self):
        return len(H.FAULT_NAMES)

    def __getitem__(self, key):
        for b, name in H.FAULT_NAMES.items():
            if name == key:
                return self.env.buffers.fault_counts[b]
        raise KeyError(key)

    def consume(self):
        """Counts as ints (one host sync) and restart; `fatal` = occurrences that ended an episode."""
        counts = self.env.buffers.fault_counts.tolist()
        self.env.buffers.fault_counts.zero_()
        out = {name: int(counts[b]) for b, name in sorted(H.FAULT_NAMES.items())}
        out["fatal"] = sum(int(counts[b]) for b in H.FAULT_NAMES if (H.FAULT_FATAL_MASK >> b) & 1)
        drops = self.env.buffers.contact_drop_counts.tolist()          # contact points that found no solver slot, per class
        self.env.buffers.contact_drop_counts.zero_()
        if any(drops):
            out["contact_dropped_by_class"] = {name: int(drops[c]) for c, name in sorted(H.CONTACT_CLASS_NAMES.items()) if drops[c]}
        return out


class LeggedRobot(BaseTask):
    # The measurement families, one row each, in the order step() launches them: the name load_state() reports, the attribute the
    # family object is kept under, the host module and the class it is made of (the module is imported by the family's first start_*()),
    # and the method step() calls while the family is armed.  The behaviour table has none: it is folded inside the scalar table's branch
    # only.  The reward family's accumulate() takes the gravity of the step just taken.  step() spells both out.
    _FAMILIES = (("metrics", "_metrics", "go1eval_host", "Go1Eval", "accumulate"),
                 ("behaviour", "_behaviour", "go1eval_host", "Go1Behaviour", None),
                 ("trace", "_trace", "go1eval_host", "Go1Trace", "record"),
                 ("terrain", "_traversal", "go1eval_host", "Go1Terrain", "accumulate"),
                 ("joints", "_joints", "go1eval_host", "Go1Joints", "accumulate"),
                 ("feet", "_feet", "go1feet_host", "Go1Feet", "accumulate"),
                 ("trunk", "_trunk", "go1trunk_host", "Go1Trunk", "accumulate"),
                 ("gait", "_gait", "go1gait_host", "Go1Gait", "accumulate"),
                 ("spectrum", "_spectrum", "go1spectrum_host", "Go1Spectrum", "accumulate"),
                 ("placement", "_place", "go1place_host", "Go1Place", "accumulate"),
                 ("rewards", "_reward", "go1reward_host", "Go1Reward", "accumulate"),
                 ("episodes", "_episodes", "go1episode_host", "Go1Episodes", "accumulate"),
                 ("sensitivity", "_sens", "go1sens_host", "Go1Sensitivity", "accumulate"),
                 ("observations", "_obs", "go1obs_host", "Go1Observations", "accumulate"))
    _STEPPED = tuple((attr, method) for _, attr, _, _, method in _FAMILIES if method)
    # load_state() is refused while one of them is armed: their accumulators are not part of a saved state
    _STATE_FAMILIES = tuple((name, attr) for name, attr, _, _, _ in _FAMILIES)
    _HOST = {attr: (module, cls) for _, attr, module, cls, _ in _FAMILIES}
    _HOST["_push"] = ("go1eval_host", "Go1Push")          # made by the first push_robots(); neither stepped nor a state family

    def __init__(self, cfg, sim_params, physics_engine, sim_device, headless, eval_cfg=None,
                 initial_dynamics_dict=None):
        self.cfg = cfg
        self.eval_cfg = eval_cfg
        self.sim_params = sim_params
        self.height_samples = None
        self.debug_viz = False
        self.init_done = False
        self.initial_dynamics_dict = initial_dynamics_dict
        self._render = None               # go1render_host.Go1Render, created by the first start_recording() / render()
        self._frames = [[], []]           # per camera: the last complete recording handed out
        for attr in self._HOST:           # _metrics ... _obs and _push: each made by the first start_*() / push_robots() of its family
            setattr(self, attr, None)
        self._state = None                # go1state_host.Go1State, created by the first save_state() / load_state()
        if eval_cfg is not None:          # reference legged_robot.py:41-42
            self._parse_cfg(eval_cfg)
        self._parse_cfg(cfg)
        super().__init__(cfg, sim_params, physics_engine, sim_device, headless, eval_cfg)
        self._init_buffers()
        self.init_done = True
        self.record_now = False
        self.record_eval_now = False
        self.collecting_evaluation = False
        self.num_still_evaluating = 0

    # ------------------------------------------------------------------------------------------------
    def _parse_cfg(self, cfg):
        """reference legged_robot.py:1716-1732 (derived step counts are written back into cfg, as there)."""
        self.dt = H.policy_dt(cfg)
        self.obs_scales = cfg.obs_scales
        self.curriculum_thresholds = vars(cfg.curriculum_thresholds)
        cfg.command_ranges = vars(cfg.commands)
        if cfg.terrain.mesh_type not in ('heightfield', 'trimesh'):
            cfg.terrain.curriculum = False
        cfg.env.max_episode_length = np.ceil(cfg.env.episode_length_s / self.dt)
        self.max_episode_length = cfg.env.max_episode_length
        dr = cfg.domain_rand
        dr.push_interval = np.ceil(dr.push_interval_s / self.dt)
        dr.rand_interval = np.ceil(dr.rand_interval_s / self.dt)
        dr.gravity_rand_interval = np.ceil(dr.gravity_rand_interval_s / self.dt)
        dr.gravity_rand_duration = np.ceil(dr.gravity_rand_interval * dr.gravity_impulse_duration)

    def create_sim(self):
        """reference legged_robot.py:493-515 + _create_envs :1481-1609: terrain, origins, per-env dynamics
        parameters, then the simulator instance (go1sim_create replaces gym.create_sim / prepare_sim)."""
        cfg = self.cfg
        mesh_type = cfg.terrain.mesh_type
        if mesh_type not in (None, 'plane', 'heightfield', 'trimesh'):
            raise ValueError("Terrain mesh type not recognised. Allowed types are [None, plane, heightfield, trimesh]")
        self.up_axis_idx = 2
        if self.eval_cfg is not None:
            et = self.eval_cfg.terrain
            if et.mesh_type in ('heightfield', 'trimesh') and mesh_type not in ('heightfield', 'trimesh'):
                # (the reference builds no Terrain then, legged_robot.py:500-505, and fails in _get_env_origins)
                raise ValueError("eval_cfg.terrain.mesh_type is a generated terrain but cfg.terrain.mesh_type is not: the "
                                 "evaluation region is appended to the training terrain (terrain.py:37-54)")
            if mesh_type in ('heightfield', 'trimesh') and et.mesh_type in ('heightfield', 'trimesh') and \
                    (et.horizontal_scale, et.vertical_scale) != (cfg.terrain.horizontal_scale, cfg.terrain.vertical_scale):
                raise ValueError("eval_cfg.terrain: horizontal_scale / vertical_scale must equal the training terrain's (both "
                                 "regions live in one height field, converted with the training scales: terrain.py:30-36)")
            if self.num_train_envs % 16 != 0:
                raise ValueError(f"eval_cfg: cfg.env.num_envs = {self.num_train_envs} must be a multiple of 16 (the step kernel "
                                 f"selects the train / evaluation configuration per wavefront of 16 environments)")
        if mesh_type in ('heightfield', 'trimesh'):
            if self.eval_cfg is not None and self.eval_cfg.terrain.mesh_type in ('heightfield', 'trimesh'):
                # reference legged_robot.py:502-503: a second tile grid for the evaluation environments behind the training one
                self.terrain = Terrain(cfg.terrain, self.num_train_envs, self.eval_cfg.terrain, self.num_eval_envs)
            else:
                self.terrain = Terrain(cfg.terrain, self.num_train_envs)
            hs = self.terrain.heightsamples
            self.height_samples = torch.tensor(hs).view(self.terrain.tot_rows, self.terrain.tot_cols).to(self.device)
        seed = int(getattr(cfg, "seed", getattr(cfg.env, "seed", 0)))
        offset = int(getattr(cfg.env, "env_id_offset", 0))
        # Environments sharded over ranks (one process per GPU): the command curriculum stays ONE global curriculum — every
        # rank adds up the per-bin success counts of all shards before the weight update, so weights, CDFs and therefore
        # the sampled commands are those of a single-GPU run over the concatenated shards (RNG streams are
        # keyed by global env id).  one int32 all-reduce of the K x 4 x 441 success counts every K = commands.curriculum_update_interval env steps (7 KB per step at the default K = 1); `Cfg.commands.global_curriculum = False` keeps
        # per-rank curricula instead.
        import torch.distributed as dist
        self._curriculum_sync = bool(dist.is_available() and dist.is_initialized()
                                     and (dist.get_world_size() > 1 or os.environ.get("GO1_FORCE_DP", "0") not in ("", "0"))
                                     and cfg.commands.command_curriculum and getattr(cfg.commands, "global_curriculum", True))
        self.sim_config, self.sim_meta = H.build_sim_config(
            cfg, num_envs=self.num_envs, seed=seed, env_id_offset=offset,
            # solver sweeps per substep = the reference's PhysX setting (num_position_iterations = 4, num_velocity_iterations
            # = 0, legged_robot_config.py:413-414); `num_solver_sweeps` overrides it
            solver_iterations=int(getattr(H.physx_section(cfg), "num_solver_sweeps",
                                          getattr(H.physx_section(cfg), "num_position_iterations", 4))),
            defer_curriculum_update=self._curriculum_sync)
        self.buffers = B = H.SimBuffers(self.sim_config, self.sim_meta, self.device)
        if mesh_type in ('heightfield', 'trimesh'):
            # 'heightfield': the height field's bilinear surface.  'trimesh': the reference corrects faces steeper than slope_treshold into vertical
            # walls (terrain.py:33-36, convert_heightfield_to_trimesh) — simulated as vertical contact faces on the same height
            # field (include/go1sim.h hf_wall_units)
            H.bind_height_field(self.sim_config, B, self.terrain.heightsamples, cfg.terrain.horizontal_scale,
                                cfg.terrain.vertical_scale, cfg.terrain.border_size,
                                slope_threshold=float(getattr(cfg.terrain, "slope_treshold", 0.75)) if mesh_type == 'trimesh' else None)
        self.num_dof = self.num_dofs = self.num_actuated_dof = 12
        self.num_bodies = 17
        self.dof_names = list(H.DOF_NAMES)
        self.body_names = list(H.BODY_NAMES)
        self.feet_indices = torch.tensor([4, 8, 12, 16], device=self.device)
        self.penalised_contact_indices = torch.tensor(
            [i for i in range(17) if self.sim_config.penalised_body_mask >> i & 1], device=self.device)
        self.termination_contact_indices = torch.tensor(
            [i for i in range(17) if self.sim_config.termination_body_mask >> i & 1], device=self.device)
        self._get_env_origins()
        self._init_custom_buffers__()
        self._call_train_eval(self._randomize_rigid_body_props, torch.arange(self.num_envs, device=self.device))
        self.category_names = self.sim_meta["category_names"]
        self.curricula = self.sim_meta["curricula"]
        # the actuator network: the reference loads resources/actuator_nets/unitree_go1.pt here (legged_robot.py:1238-1240), built
        # into the step library; `control.actuator_net_file` (NOT a reference switch) names a retrained one, read only when the
        # network is the torque model, as there.  One table for all environments (train and evaluation: one robot).
        act_file = getattr(cfg.control, "actuator_net_file", None)
        act_table = H.load_actuator_net(act_file) if act_file is not None and cfg.control.control_type == "actuator_net" else None
        self.sim = H.Go1Sim(self.sim_config, B, self.sim_device_id)
        if act_table is not None:
            if not callable(getattr(self.sim, "set_actuator_net", None)):
                raise RuntimeError(f"Cfg.control.actuator_net_file = {act_file!r}: the simulator {type(self.sim).__name__} cannot load an "
                                   f"actuator network (it only has the built-in one); set actuator_net_file = None to run with that")
            self.sim.set_actuator_net(act_table)
        self.sim_config_eval = None
        if self.eval_cfg is not None:
            # evaluation environments: the train block with the fields the reference dispatches per group taken from
            # eval_cfg (go1sim_host.EVAL_CFG_FIELDS); selected per wavefront inside the kernels
            S_e, _ = H.build_sim_config(self.eval_cfg, num_envs=self.num_envs, seed=seed, env_id_offset=offset,
                                        solver_iterations=self.sim_config.solver_iterations,
                                        defer_curriculum_update=self._curriculum_sync)
            self.sim_config_eval = H.make_eval_sim_config(self.sim_config, S_e)
            self.sim.set_eval_config(self.sim_config_eval, self.num_train_envs)
        B.episode_sums_eval.fill_(-1.0)          # reference legged_robot.py:1420-1424 (only evaluation environments ever write it)

    def _call_train_eval(self, func, env_ids):
        """reference legged_robot.py:531-544: func(ids, cfg) for the training environments, func(ids, eval_cfg) for the others"""
        env_ids_train = env_ids[env_ids < self.num_train_envs]
        env_ids_eval = env_ids[env_ids >= self.num_train_envs]
        ret, ret_eval = None, None
        if len(env_ids_train) > 0:
            ret = func(env_ids_train, self.cfg)
        if len(env_ids_eval) > 0:
            ret_eval = func(env_ids_eval, self.eval_cfg)
            if ret is not None and ret_eval is not None:
                ret = torch.cat((ret, ret_eval), axis=-1)
        return ret

    def _get_env_origins(self):
        """reference legged_robot.py:1675-1714, once per group (`_call_train_eval(self._get_env_origins, ...)`, :1538): the
        training environments on cfg's tiles or grid, the evaluation environments on eval_cfg's."""
        B, N = self.buffers, self.num_envs
        origins = torch.zeros(N, 3, device=self.device)
        self.terrain_levels = torch.zeros(N, dtype=torch.long, device=self.device)
        self.terrain_types = torch.zeros(N, dtype=torch.long, device=self.device)
        self.custom_origins = False
        for lo_, n_, c_ in ((0, self.num_train_envs, self.cfg), (self.num_train_envs, self.num_eval_envs, self.eval_cfg)):
            if n_ == 0:
                continue
            ter = c_.terrain
            self.custom_origins = ter.mesh_type in ("heightfield", "trimesh")      # (an attribute: the last group's value stays)
            if self.custom_origins:
                lo, hi = (ter.min_init_terrain_level, ter.max_init_terrain_level) if ter.curriculum else (0, ter.num_rows - 1)
                if ter.center_robots:
                    lo, hi = ter.num_rows // 2 - ter.center_span, ter.num_rows // 2 + ter.center_span - 1
                    tlo, thi = ter.num_cols // 2 - ter.center_span, ter.num_cols // 2 + ter.center_span - 1
                    levels = torch.randint(lo, hi + 1, (n_,), device=self.device)
                    types = torch.randint(tlo, thi + 1, (n_,), device=self.device)
                else:
                    levels = torch.randint(lo, hi + 1, (n_,), device=self.device)
                    types = torch.div(torch.arange(n_, device=self.device), (n_ / ter.num_cols), rounding_mode='floor').to(torch.long)
                ter.max_terrain_level = ter.num_rows
                ter.terrain_origins = torch.from_numpy(ter.env_origins).to(self.device).to(torch.float)
                self.terrain_levels[lo_:lo_ + n_], self.terrain_types[lo_:lo_ + n_] = levels, types
                origins[lo_:lo_ + n_] = ter.terrain_origins[levels, types]
            else:
                cols = np.floor(np.sqrt(n_))
                rows = np.ceil(n_ / cols)
                xx, yy = torch.meshgrid(torch.arange(rows), torch.arange(cols), indexing="ij")
                origins[lo_:lo_ + n_, 0] = c_.env.env_spacing * xx.flatten()[:n_].to(self.device)
                origins[lo_:lo_ + n_, 1] = c_.env.env_spacing * yy.flatten()[:n_].to(self.device)
        # `_reset_root_states` branches on this attribute for every environment (reference :966-980), whatever its group
        self.sim_config.custom_origins = int(self.custom_origins)
        B.env_origins.copy_(origins.t())
        self.env_origins = B.env_origins.t()

    def _init_custom_buffers__(self):
        """reference legged_robot.py:1260-1297: views of the per-env dynamics parameters (+ optional presets)."""
        B = self.buffers
        B.friction_coeffs.fill_(1.0)          # rigid_shape_props_asset[1].friction: Isaac Gym default material
        B.restitutions.fill_(0.0)
        self.default_friction, self.default_restitution = 1.0, 0.0
        self.friction_coeffs = B.friction_coeffs.unsqueeze(1).expand(-1, 4)
        self.restitutions = B.restitutions.unsqueeze(1).expand(-1, 4)
        self.payloads = B.payloads
        self.com_displacements = B.com_displacements.t()
        self.motor_strengths = B.motor_strengths.t()
        self.motor_offsets = B.motor_offsets.t()
        self.Kp_factors = B.Kp_factors.t()
        self.Kd_factors = B.Kd_factors.t()
        if self.initial_dynamics_dict is not None:
            for k, v in self.initial_dynamics_dict.items():
                v = v.to(self.device)
                if k in ("friction_coeffs", "restitutions"):
                    getattr(B, k).copy_(v.reshape(self.num_envs, -1)[:, 0])
                elif k == "payloads":
                    B.payloads.copy_(v)
                elif k in ("com_displacements", "motor_strengths", "Kp_factors", "Kd_factors"):
                    getattr(B, k).copy_(v.t())

    def _randomize_rigid_body_props(self, env_ids, cfg):
        """reference legged_robot.py:611-633 (set-up time; the step kernel re-draws nothing here unless
        randomize_rigids_after_start, which is not on the train.py path)."""
        B, dr, n = self.buffers, cfg.domain_rand, len(env_ids)
        u = lambda rng, *shape: torch.rand(*shape, device=self.device) * (rng[1] - rng[0]) + rng[0]
        # (values preset through `initial_dynamics_dict` are overwritten by this draw when the switch of their quantity is on, as in
        # the reference: _init_custom_buffers__ :1283-1288 runs before it, :1547-1548)
        if dr.randomize_base_mass:
            B.payloads[env_ids] = u(dr.added_mass_range, n)
        if dr.randomize_com_displacement:
            B.com_displacements[:, env_ids] = u(dr.com_displacement_range, 3, n)
        if dr.randomize_friction:
            B.friction_coeffs[env_ids] = u(dr.friction_range, n)
        if dr.randomize_restitution:
            B.restitutions[env_ids] = u(dr.restitution_range, n)

    def _init_buffers(self):
        """Expose the simulator's SoA buffers under the reference's attribute names (legged_robot.py:1123-1258).
        `.t()` views keep the reference's (N, ...) shapes and in-place write semantics."""
        B, N = self.buffers, self.num_envs
        S = self.sim_config
        self.root_states = B.root_states.t()
        self.base_pos = self.root_states[:, 0:3]
        self.base_quat = self.root_states[:, 3:7]
        self.dof_pos = B.dof_pos.t()
        self.dof_vel = B.dof_vel.t()
        self.contact_forces = B.contact_forces.view(17, 3, N).permute(2, 0, 1)
        self.foot_positions = B.foot_positions.view(4, 3, N).permute(2, 0, 1)
        self.foot_velocities = B.foot_velocities.view(4, 3, N).permute(2, 0, 1)
        self.prev_foot_velocities = B.prev_foot_velocities.view(4, 3, N).permute(2, 0, 1)
        self.base_lin_vel = B.base_lin_vel.t()
        self.base_ang_vel = B.base_ang_vel.t()
        self.projected_gravity = B.projected_gravity.t()
        self.torques = B.torques.t()
        self.actions = B.actions.t()
        self.last_actions = B.last_actions.t()
        self.last_last_actions = B.last_last_actions.t()
        self.joint_pos_target = B.joint_pos_target.t()
        self.last_joint_pos_target = B.last_joint_pos_target.t()
        self.last_last_joint_pos_target = B.last_last_joint_pos_target.t()
        self.last_dof_vel = B.last_dof_vel.t()
        # what the actuator network carries from substep to substep (reference :1226-1231)
        self.joint_pos_err_last = B.joint_pos_err_last.t()
        self.joint_pos_err_last_last = B.joint_pos_err_last_last.t()
        self.joint_vel_last = B.joint_vel_last.t()
        self.joint_vel_last_last = B.joint_vel_last_last.t()
        self.p_gains = torch.full((12,), float(S.kp), device=self.device)                 # :1206-1222 (one gain for every joint)
        self.d_gains = torch.full((12,), float(S.kd), device=self.device)
        self.base_init_state = torch.tensor(list(S.base_init_state), device=self.device)  # :1590-1594
        self.forward_vec = torch.tensor([1.0, 0.0, 0.0], device=self.device).repeat(N, 1)
        self.commands = B.commands.t()[:, :self.cfg.commands.num_commands]
        self.gait_indices = B.gait_indices
        self.clock_inputs = B.clock_inputs.t()
        self.desired_contact_states = B.desired_contact_states.t()
        self.foot_indices = B.foot_indices.t()
        self.episode_length_buf = B.episode_length_buf
        self.reset_buf = B.reset_buf
        self.time_out_buf = B.time_out_buf.view(torch.bool)
        self.last_contacts = B.last_contacts.t().view(torch.bool)
        self.rew_buf = B.rew_buf
        self.obs_buf = B.obs_buf
        self.privileged_obs_buf = B.privileged_obs_buf[:, :self.num_privileged_obs]
        self.default_dof_pos = torch.tensor(list(S.default_dof_pos), device=self.device).unsqueeze(0)
        self.torque_limits = torch.tensor(list(S.torque_limits), device=self.device)
        self.dof_pos_limits = torch.tensor([list(S.dof_pos_soft_lower), list(S.dof_pos_soft_upper)], device=self.device).t()
        self.noise_scale_vec = torch.tensor(list(S.noise_scale_vec)[:self.num_obs], device=self.device)
        self.commands_scale = torch.tensor(list(S.commands_scale)[:self.cfg.commands.num_commands], device=self.device)
        self.reward_names = list(self.sim_meta["reward_names"])
        self.reward_scales = dict(self.sim_meta["reward_scales"])
        self.episode_sum_names = list(self.sim_meta["episode_sum_names"])
        self.episode_sums = {n: B.episode_sums[i] for i, n in enumerate(self.episode_sum_names)}
        self.command_sums = {n: B.command_sums[i] for i, n in enumerate(self.sim_meta["command_sum_names"])}
        self.common_step_counter = 0
        self.measured_heights = B.measured_heights.t() if S.measure_heights else 0
        self.add_noise = self.cfg.noise.add_noise
        nt = self.num_train_envs
        self.extras = {"env_bins": B.env_command_bins[:nt], "train/episode": _EpisodeStats(self), "sim_faults": _SimFaults(self)}
        self.fault_flags = B.fault_flags
        # evaluation environments (reference legged_robot.py:188-195, 1420-1424): their first finished episode's sums;
        # the reference's extras["eval/episode"] is created empty and never filled — kept so for the Runner's logging branch
        self.episode_sums_eval = {n: B.episode_sums_eval[i] for i, n in enumerate(self.episode_sum_names)}
        if self.num_eval_envs > 0:
            self.extras["eval/episode"] = {}
        if self.cfg.env.send_timeouts:
            self.extras["time_outs"] = self.time_out_buf[:nt]
        if self.cfg.commands.command_curriculum:
            self.extras["curriculum/distribution"] = _CurriculumDistribution(self)

    # ------------------------------------------------------------------------------------------------
    def step(self, actions):
        """reference legged_robot.py:60-88 — one kernel launch, no host sync."""
        actions = actions.to(device=self.device, dtype=torch.float32)
        if not actions.is_contiguous():
            actions = actions.contiguous()
        self.sim.step(actions)
        self._record_step()
        for attr, method in self._STEPPED:
            family = getattr(self, attr)
            if family is not None and family.armed:
                if attr == "_reward":
                    family.accumulate(H.gravity_at(self.sim_config, self.common_step_counter))     # (the gravity of the step just taken)
                else:
                    getattr(family, method)()
                if attr == "_metrics" and self._behaviour is not None and self._behaviour.armed:      # (only beside the scalar table)
                    self._behaviour.accumulate()
        if self._curriculum_sync and (self.common_step_counter + 1) % self.sim_config.curriculum_update_interval == 0:
            # ONE exchange for the last `curriculum_update_interval` steps' success counts (a slot per step), then the per-step
            # updates in order: every rank applies what a single process over the concatenated shards would
            import torch.distributed as dist
            dist.all_reduce(self.buffers.curriculum_success)
            self.sim.curriculum_update()
        self.common_step_counter += 1
        return self.obs_buf, self.privileged_obs_buf, self.rew_buf, self.reset_buf, self.extras

    # gravity is a function of (seed, step counter) that kernels and host evaluate alike: no device buffer, no read-back
    @property
    def gravities(self):
        """(N, 3) offset of the gravity vector from (0, 0, -9.8) now in force (reference `self.gravities`, :549-555)"""
        g = torch.from_numpy(H.gravity_at(self.sim_config, self.common_step_counter) - np.array([0.0, 0.0, -9.8], np.float32))
        return g.to(self.device).unsqueeze(0).repeat(self.num_envs, 1)

    @property
    def gravity_vec(self):
        """(N, 3) unit vector along the gravity now in force (reference `self.gravity_vec`, :559)"""
        g = torch.from_numpy(H.gravity_at(self.sim_config, self.common_step_counter))
        return (g / g.norm()).to(self.device).unsqueeze(0).repeat(self.num_envs, 1)

    default_body_mass = 4.801          # base link after the fixed-joint collapse (trunk + imu; csrc/go1_model_data.h GO1_BODY_MASS[0])

    def reset_idx(self, env_ids):
        """reference legged_robot.py:150-239."""
        if len(env_ids) == 0:
            return
        full = len(env_ids) == self.num_envs
        if full:
            self.sim.reset_idx(None)
        else:
            self.sim.reset_idx(torch.as_tensor(env_ids, device=self.device))
        if self._render is not None and self._render.any_armed:     # a reset of the recorded env ends or starts a recording (:1003-1015)
            self._render.note_reset(None if full else env_ids)
        if self._reward is not None and self._reward.armed:         # the reset cleared histories the reward family keeps a snapshot of
            self._reward.snapshot()
        if self._sens is not None and self._sens.armed:             # the reset re-drew the motor parameters: what is in force from now
            self._sens.snapshot()
        if self._obs is not None and self._obs.armed:               # the robots were put elsewhere between two steps: their next step folds no change
            self._obs.note_reset(None if full else env_ids)

    def set_idx_pose(self, env_ids, dof_pos, base_state):
        """reference legged_robot.py:241-261: the buffers ARE the simulator state, so writing them is the push."""
        if len(env_ids) == 0:
            return
        if dof_pos is not None:
            self.dof_pos[env_ids] = dof_pos.to(self.device)
            self.dof_vel[env_ids] = 0.
        self.root_states[env_ids] = base_state.to(self.device)

    def set_main_agent_pose(self, loc, quat):
        self.root_states[0, 0:3] = torch.tensor(loc, device=self.device, dtype=torch.float)
        self.root_states[0, 3:7] = torch.tensor(quat, device=self.device, dtype=torch.float)

    @property
    def env_command_bins(self):
        return self.buffers.env_command_bins.cpu().numpy()

    @property
    def env_command_categories(self):
        return self.buffers.env_command_categories.cpu().numpy()

    def sync_curricula_from_device(self):
        w = self.buffers.curriculum_weights.double().cpu().numpy()
        for cur, row in zip(self.curricula, w):
            cur.weights = row

    def sync_curricula_to_device(self):
        """After a host-side edit of `curricula[i].weights` (e.g. Runner resume, ppo_cse/__init__.py:83-91)."""
        w = np.stack([c.weights for c in self.curricula]).astype(np.float32)
        self.buffers.curriculum_weights.copy_(torch.from_numpy(w))
        cdf = np.cumsum(w.astype(np.float64), axis=1)
        self.buffers.curriculum_cdf.copy_(torch.from_numpy((cdf / cdf[:, -1:]).astype(np.float32)))

    # ---- recording (reference legged_robot.py:1591-1673): libgo1render draws the recorded env on the device -----------------
    # Camera 0 records train env 0, camera 1 the first evaluation env (reference :1600-1604).  The state of a recording lives in
    # a device control block (include/go1render.h): step() enqueues two launches while a camera is armed and none otherwise;
    # get_complete_frames() reads the state once per call.  No-op (as the reference without a camera sensor) when
    # cfg.env.record_video is off, when the simulator's buffers are not on a GPU, and on data-parallel ranks that do not hold
    # global env 0 (one video per run).
    def _renderer(self):
        if self._render is None:
            import go1render_host
            self._render = go1render_host.Go1Render(self.sim_config, self.buffers, num_cameras=2 if self.num_eval_envs > 0 else 1)
        return self._render

    def _can_record(self):
        return bool(self.cfg.env.record_video) and self.buffers.device.type == "cuda" and int(self.sim_config.env_id_offset) == 0

    def _record_step(self):
        if self._render is not None and self._render.any_armed:
            self._render.record()

    def _start(self, cam, env):
        self._frames[cam] = []
        if self._can_record():
            # a recording spans at most the episode between two resets (max_episode_length + 1 steps): the ring never fills
            self._renderer().arm(cam, env, int(self.max_episode_length) + 2)

    def _pause(self, cam):
        self._frames[cam] = []
        if self._render is not None and cam < len(self._render.armed):
            self._render.disarm(cam)

    def _complete(self, cam):
        rec = self._render
        if rec is not None and cam < len(rec.armed) and rec.armed[cam]:
            frames = rec.complete_frames(cam)
            if frames is not None:
                self._frames[cam] = frames
        return self._frames[cam]

    def start_recording(self):
        self.record_now = True
        self._start(0, 0)

    def start_recording_eval(self):
        self.record_eval_now = True
        if self.num_eval_envs > 0:
            self._start(1, self.num_train_envs)

    def pause_recording(self):
        self.record_now = False
        self._pause(0)

    def pause_recording_eval(self):
        self.record_eval_now = False
        self._pause(1)

    def get_complete_frames(self):
        """[] until the recording started by start_recording() is complete, then its frames ((240, 360, 4) uint8 RGBA arrays)
        until pause_recording() / start_recording()"""
        return self._complete(0)

    def get_complete_frames_eval(self):
        return self._complete(1)

    # ---- evaluation metrics (reference go1_gym_learn/eval_metrics/metrics.py, called by the host after every step there):
    # libgo1eval folds the ten scalar metrics of every environment into device accumulators (include/go1eval.h).  While metrics
    # are armed step() enqueues one more launch, after the simulator's and the recorder's; otherwise none, and the library is
    # never imported.  start_metrics(behaviour=True) arms the library's second table as well (gait and behaviour tracking): one
    # further launch per step.
    def _need_gpu_metrics(self, what):
        if self.buffers.device.type != "cuda":
            raise NotImplementedError(f"{what}(): the metrics are a HIP library; this simulator's buffers are not on a GPU")

    def _family(self, what, attr, *args, **kwargs):
        """for the hook `what`: the family object kept under `attr`, made on first use as its class of _FAMILIES on the simulator's
        configuration and buffers and the arguments given (its host module is not imported before that)"""
        self._need_gpu_metrics(what)
        if getattr(self, attr) is None:
            import importlib
            module, cls = self._HOST[attr]
            setattr(self, attr, getattr(importlib.import_module(module), cls)(self.sim_config, self.buffers, *args, **kwargs))
        return getattr(self, attr)

    def _started(self, what, attr, start):
        """for the hook `what`: the family object kept under `attr`, which the hook `start` makes"""
        self._need_gpu_metrics(what)
        if getattr(self, attr) is None:
            raise RuntimeError(f"{what}(): {start}() was never called")
        return getattr(self, attr)

    def _disarm(self, what, *attrs):
        """for the hook `what`: stop the family objects kept under `attrs` that exist; what they measured stays readable"""
        self._need_gpu_metrics(what)
        for attr in attrs:
            if getattr(self, attr) is not None:
                getattr(self, attr).disarm()

    def start_metrics(self, groups, warmup_steps=0, behaviour=False):
        """begin a measurement: `groups` = one int per environment (the row of the result table it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps count towards no metric.  behaviour=True also arms the
        behaviour table (gait, body height, attitude, foot placement and stride tracking): one more launch per step"""
        self._family("start_metrics", "_metrics").arm(groups, warmup_steps)
        if behaviour:
            self._family("start_metrics", "_behaviour", self.dt).arm(groups, warmup_steps)
        elif self._behaviour is not None:
            self._behaviour.disarm()
            self._behaviour.table = None          # a measurement without the behaviour table reads none

    def stop_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_metrics", "_metrics", "_behaviour")

    def read_metrics(self):
        """{metric name: (groups, 6) array of count, mean, std, min, max, nonfinite; "groups": (groups, 5) array of envs, steps,
        episodes_terminated, episodes_timed_out, fall_rate}: one reduction launch and one device-to-host copy.  After
        start_metrics(behaviour=True) also "behaviour": {behaviour metric name: (groups, 6) array}, by one more of each"""
        res = self._started("read_metrics", "_metrics", "start_metrics").results()
        if self._behaviour is not None and self._behaviour.table is not None:
            res["behaviour"] = self._behaviour.results()
        return res

    # ---- the trace (include/go1eval.h, third kernel family): a per-step time series of 24 channels of chosen environments, written on
    # the device by one more launch per step while it is armed, after the metrics launches; independent of start_metrics().  What the
    # reference's scripts/play.py reads to the host after every step, and the step-response analysis of a command switch.
    def start_trace(self, env_ids=None, capacity=None):
        """begin a trace of the environments `env_ids` (None: all) with room for `capacity` steps (default: an episode,
        max_episode_length + 2); steps beyond the capacity are not recorded"""
        self._family("start_trace", "_trace").arm(env_ids, int(self.max_episode_length) + 2 if capacity is None else capacity)

    def stop_trace(self):
        """stop recording; what was recorded stays readable"""
        self._disarm("stop_trace", "_trace")

    def read_trace(self):
        """{channel name: (rows, K) float32 array, "env_ids", "rows", "truncated"}: one device-to-host copy"""
        return self._started("read_trace", "_trace", "start_trace").read()

    def trace_response(self, signals, switch_row, pre, smooth, band, hold, tail, groups, dt=None):
        """the step response of the recorded trace around the command switch at row `switch_row` (go1eval_host.Go1Trace.response;
        dt defaults to the policy step): two launches and one device-to-host copy"""
        trace = self._started("trace_response", "_trace", "start_trace")
        return trace.response(signals, switch_row, pre, smooth, band, hold, tail, self.dt if dt is None else dt, groups)

    # ---- the push and the recovery from it (include/go1eval.h, fourth kernel family).  The reference's _push_robots draws a random
    # planar velocity at a fixed interval and REPLACES the base velocity; this one ADDS a chosen velocity step to chosen environments.
    def push_robots(self, push, env_ids=None):
        """add a velocity step to the base of the environments `env_ids` (None: all, in order) now, between two step() calls:
        push (K, 4) array or tensor of forward, left (the robot's heading frame), up (m/s) and yaw rate (rad/s) steps.  One launch
        on the simulator's stream; the table is checked on the host first (finite, no id twice, ids in range)."""
        pusher = self._family("push_robots", "_push")
        pusher.load(push, env_ids)
        pusher.launch()

    def trace_recovery(self, push_row, pre, smooth, band, hold, groups, dt=None):
        """the recovery of the recorded trace from the push before row `push_row` (go1eval_host.Go1Trace.recovery; dt defaults to
        the policy step): two launches and one device-to-host copy"""
        trace = self._started("trace_recovery", "_trace", "start_trace")
        return trace.recovery(push_row, pre, smooth, band, hold, self.dt if dt is None else dt, groups)

    # ---- terrain traversal (include/go1eval.h, fifth kernel family): does a robot leave the tile it was placed on, fall or time out
    # first, and how high are its base and feet above the ground they are over.  One more launch per step while it is armed, after the
    # trace's; independent of start_metrics() and start_trace().
    def place_on_terrain(self, levels, types, env_ids=None):
        """put the training environments `env_ids` (None: all of them) on the tiles (levels[i], types[i]) of the terrain's tile grid
        (row = level = difficulty, column = type) and reset them there: terrain_levels, terrain_types and the device env_origins
        are set from terrain_origins[levels, types].  A scalar names one tile for all.  Raises on a configuration without a tile
        grid (the plane), on an evaluation environment and on an index outside the grid; reads nothing from the device."""
        ter = self.cfg.terrain
        if ter.mesh_type not in ("heightfield", "trimesh"):
            raise ValueError(f"place_on_terrain(): terrain.mesh_type = {ter.mesh_type!r} has no tile grid")
        if env_ids is None:
            ids = np.arange(self.num_train_envs, dtype=np.int64)
        else:
            ids = np.asarray(torch.as_tensor(env_ids).cpu(), dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.num_train_envs):
            raise ValueError(f"place_on_terrain(): environment ids have to lie in [0, {self.num_train_envs}), the training environments")
        rows, cols = (np.asarray(torch.as_tensor(v).cpu(), dtype=np.int64).reshape(-1) for v in (levels, types))
        if rows.size not in (1, ids.size) or cols.size not in (1, ids.size):
            raise ValueError(f"place_on_terrain(): levels and types have to name one tile, or one per environment ({ids.size})")
        rows, cols = np.broadcast_to(rows, ids.shape), np.broadcast_to(cols, ids.shape)
        if ids.size and (rows.min() < 0 or rows.max() >= ter.num_rows or cols.min() < 0 or cols.max() >= ter.num_cols):
            raise ValueError(f"place_on_terrain(): a tile outside the grid of {ter.num_rows} levels x {ter.num_cols} types")
        if ids.size == 0:
            return
        ids, rows, cols = (torch.from_numpy(np.array(a)).to(self.device) for a in (ids, rows, cols))
        self.terrain_levels[ids], self.terrain_types[ids] = rows, cols
        self.buffers.env_origins[:, ids] = ter.terrain_origins[rows, cols].t()
        self.reset_idx(ids)

    def start_terrain_metrics(self, groups, warmup_steps=0):
        """begin a terrain measurement: `groups` = one int per environment (the row of the result table it counts towards, -1 =
        not evaluated).  Every environment is measured from now for its first episode on its home tile (env_origins +- half a
        tile: terrain_length x terrain_width, or env_spacing in both directions on the plane); steps with episode_length_buf <=
        warmup_steps fold no metric"""
        ter = self.cfg.terrain
        tile = (ter.terrain_length, ter.terrain_width) if ter.mesh_type in ("heightfield", "trimesh") else (self.cfg.env.env_spacing,) * 2
        self._family("start_terrain_metrics", "_traversal", self.dt, *tile).arm(groups, warmup_steps)

    def stop_terrain_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_terrain_metrics", "_traversal")

    def read_terrain_metrics(self):
        """go1eval_host.Go1Terrain.read(): {"metrics": {name: (groups, 6)}, "outcomes": {name: (groups, 6)}, "groups": (groups, 6) array
        of envs, running, traversed, fell, timed_out, success_rate, "status", "steps", "end_step", "max_dist": per environment}: one
        reduction launch and the device-to-host copies"""
        return self._started("read_terrain_metrics", "_traversal", "start_terrain_metrics").read()

    # ---- per-joint actuator usage (include/go1eval.h, sixth kernel family): ten values per joint and step and a torque-speed histogram
    # per joint.  One more launch per step while it is armed, after the terrain family's; independent of the other measurements.
    def start_joint_metrics(self, groups, warmup_steps=0):
        """begin a joint measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps fold nothing.  Saturation is tested against
        rewards.soft_torque_limit x the simulator's torque limit and rewards.soft_dof_vel_limit x the URDF's speed limit (a factor
        the configuration does not carry is 1)"""
        rewards = self.cfg.rewards
        joints = self._family("start_joint_metrics", "_joints", self.dt, H._DOF_VELOCITY, soft_torque_limit=float(getattr(rewards, "soft_torque_limit", 1.0)),
                              soft_vel_limit=float(getattr(rewards, "soft_dof_vel_limit", 1.0)))
        joints.arm(groups, warmup_steps)

    def stop_joint_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_joint_metrics", "_joints")

    def read_joint_metrics(self):
        """go1eval_host.Go1Joints.read(): {"metrics": {name: (groups, 12, 6)}, "groups": (groups, 3) array of envs, steps, resets, "hist":
        (groups, 12, 8, 8) torque-bin x speed-bin counts, "tau_edges", "vel_edges": (12, 9), and the per-environment "steps", "resets",
        "prev_dof_vel", "env_hist"}: one reduction launch and the device-to-host copies"""
        return self._started("read_joint_metrics", "_joints", "start_joint_metrics").read()

    # ---- foot loading (include/go1feet.h, libgo1feet.so: a library of its own): twelve values per foot (contact, vertical and horizontal
    # force, friction use, force excess, impact speed, and per stance peak force, impulse, slip and time) and the GRF profile over the
    # gait phase.  One more launch per step while it is armed, after the joint family's; independent of the other measurements.
    def start_foot_metrics(self, groups, warmup_steps=0):
        """begin a foot-loading measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps fold nothing and break every stance.  The ground's friction and
        max_contact_force are the simulator's (terrain.static_friction, rewards.max_contact_force)"""
        self._family("start_foot_metrics", "_feet", self.dt).arm(groups, warmup_steps)

    def stop_foot_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_foot_metrics", "_feet")

    def read_foot_metrics(self):
        """go1feet_host.Go1Feet.read(): {"metrics": {name: (groups, 4, 6)}, "groups": (groups, 3) array of envs, steps, resets, "profile":
        (groups, 4, 16) mean vertical force per phase bin, "profile_sum", "profile_count", "phase_edges": (17,), and the per-environment
        state}: one reduction launch and the device-to-host copies"""
        return self._started("read_foot_metrics", "_feet", "start_foot_metrics").read()

    # ---- trunk motion (include/go1trunk.h, libgo1trunk.so: a library of its own): seventeen values per environment (roll, pitch and tilt
    # as sines, their rates, the vertical velocity, the trunk's accelerations, the number of supporting feet, the base's margin inside the
    # support polygon, and per straight segment the lateral drift, the heading drift and the progress error) and a tilt histogram.  One
    # more launch per step while it is armed, after the foot family's; independent of the other measurements.
    def start_trunk_metrics(self, groups, warmup_steps=0, segment_steps=50, tilt_limit=0.25):
        """begin a trunk measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps fold nothing and end an open segment.  segment_steps: the policy steps
        of a drift segment; 50 is 1 s, two strides or more at 2 Hz and above, so the sway within a stride cancels.  tilt_limit: the sine
        beyond which a step counts as tilt_exceeded; 0.25 (about 14.5 degrees) is a placeholder, as the push family's band is: no
        measurement of a robot's falls stands behind it"""
        self._family("start_trunk_metrics", "_trunk", self.dt).arm(groups, warmup_steps, segment_steps=segment_steps, tilt_limit=tilt_limit)

    def stop_trunk_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_trunk_metrics", "_trunk")

    def read_trunk_metrics(self):
        """go1trunk_host.Go1Trunk.read(): {"metrics": {name: (groups, 6)}, "groups": (groups, 4) array of envs, steps, resets,
        segments_dropped, "tilt_hist": (groups, 16), "tilt_edges": (17,), the per-environment state and "env_max_tilt"}: one reduction
        launch and the device-to-host copies"""
        return self._started("read_trunk_metrics", "_trunk", "start_trunk_metrics").read()

    # ---- inter-leg coordination (include/go1gait.h, libgo1gait.so: a library of its own): fifteen values per environment (the synchrony of
    # the six pairs of feet, and per stride of the reference foot FL the touchdown phases of the other three against the commanded ones and
    # their touchdown counts), a support-pattern histogram and three touchdown-phase histograms.  One more launch per step while it is
    # armed, after the trunk family's; independent of the other measurements.
    def start_gait_metrics(self, groups, warmup_steps=0, min_stride_steps=1, max_stride_steps=100):
        """begin a gait measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps fold nothing and end an open stride.  min_stride_steps: a touchdown
        of FL sooner after the stride's opening is chatter (1: no debounce); max_stride_steps: a stride that outgrows it is dropped
        (100 is 2 s)"""
        self._family("start_gait_metrics", "_gait").arm(groups, warmup_steps, min_stride_steps=min_stride_steps, max_stride_steps=max_stride_steps)

    def stop_gait_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_gait_metrics", "_gait")

    def read_gait_metrics(self):
        """go1gait_host.Go1Gait.read(): {"metrics": {name: (groups, 6)}, "groups": (groups, 5) array of envs, steps, resets, strides,
        strides_dropped, "support_hist": (groups, 16), "phase_hist": (groups, 3, 16), "phase_centres": (16,), "support_patterns", and the
        per-environment state}: one reduction launch and the device-to-host copies"""
        return self._started("read_gait_metrics", "_gait", "start_gait_metrics").read()

    # ---- spectra (include/go1spectrum.h, libgo1spectrum.so: a library of its own): the power spectral density of forty signals (the
    # twelve clipped actions, torques and joint speeds, the three trunk rates and the vertical velocity) by Welch's method over segments
    # of the family's own step clock, and per closed segment five band figures per signal.  One more launch per step while it is armed,
    # after the gait family's, and one fold launch per segment_steps steps; independent of the other measurements.
    def start_spectrum_metrics(self, groups, warmup_steps=0, segment_steps=100, high_freq=10.0, taper="hann"):
        """begin a spectral measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); a step with episode_length_buf <= warmup_steps or a reset spoils the segment it falls in.  segment_steps: even, 8 to
        128 policy steps per segment (100 is 2 s: 0.5 Hz bins up to 25 Hz); high_freq: high_share counts the bins from this frequency on
        (10 Hz is a placeholder, nothing measured stands behind it); taper: "hann" or "boxcar" """
        self._family("start_spectrum_metrics", "_spectrum", self.dt).arm(groups, warmup_steps, segment_steps=segment_steps, high_freq=high_freq, taper=taper)

    def stop_spectrum_metrics(self):
        """stop recording steps; what was measured stays readable.  A segment left open is discarded, not counted as dropped"""
        self._disarm("stop_spectrum_metrics", "_spectrum")

    def read_spectrum_metrics(self):
        """go1spectrum_host.Go1Spectrum.read(): {"metrics": {row: (groups, 40, 6)}, "groups": (groups, 5) array of envs, steps, resets,
        segments, segments_dropped, "psd": (groups, 40, F) mean density, "psd_segments": (groups, 40), "freq": (F,), "signals": the forty
        names, "high_bin", and the per-environment state}: one reduction launch and the device-to-host copies"""
        return self._started("read_spectrum_metrics", "_spectrum", "start_spectrum_metrics").read()

    # ---- foot placement (include/go1place.h, libgo1place.so: a library of its own): fourteen values per foot (the error against the Raibert
    # heuristic's target in stance and in swing, the touchdown and liftoff points against the nominal stance point, the stance sweep, the
    # stride length and its error, the track width error) and an 8 x 8 footprint map per foot.  One more launch per step while it is
    # armed, after the spectrum family's; independent of the other measurements.
    def start_placement_metrics(self, groups, warmup_steps=0, map_cell=0.03):
        """begin a foot-placement measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps fold nothing and end every open stance and stride.  map_cell: the side
        of a cell of the footprint map in metres (0.03 is a placeholder, nothing measured stands behind it: the map spans +-0.12 m)"""
        self._family("start_placement_metrics", "_place").arm(groups, warmup_steps, map_cell=map_cell)

    def stop_placement_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_placement_metrics", "_place")

    def read_placement_metrics(self):
        """go1place_host.Go1Place.read(): {"metrics": {name: (groups, 4, 6)}, "groups": (groups, 6) array of envs, steps, resets, touchdowns,
        strides, map_outside, "map": (groups, 4, 8, 8), "map_edges": (9,), and the per-environment state}: one reduction launch and the
        device-to-host copies"""
        return self._started("read_placement_metrics", "_place", "start_placement_metrics").read()

    # ---- the reward term by term (include/go1reward.h, libgo1reward.so: a library of its own): the step kernel adds its reward terms to
    # episode_sums and stores only the clipped total; while this family is armed one more launch per step, after the placement family's,
    # evaluates the terms of the step just taken once more with the step kernel's own device functions and folds them per environment
    # (K terms, their sum, its positive and negative part, and the clipped total).  The step of a reset and the step of a teleport are
    # counted, not measured.  Independent of the other measurements.
    def start_reward_metrics(self, groups, warmup_steps=0):
        """begin a reward measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps fold nothing"""
        self._family("start_reward_metrics", "_reward", self.reward_names).arm(groups, warmup_steps)

    def stop_reward_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_reward_metrics", "_reward")

    def read_reward_metrics(self):
        """go1reward_host.Go1Reward.read(): {"names", "scales", "terms": {name: (groups, 6)}, "sum", "positive", "negative", "total":
        (groups, 6), "share": {name: (groups,)}, "groups": (groups, 4) array of envs, measured, reset, teleported env-steps, and the
        per-environment state}: one reduction launch and the device-to-host copies"""
        return self._started("read_reward_metrics", "_reward", "start_reward_metrics").read()

    # ---- whole episodes (include/go1episode.h, libgo1episode.so: a library of its own): the state of every environment's open episode is
    # carried on the device from step to step, and at its close eleven values are folded (length, whether it fell, return, reward per step,
    # discounted return, displacement, path length, the two tracking errors over the episode) and its length enters the histogram of the
    # falls or of the time-outs; the episodes still open at the read are binned by their age: the censored observations of a survival
    # curve.  One more launch per step while it is armed, after the reward family's; independent of the other measurements.
    def start_episode_metrics(self, groups, warmup_steps=0, gamma=0.99, bin_steps=63):
        """begin an episode measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps enter no tracking error (returns and lengths count every step).  gamma:
        the discount of discounted_return, in (0, 1]; bin_steps: the width of a length bin (63 puts the 1001 steps of a 20 s episode into
        the sixteen bins).  Started before reset(), every environment's first episode is seen whole"""
        self._family("start_episode_metrics", "_episodes").arm(groups, warmup_steps, gamma=gamma, bin_steps=bin_steps)

    def stop_episode_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_episode_metrics", "_episodes")

    def read_episode_metrics(self):
        """go1episode_host.Go1Episodes.read(): {"metrics": {name: (groups, 6)}, "groups": (groups, 9) array of envs, steps, closed, fell,
        timed_out, open, cut, unseen, open_steps, "fall_hist", "timeout_hist", "open_hist": (groups, 16), "bin_edges": (17,) in steps,
        "gamma", "bin_steps", and the per-environment state}: one reduction launch and the device-to-host copies"""
        return self._started("read_episode_metrics", "_episodes", "start_episode_metrics").read()

    # ---- robustness against the randomised dynamics (include/go1sens.h, libgo1sens.so: a library of its own): the values of the nine
    # dynamics parameters in force are carried on the device from step to step (the step kernel re-draws them at resets and at the
    # randomisation interval, and on the step of a fall the buffers already hold the respawned robot's), and every step's exposure, fall
    # or time-out, reward, tracking errors and power are charged to the bin of the value that was in force.  One more launch per step
    # while it is armed, after the episode family's; independent of the other measurements.
    def start_sensitivity_metrics(self, groups, warmup_steps=0, ranges=None, pair=None):
        """begin a sensitivity measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 = not
        evaluated); steps with episode_length_buf <= warmup_steps enter no tracking error and no power (exposure, falls and rewards count
        every step).  The parameters whose randomize_* switch is on are measured over the configuration's range in sixteen bins;
        ranges = {name: (lo, hi)} replaces a range or adds a parameter (names: go1sens_host.PARAMETERS; None for the span: the
        configuration's range of a parameter whose switch is off).  pair = (name, name): also an
        8 x 8 map over two measured parameters"""
        family = self._family("start_sensitivity_metrics", "_sens")
        family.arm(groups, warmup_steps, ranges=family.ranges_of(self.cfg.domain_rand, ranges), pair=pair)

    def stop_sensitivity_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_sensitivity_metrics", "_sens")

    def read_sensitivity_metrics(self):
        """go1sens_host.Go1Sensitivity.read(): {"parameters", "active", "edges": (9, 17), "value": {name: (groups, 6)}, "curves":
        {quantity: (groups, 9, 16)} of steps, measured, falls, timeouts and the sums of reward, the two tracking errors and power,
        "counts": (groups, 9, 3) unbinned, redraws, bad, "groups": (groups, 2) environments and launches, "pair", "pair_map":
        (groups, 4, 8, 8) or None, and the per-environment state}: one reduction launch and the device-to-host copies"""
        return self._started("read_sensitivity_metrics", "_sens", "start_sensitivity_metrics").read()

    # ---- what the policy is fed (include/go1obs.h, libgo1obs.so: a library of its own): every column of obs_buf, and of
    # privileged_obs_buf when asked, is a channel with its moments, sixteen bins and two tails over a range, the steps at the observation
    # clip, and the moments of its change from one step to the next (the previous value is carried on the device: a reset step already
    # holds the respawned robot's observation and folds no change).  One more launch per step while it is armed, after the sensitivity
    # family's; independent of the other measurements.
    def start_observation_metrics(self, groups, warmup_steps=0, ranges=None, privileged=True):
        """begin an observation measurement: `groups` = one int per environment (the row of the result tables it counts towards, -1 =
        not evaluated); the first warmup_steps steps after the start (or after a reset_idx from outside) enter nothing.  Every channel
        gets sixteen bins over eval_metrics.observations.default_ranges(cfg) (placeholders by kind); ranges = {channel name or kind:
        (lo, hi)} replaces them (observations.ranges_from(an earlier read) builds such a dict).  privileged=False leaves the privileged
        columns out.  Refused if the names the configuration's switches give are not num_obs"""
        self._need_gpu_metrics("start_observation_metrics")
        from go1_gym_learn.eval_metrics import observations
        names, kinds = observations.channel_names(self.cfg, privileged), observations.channel_kinds(self.cfg, privileged)
        named = len(observations.channel_names(self.cfg))
        if named != self.num_obs:
            raise ValueError(f"start_observation_metrics(): the configuration's switches name {named} observation columns, the simulator has {self.num_obs}")
        spans = observations.channel_spans(self.cfg, names, kinds, ranges)
        family = self._family("start_observation_metrics", "_obs")
        family.names, family.kinds = names, kinds
        family.arm(groups, warmup_steps, spans=spans, privileged=privileged)

    def stop_observation_metrics(self):
        """stop folding steps; what was measured stays readable"""
        self._disarm("stop_observation_metrics", "_obs")

    def read_observation_metrics(self):
        """go1obs_host.Go1Observations.read() with the channels' names: {"channels", "kinds", "edges": (C, 17), "clip", "value", "delta":
        (groups, C, 6), "hist": (groups, C, 16), "tails": (groups, C, 3) below, above, at_clip, "groups": (groups, 4) environments,
        launches, measured env-steps, resets (reset steps and resets from outside), and the per-environment state}: one reduction launch and the device-to-host copies"""
        family = self._started("read_observation_metrics", "_obs", "start_observation_metrics")
        return dict(family.read(), channels=list(family.names), kinds=list(family.kinds))

    def last_reward_terms(self):
        """((K + 4, N) scaled terms, sum, positive, negative and total of the last accumulated step, (N,) valid): views, no copy"""
        return self._started("last_reward_terms", "_reward", "start_reward_metrics").last()

    @property
    def reward_functions(self):
        """the reference's list of bound `_reward_*` methods (read by eval_metrics.metrics.auxiliary_rewards).  It exists only while the
        reward family is armed and has accumulated a step: K callables in reward_names order, each returning the LAST step's raw term
        (they do not recompute: called twice they return the same).  Otherwise the attribute does not exist: hasattr() is false."""
        family = self._reward
        if family is None or not family.armed or family.accumulated == 0:
            raise AttributeError(f"'{type(self).__name__}' object has no attribute 'reward_functions'")
        return family.raw_functions()

    # ---- the state (include/go1state.h, libgo1state.so: a library of its own): hold a moment still.  save_state() gathers the full
    # simulator state of chosen environments into a packed snapshot on the device (one launch), load_state() scatters snapshot rows
    # into chosen environments (one launch), re-phased to where the lag and history rings stand now.  Neither runs during step(): an
    # environment that never saves imports nothing.  What a snapshot does not hold: the terrain, the configuration, the host-backend
    # curriculum objects (device_curriculum=False), and the accumulators of the measurement families.
    def _stater(self, what):
        if self._state is None:
            if self.buffers.device.type != "cuda":
                raise NotImplementedError(f"{what}(): the state copies are a HIP library; this simulator's buffers are not on a GPU")
            import go1state_host
            self._state = go1state_host.Go1State(self.sim_config, self.buffers, self.sim)
        return self._state

    def save_state(self, env_ids=None):
        """the full simulator state of the environments `env_ids` (None: all, with the step counter's global companions: curriculum
        weights and counts, episode log, fault counts) as a go1state_host.SimState on the device.  One launch (two for all) on the
        simulator's stream; nothing is read to the host, ids given on the host are checked on the host."""
        return self._stater("save_state").capture(env_ids)

    def load_state(self, state, env_ids=None, rows=None, restore_clock=None):
        """put row rows[k] (None: k) of `state` into environment env_ids[k] (None: the environments in order).  Rows may repeat: one
        robot's state fanned out to many environments; the environments must be distinct.  restore_clock (default: for a whole state
        loaded whole) also restores the global arrays and sets the simulator's and the environment's step counter to the state's, so
        that the counter-based random streams and the gravity schedule replay; otherwise counters and globals stay as they are and a
        branched environment's draws after the load are those of its own index.  Refused while a measurement family, a trace or a
        camera is armed: their accumulators are not part of the state, and a restore is a teleport to them."""
        stater = self._stater("load_state")
        armed = [name for name, attr in self._STATE_FAMILIES if getattr(self, attr) is not None and getattr(self, attr).armed]
        if self._render is not None and self._render.any_armed:
            armed.append("camera")
        if armed:
            raise RuntimeError(f"load_state(): refused while {', '.join(armed)} {'is' if len(armed) == 1 else 'are'} armed: stop "
                               f"{'it' if len(armed) == 1 else 'them'} first (a restore is a teleport to what they accumulate)")
        if restore_clock is None:
            restore_clock = bool(state.whole) and env_ids is None and rows is None
        stater.restore(state, env_ids, rows, restore_global=bool(restore_clock))
        if restore_clock:
            self.sim.set_counters(state.counter, self.sim.counters()[1])
            self.common_step_counter = int(state.counter)

    def render(self, mode="rgb_array"):
        """reference :1612-1620: env 0 from its recording camera, now: (240, 360, 4) uint8 RGBA"""
        assert mode == "rgb_array"
        if self.buffers.device.type != "cuda":
            raise NotImplementedError("render(): the renderer is a HIP library; this simulator's buffers are not on a GPU")
        return self._renderer().image(0).cpu().numpy()
