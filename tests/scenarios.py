"""The sharpest physics scenarios of the parity tests, built ONCE for the SIMT emulator (tests/test_emu_parity.py) and for the compiled
kernel on the MI355X (tests/test_gpu_scenarios.py): both call the same builders, so both provably run the same inputs.

Four free-flight scenarios, one physics substep at a time in zero gravity — `self_collision` (lower legs swung into each other),
`thigh_capsules` (pair types 1-3), `hip_capsules` (pair types 4 and 5, every joint held by a PD torque recomputed every substep),
`limit_rows` (20 N m held against the hip rate limit / the thigh stops) — and the contact-heavy state of the full-step test (robots thrown
onto the ground in random orientations, joint angles over the whole limit box).

Tiling: the free-flight builders draw for 16 environments (fixed generator seeds, draw order and shapes); for N > 16 environment e gets
the state of environment e % 16 — EVERY buffer is tiled, not only the ones a builder touches — so at N = 16 the inputs are bit for bit
those of the 16-environment build and at N = 40 two full workgroups and a ragged one of 8 compute the same thing.

Events: counters of what the scenario is about, taken from the ORACLE's buffers and contact signature only (or, for the GPU tests' second
look, from the `_sig` twin's own): never from a comparison."""
import numpy as np
import torch

from util import make_sim, self_contacts_listed, self_pair_codes, standing_state

BASE = 16                                             # environments a free-flight builder draws for
SUBSTEPS = {"self_collision": 260, "thigh_capsules": 120, "hip_capsules": 120, "limit_rows": 120}
# joint limits of the Go1 (hip, thigh, calf) x 4 legs
DOF_LO = torch.tensor([-0.802851455917, -1.0471975512, -2.69653369433] * 4).unsqueeze(1)
DOF_HI = torch.tensor([0.802851455917, 4.18879020479, -0.916297857297] * 4).unsqueeze(1)


class Scenario:
    """S, Bc: configuration and CPU buffers (signature enabled) of N environments; torque_fn: None, or Bc -> (12, N) torques to impose
    before every substep (hip_capsules' PD hold); env_dims: buffer name -> the dimension that counts environments (tiled())"""

    def __init__(self, name, S, Bc, torque_fn, env_dims):
        self.name, self.S, self.Bc, self.torque_fn, self.env_dims = name, S, Bc, torque_fn, env_dims
        self.N = Bc.root_states.shape[1]
        self.substeps = SUBSTEPS[name]
        self.events = Events()

    def not_tiled(self, B, keys=None):
        """names of the buffers of B (any device) in which some environment e >= 16 is not bit-identical to environment e % 16"""
        idx = torch.arange(self.N) % BASE
        names, flags = [], []
        for k, d in self.env_dims.items():
            t = B.tensors.get(k)
            if t is None or (keys is not None and k not in keys):
                continue
            ref = t.narrow(d, 0, BASE).index_select(d, idx.to(t.device))
            ne = t != ref
            if t.is_floating_point():
                ne = ne & ~(t.isnan() & ref.isnan())
            names.append(k)
            flags.append(ne.any())
        if not flags:
            return []
        flags = torch.stack(flags).cpu().tolist()          # (one transfer for all buffers)
        return [k for k, f in zip(names, flags) if f]


def _free_flight(name, N, fill):
    """fill(S, B) -> extras builds the 16-environment state; for N > 16 every buffer of a fresh N-environment set is tiled from it"""
    assert N >= BASE
    extra = {"domain_rand": dict(randomize_gravity=False)}

    def fresh(n):
        cfg, S, meta, B = make_sim("train", n, extra=extra)
        S.gravity[0] = S.gravity[1] = S.gravity[2] = 0.0
        return S, B
    S16, B16 = fresh(BASE)
    extras = fill(S16, B16)
    B16.enable_contact_signature()
    idx = torch.arange(N) % BASE
    env_dims = {}
    if N == BASE:                                      # nothing to tile (and nothing for not_tiled() to compare)
        return S16, B16, env_dims, extras, idx
    # the dimension in which a buffer's shape differs between the two sets counts environments
    S, B = fresh(N)
    B.enable_contact_signature()
    for k, t in B16.tensors.items():
        tn = B.tensors.get(k)
        if t is None or tn is None:
            assert t is None and tn is None, k
            continue
        differ = [d for d in range(t.dim()) if t.shape[d] != tn.shape[d]]
        assert len(differ) <= 1 and t.dim() == tn.dim(), (k, t.shape, tn.shape)
        if differ:
            assert t.shape[differ[0]] == BASE, (k, t.shape)
            env_dims[k] = differ[0]
        tn.copy_(t.index_select(differ[0], idx) if differ else t)
    return S, B, env_dims, extras, idx


def self_collision(N=BASE):
    """in free flight the hips swing the lower legs into each other (left-right and, with the thighs, front-rear) and fold the feet
    against the trunk"""
    def fill(S, Bc):
        assert S.self_collision == 1
        standing_state(S, Bc, z=3.0)
        g = torch.Generator().manual_seed(5)
        Bc.torques.zero_()
        Bc.torques[[0, 6]] = -1.0
        Bc.torques[[3, 9]] = 1.0                                   # hips: left and right legs towards each other
        Bc.torques[[1, 4], 4:8] = 1.5                              # envs 4-7: front thighs back ...
        Bc.torques[[7, 10], 4:8] = -1.5                            # ... rear thighs forward: front-rear pairs
        Bc.torques[[0, 3, 6, 9], 4:8] = 0.0
        Bc.torques[[2, 5, 8, 11], 8:12] = -3.0                     # envs 8-11: calves fold up, thighs swing the feet to the belly
        Bc.torques[[1, 4, 7, 10], 8:12] = torch.tensor([3.0, 3.0, -3.0, -3.0]).unsqueeze(1)
        Bc.torques[[0, 3, 6, 9], 8:12] = 0.0
        Bc.torques[:, 12:16] = torch.empty(12, 4).uniform_(-2.0, 2.0, generator=g)
    S, B, env_dims, _, _ = _free_flight("self_collision", N, fill)
    return Scenario("self_collision", S, B, None, env_dims)


def thigh_capsules(N=BASE):
    """the front hips roll inwards, one thigh pitched forward and one back, and the thighs scissor into each other"""
    def fill(S, Bc):
        standing_state(S, Bc, z=3.0)
        g = torch.Generator().manual_seed(7)
        Bc.dof_pos[:] = torch.tensor([-0.3, 1.1, -1.0, 0.3, -0.5, -1.0, 0.1, 1.0, -1.5, -0.1, 1.0, -1.5]).unsqueeze(1)
        Bc.dof_pos[[1, 4]] += torch.empty(2, BASE).uniform_(-0.3, 0.3, generator=g)
        Bc.torques.zero_()
        Bc.torques[0] = -torch.empty(BASE).uniform_(3.0, 8.0, generator=g)
        Bc.torques[3] = torch.empty(BASE).uniform_(3.0, 8.0, generator=g)
        Bc.torques[1] = -torch.empty(BASE).uniform_(0.5, 2.5, generator=g)
        Bc.torques[4] = torch.empty(BASE).uniform_(0.5, 2.5, generator=g)
    S, B, env_dims, _, _ = _free_flight("thigh_capsules", N, fill)
    return Scenario("thigh_capsules", S, B, None, env_dims)


def hip_capsules(N=BASE):
    """a fore lower leg (knee stretched) is swung back into the hind hip of its side (environments 0-7 of 16: type 5; environments 8-15: the
    hind lower leg swung FORWARD into the fore hip = type 4), every joint held by a PD torque recomputed from the oracle's state"""
    def fill(S, Bc):
        standing_state(S, Bc, z=3.0)
        g = torch.Generator().manual_seed(9)
        back = torch.tensor([-0.4, 1.5, -0.98, -0.1, 0.8, -1.5, -0.43, 2.3, -2.5, -0.1, 1.0, -1.5])       # FL lower leg -> RL hip (tests/test_oracle_physics.py)
        fwd = torch.tensor([0.3, 0.0, -1.5, -0.1, 0.8, -1.5, 0.58, -0.4, -1.0, -0.1, 1.0, -1.5])          # RL lower leg -> FL hip (thigh angle < 0: forward)
        Bc.dof_pos[:, :8] = back.unsqueeze(1)
        Bc.dof_pos[:, 8:] = fwd.unsqueeze(1)
        Bc.dof_pos[[0, 6]] += torch.empty(2, BASE).uniform_(-0.15, 0.15, generator=g)
        q_hold = Bc.dof_pos.clone()
        drive = torch.empty(BASE).uniform_(1.0, 2.5, generator=g)
        return q_hold, drive
    S, B, env_dims, (q_hold, drive), idx = _free_flight("hip_capsules", N, fill)
    q_hold, drive = q_hold[:, idx], drive[idx]
    back_envs, fwd_envs = idx < 8, idx >= 8

    def torque_fn(Bc):
        tau = 30.0 * (q_hold - Bc.dof_pos) - 1.0 * Bc.dof_vel
        tau[1, back_envs] = drive[back_envs] - 0.5 * Bc.dof_vel[1, back_envs]          # FL thigh backwards
        tau[7, fwd_envs] = -drive[fwd_envs] - 0.5 * Bc.dof_vel[7, fwd_envs]            # RL thigh forwards
        return tau
    return Scenario("hip_capsules", S, B, torque_fn, env_dims)


def limit_rows(N=BASE):
    """zero gravity, free flight, 20 N m held against the hip velocity limit / the thigh stops"""
    def fill(S, Bc):
        standing_state(S, Bc, z=5.0)
        Bc.torques.zero_()
        Bc.torques[[0, 3, 6, 9], 0:4] = 20.0
        Bc.torques[[1, 4, 7, 10], 4:8] = -20.0
        Bc.torques[:, 8:12] = torch.tensor([20.0, -20.0, 20.0] * 4).unsqueeze(1)
        Bc.dof_vel[[0, 3, 6, 9], 12:16] = 30.0
    S, B, env_dims, _, _ = _free_flight("limit_rows", N, fill)
    return Scenario("limit_rows", S, B, None, env_dims)


FREE_FLIGHT = {"self_collision": self_collision, "thigh_capsules": thigh_capsules, "hip_capsules": hip_capsules, "limit_rows": limit_rows}

# the contact-heavy full steps: error / tolerance of a FULL step (4 substeps without re-synchronisation, joints at their 28 rad/s rate
# limits: a rate error inside its own tolerance moves a joint by 5e-5 rad per substep)
CONTACT_HEAVY_TOL = (("root_states", 1e-3, 1e-3), ("dof_pos", 2e-4, 0), ("dof_vel", 1e-2, 1e-3), ("torques", 5e-3, 0), ("rew_buf", 1e-4, 0),
                     ("contact_forces", 1e-1, 5e-3))
CONTACT_HEAVY_STEPS = 6


def contact_heavy_state(Bc, seed):
    """robots thrown onto the ground in random orientations with folded / splayed legs (joint angles over the whole limit box), into the
    buffers of a pair set up with randomize_dr() and the oracle's reset_idx(); returns the generator of the action stream"""
    N = Bc.root_states.shape[1]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(4, N, generator=g)
    Bc.root_states[3:7] = q / q.norm(dim=0, keepdim=True)
    Bc.root_states[2].uniform_(0.06, 0.25, generator=g)
    Bc.root_states[7:13].uniform_(-1.5, 1.5, generator=g)
    lo = torch.tensor([-0.86, -0.68, -2.81] * 4).unsqueeze(1)
    hi = torch.tensor([0.86, 4.50, -0.89] * 4).unsqueeze(1)
    Bc.dof_pos[:] = lo + (hi - lo) * torch.rand(12, N, generator=g)
    Bc.dof_vel.uniform_(-4, 4, generator=g)
    Bc.episode_length_buf[:] = 5
    return np.random.default_rng(seed + 1)


def contact_heavy_actions(rng, N):
    return (rng.standard_normal((N, 12)) * 1.5).astype(np.float32)


class KernelCounters:
    """The kernel's own `fault_counts`, read BEFORE every re-synchronisation.  The re-synchronisation copies every buffer of the oracle's set over
    the kernel's, the counters included, and the oracle never counts a fault: read after it, they are the oracle's zeros whatever the kernel did."""

    def __init__(self):
        self.faults = None

    def add(self, B, Bc):
        """B: the kernel's buffers after a substep / step that started from the re-synchronised state; Bc: the oracle's"""
        assert int(Bc.fault_counts.sum()) == 0           # (so what B holds is what the kernel counted since the last re-synchronisation)
        f = B.fault_counts.cpu().long()
        self.faults = f if self.faults is None else self.faults + f


class Events:
    """what happened, read off one buffer set's net contact forces and contact signature (include/go1sim.h `contact_signature`, tests/util.py
    self_pair_codes): the oracle's — or, for a second look, a `_sig` instance's own.  Free-flight counters cover environments 0..15."""

    def __init__(self):
        self.leg_leg = self.trunk_leg = self.thigh_pairs = self.limit_rows = self.self_pair_substeps = 0
        self.seen = {5: 0, 6: 0}
        self.peak_listed = self.self_pairs = self.split_substeps = 0

    def substep(self, B):
        """after ONE physics substep (the signature's rows 0..3)"""
        N = B.root_states.shape[1]
        cf = B.contact_forces.cpu().view(17, 3, N)[:, :, :BASE]
        calf = cf[[3, 7, 11, 15]].norm(dim=1) > 0.5
        self.leg_leg += int((calf.sum(0) >= 2).sum())              # two lower legs loaded: a leg-leg row
        self.trunk_leg += int(((cf[0].norm(dim=0) > 0.5) & (calf.sum(0) >= 1)).sum())
        if B.contact_signature is None:
            return
        w2 = B.contact_signature[2, :BASE].cpu().numpy().astype(np.uint32)
        for w in w2.tolist():
            codes = self_pair_codes(w)[0]
            self.thigh_pairs += any(c in (2, 3, 4) for c in codes)  # a pair with a thigh: types 1-3
            if codes[1] in self.seen:                               # pair (0, 2), FL - RL: hip - lower leg, lower leg - hip
                self.seen[codes[1]] += 1
        self.limit_rows += int(((w2 >> 28) & 0xF != 0).sum())       # legs with limit rows
        self.self_pair_substeps += int((w2 & 0xFFFFFFF != 0).sum())

    def full_step(self, B):
        """after a full step (4 substeps x 4 words), every environment"""
        N = B.root_states.shape[1]
        sig = B.contact_signature.cpu().view(4, 4, N).numpy().astype(np.uint32)
        listed = np.array([[bin(int(sig[sb, 0, e])).count("1") + bin(int(sig[sb, 1, e]) & 0x7FFFFFFF).count("1") + self_contacts_listed(sig[sb, 2, e])
                            for e in range(N)] for sb in range(4)])
        self.peak_listed = max(self.peak_listed, int(listed.max()))
        self.self_pairs += int((sig[:, 2] & 0xFFFFFFF != 0).sum())
        # legs holding hip / thigh rows (word 0 bits 20..27: thigh ends, word 1 bits 9..12: thigh walls, 13..20: hip ends): with two or more
        # of them the leg phase of the sweep splits the base (csrc/go1_physics.h "MASS SPLITTING")
        legs_split = sum((((sig[:, 0] >> (20 + 2 * leg)) & 3) | ((sig[:, 1] >> (13 + 2 * leg)) & 3) | ((sig[:, 1] >> (9 + leg)) & 1)) != 0 for leg in range(4))
        self.split_substeps += int((legs_split >= 2).sum())

    def free_flight(self):
        return dict(leg_leg=self.leg_leg, trunk_leg=self.trunk_leg, thigh_pairs=self.thigh_pairs, hip_lower=self.seen[5], lower_hip=self.seen[6],
                    limit_rows=self.limit_rows, self_pair_substeps=self.self_pair_substeps)

    def contact_heavy(self):
        return dict(peak_listed=self.peak_listed, self_pairs=self.self_pairs, split_substeps=self.split_substeps)
