"""The bulk gate of tests/test_gpu_parity.py (Attribution.finish(): per quantity, the kernel's median / 99 % error inside the tolerances
against the fp32 oracle's) shown to BITE, without a GPU.

The stand-in for the kernel is a second valid fp32 evaluation: the fp32 build of the oracle started from inputs perturbed by one fp32 ulp
(ShadowPert's perturbation), beside the fp64 oracle and the unperturbed fp32 oracle of the parity tests — train_noise, 256 environments,
full steps re-synchronised every step, FULL_STEP_TOL / ROW_TOL.  As it is, the stand-in passes; with its error scaled by 3 (B64 + 3 (Bx - B64))
everything stays inside the tolerances — the rate-of-outliers assertions finish() had before see nothing — and the gate fails, naming the
quantity."""
import numpy as np
import pytest
import torch

from test_gpu_parity import (BULK_MEDIAN_MIN_STEPS, BULK_Q99_MIN_STEPS, FULL_STEP_TOL, ROW_TOL, STATE_KEYS, Attribution,  # noqa: E402  (helpers and
                             grazing_collision_count, make_ratio)                       # constants only: that module's tests need the GPU)
from util import make_sim, randomize_dr

N, STEPS, LONG = 256, 10, 20             # the cases run STEPS steps (2560 environment-steps: a median gate, no quantile gate); LONG: 5120 >= 5000
QUANTITIES = [k for k, _, _ in FULL_STEP_TOL + ROW_TOL]


ROW = tuple(k for k, _, _ in ROW_TOL)


class View:
    """buffers as Attribution reads them (.tensors, attributes), optionally with the error against `ref` scaled in some quantities /
    environments, optionally the first `n` environments only"""

    def __init__(self, B, ref=None, scale=None, n=None):
        self.tensors = {}
        for k in QUANTITIES + ["reset_buf", "contact_signature", "contact_forces"]:
            t = B.tensors[k]
            if scale and k in scale:
                r = ref.tensors[k].double()
                d = (t.double() - r) * 3.0
                if scale[k] is not None:                 # (N,) bool: these environments only
                    m = scale[k].reshape([-1] + [1] * (d.dim() - 1)) if k in ROW else scale[k]      # row-major (N, K) or [C][N]
                    d = torch.where(m, d, d / 3.0)
                t = r + d
            if n is not None:
                t = t[:n] if k in ROW else t[..., :n]
            self.tensors[k] = t.contiguous()

    def __getattr__(self, k):
        try:
            return self.__dict__["tensors"][k]
        except KeyError:
            raise AttributeError(k)


@pytest.fixture(scope="module")
def lines(oracle_lib):
    """every case's Attribution, stepped side by side through ONE run of the three oracles (finish() is each test's own)"""
    cfg, S, meta, B64 = make_sim("train_noise", N, seed=11)
    randomize_dr(B64, 11)
    B64.enable_contact_signature()
    o64 = oracle_lib.Oracle(S, B64)
    o64.reset_idx()
    B64.episode_length_buf[:] = torch.randint(0, S.max_episode_length, (N,), dtype=torch.int32, generator=torch.Generator().manual_seed(2))
    B32, Bx = B64.clone_to("cpu"), B64.clone_to("cpu")
    o32, ox = oracle_lib.Oracle(S, B32, fp32=True), oracle_lib.Oracle(S, Bx, fp32=True)
    g = torch.Generator().manual_seed(77)
    rng = np.random.default_rng(0)
    half = N // 2
    att = {name: Attribution(half if name == "short" else N) for name in ("as it is", "all", "dof_vel", "contact_forces", "tail", "tail-long", "short")}
    for step in range(LONG):
        a = (rng.standard_normal((N, 12)) * (1.0 if step % 2 else 0.3)).astype(np.float32)
        for k in STATE_KEYS:                             # ShadowPert's perturbation: one fp32 ulp
            t = Bx.tensors[k]
            t.mul_(1.0 + (torch.rand(t.shape, generator=g) * 2.0 - 1.0) * 2.0 ** -23)
        o64.step(a)
        o32.step(a)
        ox.step(a)
        ref, v32 = View(B64), View(B32)
        # the tail only: the error of dof_vel scaled where it is among the step's largest tenth — the median stays, the 99 % quantile triples
        r = att["tail"].ratio(Bx.dof_vel, B64.dof_vel, *[t[1:] for t in FULL_STEP_TOL if t[0] == "dof_vel"][0])
        top = r >= r.quantile(0.9)
        cases = {"as it is": View(Bx), "all": View(Bx, B64, {k: None for k in QUANTITIES}), "dof_vel": View(Bx, B64, {"dof_vel": None}),
                 "contact_forces": View(Bx, B64, {"contact_forces": None}), "tail-long": View(Bx, B64, {"dof_vel": top})}
        cases["tail"] = cases["tail-long"]
        for name, Bk in cases.items():
            if step < STEPS or name == "tail-long":
                att[name].step(make_ratio(att[name], FULL_STEP_TOL, ROW_TOL), Bk, ref, v32, reset_key="reset_buf",
                               also_attributed=grazing_collision_count(att[name], Bk, ref, FULL_STEP_TOL, ROW_TOL))
        if step == 0:                                    # a line below the minimum for a median: 128 environment-steps, every error scaled
            sub = [View(B, B64, sc, n=half) for B, sc in ((Bx, {k: None for k in QUANTITIES}), (B64, None), (B32, None))]
            att["short"].step(make_ratio(att["short"], FULL_STEP_TOL, ROW_TOL), *sub, reset_key="reset_buf")
        for B, o in ((B32, o32), (Bx, ox)):              # re-synchronise: one step is compared at a time
            for k, t in B64.tensors.items():
                if t is not None and B.tensors.get(k) is not None:
                    B.tensors[k].copy_(t)
            o.ctr.common_step_counter, o.ctr.lag_head, o.ctr.history_slot = o64.ctr.common_step_counter, o64.ctr.lag_head, o64.ctr.history_slot
    assert float(B64.contact_forces.abs().max()) > 50.0
    return att


def test_a_second_fp32_evaluation_passes_the_gate(lines):
    """the reference staying inside the cap: another valid fp32 evaluation is not told from the fp32 oracle"""
    att = lines["as it is"]
    att.finish("gate: fp32 oracle from inputs perturbed by one ulp")
    assert att.env_steps == N * STEPS and att.bulk_failures == [] and "contact_forces" in att.q_names and "dof_vel" in att.q_names


def test_three_times_the_error_everywhere_fails_the_gate_and_nothing_else(lines):
    att = lines["all"]
    with pytest.raises(AssertionError, match="less accurate in bulk"):
        att.finish("gate: error x3 in every quantity")
    assert att.bad == 0                                  # nothing left a tolerance: every assertion finish() had before the gate passes
    named = {k for k, stat, *_ in att.bulk_failures}
    # (not dof_pos, not rew_buf: q is good to one fp32 ulp, 1e-4 of its tolerance, a step's reward of ~0.02 to 1e-9, 1e-5 of its tolerance; three
    #  times that stays under the gate's floor of four ulps of 1)
    assert {"root_states", "dof_vel", "contact_forces", "torques", "obs_buf"} <= named, named
    assert {stat for _, stat, *_ in att.bulk_failures} == {"median"}        # 2560 environment-steps: no quantile gate


@pytest.mark.parametrize("quantity", ["dof_vel", "contact_forces"])
def test_three_times_the_error_in_one_quantity_names_that_quantity(lines, quantity):
    att = lines[quantity]
    with pytest.raises(AssertionError, match=f"{quantity} median: kernel"):
        att.finish(f"gate: error x3 in {quantity}")
    assert att.bad == 0 and [k for k, *_ in att.bulk_failures] == [quantity], att.bulk_failures


def test_no_gate_below_the_sample_minimums(lines):
    """128 environment-steps: no gate at all; 2560: the median only — a tail three times as heavy passes there and fails, by its 99 % quantile,
    in the line of 5120"""
    assert N // 2 < BULK_MEDIAN_MIN_STEPS <= N * STEPS < BULK_Q99_MIN_STEPS <= N * LONG
    lines["short"].finish("gate: error x3 in every quantity, 128 env-steps")
    lines["tail"].finish("gate: the upper tenth of dof_vel's errors x3, 2560 env-steps")
    att = lines["tail-long"]
    with pytest.raises(AssertionError, match="dof_vel 99 %: kernel"):
        att.finish("gate: the upper tenth of dof_vel's errors x3, 5120 env-steps")
    assert att.bad == 0 and [(k, stat) for k, stat, *_ in att.bulk_failures] == [("dof_vel", "99 %")], att.bulk_failures


def test_exclusions_are_capped():
    Attribution(4, bulk_exclude={"friction_coeffs": "reason", "payloads": "reason"})
    with pytest.raises(AssertionError):
        Attribution(4, bulk_exclude={"a": "x", "b": "y", "c": "z"})
    for k in ("root_states", "dof_pos", "dof_vel", "contact_forces", "rew_buf", "torques", "obs_buf"):
        with pytest.raises(AssertionError):
            Attribution(4, bulk_exclude={k: "never"})
