"""The fixed-order cross-workgroup sums of the PPO update (det_last, csrc/go1ppo.hip) publish their slab rows without a release
fence: write-through (sc1) stores, a vmcnt drain in every storing wave, a relaxed agent-scope ticket, and one acquire in the last
arriver.  An agent-scope release (buffer_wbl2) writes back the whole XCD L2 — in the weight-gradient kernel the weight-slab tiles
just stored beside the bias row — and cost these four kernels about 88 us per mini-batch step.  This compiles the library for
gfx950 with its own flags (no GPU needed) and checks the four kernels' machine code for that and for the pieces of the protocol."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as g

KERNELS = ("loss_kernel", "mse_kernel", "gae_kernel", "wgrad_tn_batched_kernel")


def _hipcc():
    path = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return path if os.path.exists(path) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("go1ppo_isa") / "go1ppo.s")
    flags = [f for f in g.PPO_FLAGS if f != "-shared"]
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(g.CSRC, "go1ppo.hip")], cwd=g.CSRC)
    asm = open(out).read()
    bodies = {}
    for name, body in re.findall(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        for k in KERNELS:
            if re.fullmatch(r"_Z\d+%s\w*" % k, name):
                bodies[k] = [ln.split(";")[0].strip() for ln in body.splitlines()]
    assert sorted(bodies) == sorted(KERNELS), sorted(bodies)
    return bodies


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_release_fence_in_the_fixed_order_sums(kernels, kernel):
    code = kernels[kernel]
    assert not [ln for ln in code if ln.startswith("buffer_wbl2")], kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_slab_rows_are_written_through_and_drained_before_the_ticket(kernels, kernel):
    code = kernels[kernel]
    ticket = [i for i, ln in enumerate(code) if ln.startswith("global_atomic_add ")]
    assert len(ticket) == 1, (kernel, ticket)                   # the one relaxed agent-scope fetch_add on det_count
    t = ticket[0]
    payload = [i for i, ln in enumerate(code[:t]) if re.match(r"(global|buffer)_store_dword(x2|x4)? .* sc1$", ln)]
    assert payload, kernel                                      # write-through slab stores ahead of the ticket
    # the last of them is drained and the workgroup meets before the ticket
    tail = code[payload[-1] + 1:t]
    drain = [i for i, ln in enumerate(tail) if re.match(r"s_waitcnt vmcnt\(0\)", ln)]
    barrier = [i for i, ln in enumerate(tail) if ln == "s_barrier"]
    assert drain and barrier and drain[0] < barrier[-1], (kernel, tail)
    # exactly one acquire (buffer_inv sc1), behind the ticket, waited for before the barrier that releases the reading waves
    inv = [i for i, ln in enumerate(code) if ln.startswith("buffer_inv")]
    assert len(inv) == 1 and inv[0] > t and code[inv[0]] == "buffer_inv sc1", (kernel, inv)
    after = code[inv[0] + 1:]
    wait = next(i for i, ln in enumerate(after) if ln.startswith("s_waitcnt") and "vmcnt(0)" in ln)
    assert wait < next(i for i, ln in enumerate(after) if ln == "s_barrier"), kernel
