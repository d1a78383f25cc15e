"""The lone-wavefront builds of the per-edge kernel after the reduction-to-branch tail of their tCG step was shortened
(docs/NOTEBOOK.md 23), from the code objects: the step's instruction count (extracted as test_lone_wave_step_isa.py
does), the register budget, the wait states between plain_in_exec's last v_cmpx and the next DPP instruction on either
side of the branch, and the register and scratch figures of the five other rtr_wave_kernel builds of
gik_k_wave3_strict.hip, which are the parent commit's.  CPU only; skips without the toolchain or a built library."""
import collections
import os
import re
import subprocess
import tempfile

import pytest

from conftest import REPO

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
W_THETA1, W_SPREAD, W_PER_EDGE = 1, 4, 8      # the bits of WaveBuild (gik_wave_kernels.hip.h) these six builds differ in


def name(slots, theta_one, spread):
    """rtr_wave_kernel<3, slots, flag word> of a per-edge build, mangled."""
    return "_ZN3gik15rtr_wave_kernelILi3ELi%dELj%dEEEvNS_9SolveArgsE" % (slots, W_THETA1 * theta_one | W_SPREAD * spread | W_PER_EDGE)


KERNEL = name(9, 1, 0)
MAX_STEP_INSTRUCTIONS = 179     # 185 in the parent; 183 with |Hdelta|^2 on the distributed sum alone
# (vgpr, agpr, sgpr, scratch bytes, spilled vgprs) of the other five, read from the parent commit's code object
PARENT_FIGURES = {
    name(9, 1, 1): (153, 0, 106, 0, 0),
    name(9, 0, 0): (206, 0, 106, 0, 0),
    name(10, 1, 0): (187, 0, 106, 0, 0),
    name(10, 1, 1): (168, 0, 106, 0, 0),
    name(10, 0, 0): (225, 0, 106, 0, 0),
}
DPP_WAIT_STATES_AFTER_VALU_EXEC_WRITE = 5      # GCNHazardRecognizer::checkDPPHazards


@pytest.fixture(scope="module")
def code_object():
    lib = os.environ.get("GIK_LIB_PATH") or os.path.join(REPO, "graphik_amd", "lib", "libgraphik_amd.so")
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF) and os.path.exists(lib)):
        pytest.skip("needs the ROCm LLVM tools and a built libgraphik_amd.so")
    tmp = tempfile.mkdtemp()
    subprocess.check_call(["cp", lib, os.path.join(tmp, "lib.so")])
    subprocess.check_call([OBJDUMP, "--offloading", "lib.so"], cwd=tmp, stdout=subprocess.DEVNULL)
    for co in [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "gfx950" in f]:
        txt = subprocess.check_output([OBJDUMP, "-d", co]).decode().split("\n")
        if any(re.match(r"^[0-9a-f]+ <" + re.escape(KERNEL) + ">:", l) for l in txt):
            return co, txt
    pytest.fail(KERNEL + " not found in the library")


def body_of(txt, kernel):
    start = next(i for i, l in enumerate(txt) if re.match(r"^[0-9a-f]+ <" + re.escape(kernel) + ">:", l))
    end = next((i for i in range(start + 1, len(txt)) if re.match(r"^[0-9a-f]+ <", txt[i])), len(txt))
    return [l for l in txt[start + 1:end] if l.split() and re.match(r"^[a-z_0-9]+$", l.split()[0])]


def figures(co):
    notes = subprocess.check_output([READELF, "--notes", co]).decode()
    out = {}
    for e in re.split(r"\n  - \.", notes):
        m = re.search(r"\.symbol:\s+(\S+)\.kd", e)
        if m:
            def g(key):
                return int(re.search(key + r":\s+(\d+)", "." + e).group(1))
            out[m.group(1)] = (g(r"\.vgpr_count"), g(r"agpr_count"), g(r"\.sgpr_count"), g(r"\.private_segment_fixed_size"),
                               g(r"\.vgpr_spill_count"))
    return out


def test_step_instruction_count(code_object):
    _, txt = code_object
    body = body_of(txt, KERNEL)
    # one step = the code between two consecutive reductions of the role-swapped loop body (the groups of eight
    # v_permlane32_swap that open them), as tools/isa_loop.py counts it
    idx = [i for i, l in enumerate(body) if "v_permlane32_swap" in l]
    groups, cur = [], [idx[0]]
    for a in idx[1:]:
        if a - cur[-1] < 80:
            cur.append(a)
        else:
            groups.append(cur)
            cur = [a]
    groups.append(cur)
    big = [g for g in groups if len(g) >= 8]
    assert len(big) >= 2, groups
    step = body[big[0][0]:big[1][0]]
    n = collections.Counter(l.split()[0] for l in step)
    total = sum(n.values())
    assert total <= MAX_STEP_INSTRUCTIONS, (total, n.most_common())
    # the exit test is the hand-written one: six v_cmpx, no chain of s_or_b64 behind them
    assert sum(v for k, v in n.items() if k.startswith("v_cmpx_")) == 6 and n["s_or_b64"] == 0, n.most_common()


def test_registers_and_scratch(code_object):
    co, _ = code_object
    vgpr, agpr, _, scratch, spill = figures(co)[KERNEL]
    assert scratch == 0 and spill == 0, (scratch, spill)
    assert vgpr + agpr <= 256, (vgpr, agpr)


def test_other_builds_keep_the_parents_figures(code_object):
    co, _ = code_object
    got = figures(co)
    for kernel, want in PARENT_FIGURES.items():
        assert got[kernel] == want, (kernel, got[kernel], want)


@pytest.mark.parametrize("slots", [9, 10])
def test_no_dpp_in_the_shadow_of_the_exec_write(code_object, slots):
    """A DPP instruction within five wait states of a VALU write of EXEC reads stale lanes.  The compiler's hazard
    recogniser does not look into plain_in_exec's statement, so the distance is checked here: from the last v_cmpx of
    every group, down the fall-through path and down every branch taken from it.  Every instruction counts as one
    wait state (s_nop N as N + 1)."""
    _, txt = code_object
    body = body_of(txt, name(slots, 1, 0))
    addr = [int(re.search(r"//\s*([0-9A-Fa-f]+):", l).group(1), 16) for l in body]
    base = addr[0]
    last = [i for i, l in enumerate(body) if l.split()[0].startswith("v_cmpx_")
            and not body[i + 1].split()[0].startswith("v_cmpx_")]
    assert len(last) == 2, last      # the two role-swapped steps

    def walk(i, left):
        while left > 0:
            op = body[i].split()[0]
            assert "dpp" not in body[i], body[i]
            left -= 1 + (int(body[i].split()[1]) if op == "s_nop" else 0)
            if op.startswith("s_cbranch") or op == "s_branch":
                off = int(re.search(r"\+0x([0-9a-f]+)>", body[i]).group(1), 16)
                walk(addr.index(base + off), left)
                if op == "s_branch":
                    return
            i += 1

    for i in last:
        walk(i + 1, DPP_WAIT_STATES_AFTER_VALU_EXEC_WRITE)
