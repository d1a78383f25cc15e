"""The lone-wavefront build of the per-edge kernel (rtr_wave_kernel<3, 9, W_THETA1 | W_PER_EDGE>, the SPLIT product of
gik_rtr.hip.h) from its code object: the instruction count of one tCG step (what tools/isa_loop.py counts) and the
register budget (at most 256 VGPRs, no scratch: two waves per SIMD stay possible).  CPU only; skips without the
toolchain or a built library."""
import collections
import os
import re
import subprocess
import tempfile

import pytest

from conftest import REPO

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNEL = "_ZN3gik15rtr_wave_kernelILi3ELi9ELj%dEEEvNS_9SolveArgsE" % (1 | 8)      # W_THETA1 | W_PER_EDGE (gik_wave_kernels.hip.h)
MAX_STEP_INSTRUCTIONS = 185     # 191 before the SPLIT exit test and the per-unit structurizer flag (NOTEBOOK 12)


@pytest.fixture(scope="module")
def code_objects():
    lib = os.environ.get("GIK_LIB_PATH") or os.path.join(REPO, "graphik_amd", "lib", "libgraphik_amd.so")
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF) and os.path.exists(lib)):
        pytest.skip("needs the ROCm LLVM tools and a built libgraphik_amd.so")
    tmp = tempfile.mkdtemp()
    subprocess.check_call(["cp", lib, os.path.join(tmp, "lib.so")])
    subprocess.check_call([OBJDUMP, "--offloading", "lib.so"], cwd=tmp, stdout=subprocess.DEVNULL)
    cos = [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "gfx950" in f]
    for co in cos:
        txt = subprocess.check_output([OBJDUMP, "-d", co]).decode().split("\n")
        starts = [i for i, l in enumerate(txt) if re.match(r"^[0-9a-f]+ <" + re.escape(KERNEL) + ">:", l)]
        if starts:
            end = next((i for i in range(starts[0] + 1, len(txt)) if re.match(r"^[0-9a-f]+ <", txt[i])), len(txt))
            return co, txt[starts[0]:end]
    pytest.fail(KERNEL + " not found in the library")


def test_step_instruction_count(code_objects):
    _, body = code_objects
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
    n = collections.Counter()
    for l in body[big[0][0]:big[1][0]]:
        p = l.split()
        if p and re.match(r"^[a-z_0-9]+$", p[0]):
            n[p[0]] += 1
    total = sum(n.values())
    assert total <= MAX_STEP_INSTRUCTIONS, (total, n.most_common())


def test_registers_and_scratch(code_objects):
    co, _ = code_objects
    notes = subprocess.check_output([READELF, "--notes", co]).decode()
    # the metadata map of each kernel ends with its .name / .symbol; take the map that names this kernel
    entries = re.split(r"\n  - \.", notes)
    mine = [e for e in entries if re.search(r"\.symbol:\s+" + re.escape(KERNEL) + r"\.kd", e)]
    assert len(mine) == 1, len(mine)
    meta = mine[0]
    vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    agpr = int(re.search(r"agpr_count:\s+(\d+)", "." + meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
    assert scratch == 0 and spill == 0, (scratch, spill)
    assert vgpr + agpr <= 256, (vgpr, agpr)
