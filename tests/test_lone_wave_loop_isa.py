"""The nine-slot lone-wavefront build of the per-edge kernel (rtr_wave_kernel<3, 9, W_THETA1 | W_PER_EDGE>) after its tCG
loop got a single exit edge (docs/NOTEBOOK.md 34), from the code object: BOTH role-swapped steps of the hot loop -- the
first as tools/isa_loop.py counts it, reduction to reduction; the second from its reduction over the back edge to the
first one's -- their scalar instructions, and the register copies that used to sit between a step's LDS gathers and
the next Hessian product.  CPU only; skips without the toolchain or a built library."""
import collections
import os
import re
import subprocess
import tempfile

import pytest

from conftest import REPO

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "_ZN3gik15rtr_wave_kernelILi3ELi9ELj%dEEEvNS_9SolveArgsE" % (1 | 8)      # W_THETA1 | W_PER_EDGE
# (first step, second step); the parent: 179 and 179 instructions, 18 and 18 of them scalar
MAX_STEP_INSTRUCTIONS = (172, 173)
MAX_STEP_SALU = (13, 14)      # 5 s_nop, 3 s_waitcnt, 2 s_mov_b64 (EXEC), s_cmp, s_cbranch, s_add; + the back edge's s_branch


@pytest.fixture(scope="module")
def steps():
    """The two steps of one round of the hot loop, as lists of disassembly lines."""
    lib = os.environ.get("GIK_LIB_PATH") or os.path.join(REPO, "graphik_amd", "lib", "libgraphik_amd.so")
    if not (os.path.exists(OBJDUMP) and os.path.exists(lib)):
        pytest.skip("needs the ROCm LLVM tools and a built libgraphik_amd.so")
    tmp = tempfile.mkdtemp()
    subprocess.check_call(["cp", lib, os.path.join(tmp, "lib.so")])
    subprocess.check_call([OBJDUMP, "--offloading", "lib.so"], cwd=tmp, stdout=subprocess.DEVNULL)
    body = None
    for co in [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "gfx950" in f]:
        txt = subprocess.check_output([OBJDUMP, "-d", co]).decode().split("\n")
        start = [i for i, l in enumerate(txt) if re.match(r"^[0-9a-f]+ <" + re.escape(KERNEL) + ">:", l)]
        if start:
            end = next((i for i in range(start[0] + 1, len(txt)) if re.match(r"^[0-9a-f]+ <", txt[i])), len(txt))
            body = [l for l in txt[start[0] + 1:end] if l.split() and re.match(r"^[a-z_0-9]+$", l.split()[0])]
            break
    assert body is not None, KERNEL + " not found in the library"
    addr = [int(re.search(r"//\s*([0-9A-Fa-f]+):", l).group(1), 16) for l in body]
    # the reductions of the two steps: the groups of eight v_permlane32_swap that open them
    idx = [i for i, l in enumerate(body) if "v_permlane32_swap" in l]
    groups, cur = [], [idx[0]]
    for a in idx[1:]:
        if a - cur[-1] < 80:
            cur.append(a)
        else:
            groups.append(cur)
            cur = [a]
    groups.append(cur)
    big = [g[0] for g in groups if len(g) >= 8]
    assert len(big) == 2, groups
    # the back edge: the first branch behind the second reduction that goes back in front of the first one
    for i in range(big[1], len(body)):
        op = body[i].split()[0]
        if op == "s_branch" or op.startswith("s_cbranch"):
            target = addr[0] + int(re.search(r"\+0x([0-9a-f]+)>", body[i]).group(1), 16)
            if target <= addr[big[0]]:
                assert op == "s_branch", body[i]      # unconditional: the loop's one exit is the step's own branch
                head = addr.index(target)
                assert big[0] - head < 80, (head, big)      # the loop header is the first step's product
                return body[big[0]:big[1]], body[big[1]:i + 1] + body[head:big[0]]
    pytest.fail("no back edge found behind the second reduction")


def test_both_steps_instruction_count(steps):
    for step, limit in zip(steps, MAX_STEP_INSTRUCTIONS):
        n = collections.Counter(l.split()[0] for l in step)
        print(len(step), n.most_common())
        assert limit < 179 and len(step) <= limit, (len(step), n.most_common())


def test_scalar_instructions_per_step(steps):
    for step, limit in zip(steps, MAX_STEP_SALU):
        n = collections.Counter(l.split()[0] for l in step if l.split()[0].startswith("s_"))
        print(sum(n.values()), n.most_common())
        assert sum(n.values()) <= limit, n.most_common()
        # one branch out of the step, no exit flag tested in the hot path, one wait per owned slot
        assert sum(v for k, v in n.items() if k.startswith("s_cbranch")) == 1, n.most_common()
        assert n["s_and_b64"] + n["s_andn2_b64"] + n["s_or_b64"] == 0, n.most_common()
        assert n["s_waitcnt"] == 3, n.most_common()


def test_no_register_copy_between_the_gathers_and_the_next_product(steps):
    for step in steps:
        ops = [l.split()[0] for l in step]
        reads = [i for i, op in enumerate(ops) if op.startswith("ds_read")]
        assert len(reads) == 8, reads      # the own row and three neighbours, b128 + b64 each
        product = next(i for i in range(reads[-1], len(ops)) if ops[i] == "s_waitcnt")
        assert not [op for op in ops[reads[-1]:product] if op.startswith("v_mov_b64")], step[reads[-1]:product]
        # ... and in the whole step only the one that puts the previous model value next to the new one
        assert sum(op.startswith("v_mov_b64") for op in ops) <= 1, [l for l in step if "v_mov_b64" in l]
