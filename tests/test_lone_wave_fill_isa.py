"""The nine-slot lone wavefront's tCG step (rtr_wave_kernel<3, 9, W_THETA1 | W_PER_EDGE>) with the model test taken in
place (docs/NOTEBOOK.md 38), from the code object: both role-swapped steps as test_lone_wave_loop_isa.py takes them
(its fixture is imported).  What the committed combination achieved; the parent's figures in the comments.  The
deferred recurrences in the reduction's wait states were measured slower and are not in the library, so the five
s_nop of a step are still there.  CPU only; skips without the toolchain or a built library.  Fails on the parent's
library (172 / 173 instructions, 16 v_readlane, one v_mov_b64)."""
import collections

from test_lone_wave_loop_isa import steps  # noqa: F401  (the fixture: the two steps as lists of disassembly lines)

STEP_INSTRUCTIONS = (169, 170)      # parent: 172 / 173
STEP_S_NOP = (5, 5)                 # parent: 5 / 5 (eight wait states; filling them lost 1.8 ms of 77.9)
STEP_V_READLANE = (14, 14)          # parent: 16 / 16 -- the model value is no longer read into scalar registers
STEP_V_MOV_B64 = (0, 0)             # parent: 1 / 1 -- nor the previous one copied back into a vector register


def counts(step):
    return collections.Counter(l.split()[0] for l in step)


def test_instructions_per_step(steps):  # noqa: F811
    for step, want in zip(steps, STEP_INSTRUCTIONS):
        n = counts(step)
        print(len(step), n.most_common())
        assert len(step) <= want, (len(step), n.most_common())


def test_model_value_stays_in_its_lanes(steps):  # noqa: F811
    for step, nop, readlane, mov in zip(steps, STEP_S_NOP, STEP_V_READLANE, STEP_V_MOV_B64):
        n = counts(step)
        assert n["v_readlane_b32"] == readlane, n.most_common()
        assert sum(v for k, v in n.items() if k.startswith("v_mov_b64")) == mov, n.most_common()
        assert n["s_nop"] <= nop, n.most_common()
        # the compares still open with the model test: v_cmpx_lt_f64 on two vector registers
        first = next(l for l in step if l.split()[0].startswith("v_cmpx_"))
        ops = first.split("//")[0].replace(",", " ").split()
        assert ops[0] == "v_cmpx_lt_f64_e64" and ops[2].startswith("v[") and ops[3].startswith("v["), first
