"""Every compiled solve / known-answer kernel instantiation (GIK_ALL_KERNELS in gik_instances.h) is reached by a
case of tests/test_variant_matrix_gpu.py or named existing test, and every case's synthetic graph sits exactly
on the boundary it claims (term counts through engine.build_terms).  No GPU needed."""
import os
import re

import numpy as np
import pytest

import synth_graphs as sg

TESTS = os.path.dirname(os.path.abspath(__file__))


def _gaps(text=None):
    compiled = set(sg.compiled_instances(text))
    cov = sg.coverage()
    wanted = {s for s in compiled if re.match(r"(rtr|rcg|kat|prep)_", s)}
    return sorted(wanted - set(cov)), sorted(set(cov) - compiled)


def test_every_instantiation_has_a_case():
    missing, stale = _gaps()
    assert not missing, f"compiled kernels without a case in tests/synth_graphs.py: {missing}"
    assert not stale, f"coverage entries for kernels gik_instances.h no longer compiles: {stale}"
    assert len(sg.compiled_instances()) == 75      # (what GIK_ALL_KERNELS yields: the parser found every group)


def test_a_new_instantiation_without_a_case_fails():
    with open(sg.INSTANCES_H) as f:
        text = f.read()
    extra = "  X(void rtr_wave_kernel<2, 7, W_THETA1>(SolveArgs))  \\\n"
    anchor = "#define GIK_KERNELS_WAVE2(X)                          \\\n"
    assert anchor in text
    missing, stale = _gaps(text.replace(anchor, anchor + extra))
    assert missing == ["rtr_wave_kernel<2,7,W_THETA1>"] and not stale
    dropped = re.sub(r"[^\n]*X\(void rcg_wave_kernel<2, 31>\(SolveArgs\)\)[^\n]*\n", "", text)
    assert dropped != text
    missing, stale = _gaps(dropped)
    assert not missing and stale == ["rcg_wave_kernel<2,31>"]
    # the self-hinge and half-space groups: a member more, a member less, a group gone (GIK_ALL_KERNELS then names a group
    # that no longer exists)
    extra = "  X(void rtr_wave_kernel<3, 20, W_THETA1 | W_ANCH | W_HALF>(SolveArgs))  \\\n"
    anchor = "#define GIK_KERNELS_ANCH_HALF(X)                                                                  \\\n"
    assert anchor in text
    missing, stale = _gaps(text.replace(anchor, anchor + extra))
    assert missing == ["rtr_wave_kernel<3,20,W_THETA1|W_ANCH|W_HALF>"] and not stale
    dropped = re.sub(r"[^\n]*X\(void kat_wave_kernel<3, 9, W_ANCH \| W_LINKS \| W_SELF>\(KatArgs\)\)[^\n]*\n", "", text)
    assert dropped != text
    missing, stale = _gaps(dropped)
    assert not missing and stale == ["kat_wave_kernel<3,9,W_ANCH|W_LINKS|W_SELF>"]
    with pytest.raises(AssertionError, match="GIK_KERNELS_ANCH_SELF"):
        sg.compiled_instances(text.replace("#define GIK_KERNELS_ANCH_SELF(X)", "#define GIK_KERNELS_ANCH_SELF_GONE(X)"))


def test_the_self_and_half_groups_are_in_the_table():
    """GIK_KERNELS_ANCH_SELF and GIK_KERNELS_ANCH_HALF: six instantiations each, every one compiled once and with an entry
    of its own in EXISTING, the solve builds through a case of the numpy twin's table."""
    import test_anchored_hinge_twin_host as th
    compiled = sg.compiled_instances()
    for group in ("GIK_KERNELS_ANCH_SELF", "GIK_KERNELS_ANCH_HALF"):
        members = sg.group_members(group)
        assert len(members) == 6
        for inst in members:
            assert compiled.count(inst) == 1 and sg.EXISTING.get(inst), inst
            if inst.startswith("rtr_wave_kernel"):
                assert sg.EXISTING[inst] == [sg._HINGE_TWIN] and sg.HINGE_TWIN_CASES.get(inst), inst
    # every case of the twin's table is named by the solve build it pins, and by no other
    flags = {3: "W_LINKS", 5: "W_SELF", 7: "W_LINKS|W_SELF", 9: "W_HALF", 11: "W_LINKS|W_HALF"}
    for case, c in th.CASES.items():
        named = [inst for inst, cases in sg.HINGE_TWIN_CASES.items() if case in cases]
        assert named == [f"rtr_wave_kernel<3,9,W_THETA1|W_ANCH|{flags[c['build']]}>"], (case, named)
    assert all(sg._HINGE_TWIN in sg.EXISTING[inst] for inst in sg.HINGE_TWIN_CASES)
    assert sorted(c for cases in sg.HINGE_TWIN_CASES.values() for c in cases) == sorted(th.CASES)


def test_named_existing_tests_exist():
    for inst, refs in sg.EXISTING.items():
        for ref in refs:
            path, name = ref.split("::")
            with open(os.path.join(os.path.dirname(TESTS), path)) as f:
                assert re.search(rf"^def {name}\(", f.read(), re.M), (inst, ref)
    for cid, c in sg.BATCH_CASES.items():
        assert c["graph"] in sg.CASES, cid


@pytest.mark.parametrize("cid", sorted(sg.CASES))
def test_case_graph_sits_on_its_boundary(cid):
    """The counts a case asks for, as engine.build_terms sees them, and the oracle's index pairs (limit_inds) equal
    build_terms' pairs: a hinge-only pair with psi_L == psi_U is dropped by both, one on top of an equality kept."""
    from oracle.c_oracle import limit_inds
    c = sg.CASES[cid]
    om, pL, pU, D, P = sg.build_graph(c["k"], c["N"], **c["graph"])
    assert om.shape == (c["N"], c["N"]) and P.shape == (c["N"], c["k"])
    n = sg.term_counts(om, pL, pU, c["graph"].get("clique", 0))
    for key, want in c["counts"].items():
        assert n[key] == want, (key, n[key], want)
    il = limit_inds(om, pL, pU)
    assert n["pairs"] == set(zip(il[0].tolist(), il[1].tolist()))
    eq_hinge = (om > 0) & (pL == pU) & (pL > 0)
    lone = (om == 0) & (pL == pU) & (pL > 0)
    assert eq_hinge.any() and lone.any()
    assert not any(lone[i, j] for i, j in n["pairs"])
    if c["graph"].get("scaled"):
        assert not np.allclose(D[om > 0], ((P[:, None] - P[None]) ** 2).sum(-1)[om > 0])
    else:
        assert np.allclose(D, ((P[:, None] - P[None]) ** 2).sum(-1))


@pytest.mark.parametrize("rid", sorted(sg.REFUSED))
def test_refused_graph_sits_on_its_boundary(rid):
    r = sg.REFUSED[rid]
    om, pL, pU, _, _ = sg.build_graph(r["k"], r["N"], **r["graph"])
    n = sg.term_counts(om, pL, pU, r["graph"].get("clique", 0))
    if "outside" in r["graph"]:
        assert n["outside"] == r["graph"]["outside"]
    if "per_node" in r["graph"]:
        assert n["per_node"] == r["graph"]["per_node"]
    if "carriers" in r["graph"]:
        assert n["carriers"] == r["graph"]["carriers"]
    if rid == "r_n129_noclq":
        assert n["carriers"] == 129
