"""Which headers a translation unit of graphik_amd/csrc/ sees, without a device (docs/NOTEBOOK.md 32).

a. gik_args.h and gik_plan.h are plain C++17: they compile with the plain C++ compiler, no HIP include path given.
b. The compiler's own dependency list (`hipcc -MM`, preprocessing only) of every unit: a kernel unit sees its own family's
   headers and none of another family's; gik_host_anch.hip, which launches no solve kernel, sees none of them at all.
   gik_wave.hip.h is the one header all families share: it holds the cross-lane primitives (dpp_f64, wave_sum, frcp) next
   to the wavefront context, so the workgroup, node-per-lane and quad units may depend on it and on nothing else of the
   wavefront family.
c. build.py's per-unit object cache follows that list: a change in the node-per-lane context header changes the digests of
   the units that include it and of no other, while source_digest, which says whether the library is stale, still changes.
"""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "graphik_amd", "csrc")
WAVE_UNITS = ["gik_k_wave3.hip", "gik_k_wave3_strict.hip", "gik_k_wave2.hip", "gik_k_anch.hip", "gik_k_anch_link.hip",
              "gik_k_anch_scene.hip", "gik_k_anch_self.hip", "gik_k_anch_half.hip"]
FAMILY = {      # context and driver headers, then the family's kernels
    "wave": {"gik_wave_strict.hip.h", "gik_wave_kernels.hip.h"},
    "block": {"gik_block.hip.h", "gik_block_kernels.hip.h"},
    "npt": {"gik_npt.hip.h", "gik_rtrv.hip.h", "gik_npt_kernels.hip.h"},
    "quad": {"gik_quad.hip.h", "gik_quad_kernels.hip.h"},
    "prep": {"gik_goal.hip.h", "gik_prep.hip.h", "gik_prep_quad.hip.h", "gik_recover_seed.hip.h"},
}
SOLVE_SHARED = {"gik_wave.hip.h", "gik_rtr.hip.h", "gik_rcg.hip.h", "gik_sched.hip.h"}      # what solve families share


def _build():
    from graphik_amd import build
    if not build.have_toolchain():
        pytest.skip("no hipcc on this machine")
    return build


def _families(*names):
    return set().union(*(FAMILY[n] for n in names))


def test_family_table_names_existing_headers():
    for h in _families(*FAMILY) | SOLVE_SHARED:
        assert os.path.exists(os.path.join(CSRC, h)), h


@pytest.mark.parametrize("header", ["gik_args.h", "gik_plan.h"])
def test_plain_headers_compile_without_hip(tmp_path, header):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    src = tmp_path / "only.cpp"
    src.write_text('#include "%s"\nint main() { return sizeof(gik::SolveArgs) > 0 ? 0 : 1; }\n' % header)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + CSRC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.fixture(scope="module")
def deps():
    build = _build()
    out = {s: {os.path.basename(h) for h in build._unit_headers(s, ())} for s in build.SOURCES}
    every = {os.path.basename(h) for h in build.headers()}
    # (a unit whose list could not be had falls back to every header, and would fail the tests below, as it should)
    assert all(d and d <= every for d in out.values())
    return out


def test_wavefront_units_see_no_other_family(deps):
    for unit in WAVE_UNITS:
        assert not deps[unit] & _families("block", "npt", "quad", "prep"), (unit, sorted(deps[unit]))
        assert FAMILY["wave"] <= deps[unit] and "gik_kernels.hip.h" not in deps[unit]


@pytest.mark.parametrize("unit,own", [("gik_k_block.hip", "block"), ("gik_k_npt.hip", "npt"), ("gik_k_npt4.hip", "npt")])
def test_workgroup_and_node_per_lane_units_see_no_other_family(deps, unit, own):
    others = _families(*(f for f in FAMILY if f != own))
    assert not deps[unit] & others, (unit, sorted(deps[unit] & others))
    assert FAMILY[own] <= deps[unit] and "gik_kernels.hip.h" not in deps[unit]


def test_prepare_and_quad_units(deps):
    assert not deps["gik_k_prep.hip"] & _families("wave", "block", "npt", "quad")
    assert not deps["gik_k_quad.hip"] & _families("wave", "block", "npt")      # (prep_quad_kernel is the quad unit's)


def test_second_host_unit_sees_no_solve_kernel_header(deps):
    d = deps["gik_host_anch.hip"]
    assert not d & (_families(*FAMILY) | SOLVE_SHARED | {"gik_kernels.hip.h", "gik_instances.h"}), sorted(d)
    assert {"gik_handle.h", "gik_args.h", "gik_plan.h", "gik_anch_glue.hip.h", "gik_anch_seed.hip.h", "gik_retry.hip.h"} <= d


def test_only_the_first_host_unit_sees_the_umbrella(deps):
    assert [u for u, d in deps.items() if "gik_kernels.hip.h" in d] == ["gik_host.hip"]
    assert _families(*FAMILY) | SOLVE_SHARED <= deps["gik_host.hip"]


def test_unit_digest_follows_the_dependency_list(tmp_path, monkeypatch):
    build = _build()
    shutil.copytree(CSRC, tmp_path / "graphik_amd" / "csrc")
    shutil.copytree(os.path.join(REPO, "include"), tmp_path / "include")
    monkeypatch.setattr(build, "REPO", str(tmp_path))
    monkeypatch.setattr(build, "SRC", str(tmp_path / "graphik_amd" / "csrc"))
    before = {s: build._unit_digest(s, ()) for s in build.SOURCES}
    lib_before = build.source_digest()
    with open(tmp_path / "graphik_amd" / "csrc" / "gik_npt.hip.h", "a") as f:
        f.write("// one more line\n")
    after = {s: build._unit_digest(s, ()) for s in build.SOURCES}
    changed = sorted(s for s in build.SOURCES if after[s] != before[s])
    assert changed == ["gik_host.hip", "gik_k_npt.hip", "gik_k_npt4.hip"]
    assert build.source_digest() != lib_before
