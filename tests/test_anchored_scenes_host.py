"""Per-goal obstacle scenes of the fixed-anchor solve, everything that needs no GPU: the synthetic scenes of
tests/synth_anchored_scenes.py meet the conditions they claim and bite (the CPU twin's first cost differs between the
three scenes of every goal, and it converges under each), the packing of a scene set and its argument checks, the C ABI
(struct, prototypes, version), where the scene kernels sit in gik_instances.h, and the host validation of
graphik_amd/csrc/gik_scenes.h walked by a stand-alone program, plain and under the sanitizers."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import synth_anchored as sa
import synth_anchored_scenes as ss
from conftest import REPO, make_graph
from parity_util import anchored_numpy_terms

HDR = os.path.join(REPO, "include", "graphik_amd.h")
INSTANCES_H = os.path.join(REPO, "graphik_amd", "csrc", "gik_instances.h")
NEW_ENTRIES = ("gik_solve_batch_scenes", "gik_anchored_ik_batch_scenes", "gik_anchored_clearance_scenes",
               "gik_anchored_link_clearance_scenes", "gik_anchored_ik_batch_retry_scenes")
# A node INSIDE[0] = 1 cm inside a sphere of radius >= 3 cm adds at least (0.03^2 - 0.02^2)^2 = 2.5e-7 to the cost; the
# costs are below 100 and the references agree to 1e-12 of them, so "differs" is asked at 1e-8: forty times below what a
# biting sphere adds, a hundred times above the noise.
DIFFERS = 1e-8


# ---- 1. the scenes meet their conditions -----------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(ss.CASES))
def test_scene_layout(cid):
    sc = ss.build(cid)
    p = sc.p
    nA, nB, stride = ss.CASES[cid]
    assert sc.counts.tolist() == [nA, nB, 0] and sc.stride == stride <= 128 and sc.obs.shape == (3, stride, 4)
    assert (cid == "near9") == (nA == 128)
    if nA < 128:
        assert stride > sc.counts.max()                     # (a scene of 128 spheres fills the largest stride there is)
    flat = p.P.reshape(-1, 3)
    for s in range(3):
        n = sc.counts[s]
        assert np.all(np.isnan(sc.obs[s, n:])) and np.all(np.isfinite(sc.obs[s, :n]))      # padding rows are NaN
        assert np.array_equal(sc.obs[s, :n, :3], sc.scenes[s][:, :3])
        assert np.array_equal(sc.obs[s, :n, 3], sc.scenes[s][:, 3] ** 2)
    for s in (0, 1):
        assert sa.clearance(flat, sc.scenes[s]).min() > sa.MIN_CLEAR          # every hidden point outside every sphere
        for b, (i, k) in enumerate(sc.inside[s]):
            assert p.mask[i] == 1
            depth = -sa.clearance(sc.Y0[b, i], sc.scenes[s])[k]
            assert ss.INSIDE[0] <= depth <= ss.INSIDE[1], (cid, s, b, depth)
    # A and B share no sphere
    assert not {tuple(r) for r in sc.scenes[0].round(12)} & {tuple(r) for r in sc.scenes[1].round(12)}
    if cid == "near9":
        for b in range(ss.B):
            for point in (sc.Y0[b, sc.near_node], p.P[b, sc.near_node]):
                assert (sa.clearance(point, sc.scenes[0]) < sa.NEAR_TAU).sum() >= ss.NEAR_COUNT > 8
    assert sorted(set(ss.SCENE_ID.tolist())) == [0, 1, 2] and len(ss.SCENE_ID) == ss.B


@functools.lru_cache(maxsize=None)
def twin(cid, s, b):
    """oracle.c_oracle.rtr_solve_anchored on goal b of a case under scene s, from the case's start point."""
    from oracle import c_oracle as co
    sc = ss.build(cid)
    p = sc.p
    return co.rtr_solve_anchored(sc.Y0[b], p.D, p.omega, p.psi_L, p.psi_U, *ss.anchor_terms(cid, s, b), traj_cap=32)


@pytest.mark.parametrize("cid", sorted(ss.CASES))
def test_scenes_bite_and_the_twin_converges(cid):
    """For every goal the first cost of the CPU twin differs pairwise between scenes A, B and C, it is the plain numpy
    reference's cost of the start point under that scene, and the twin converges (stop == 0, f < 1e-9) under all three."""
    sc = ss.build(cid)
    Z = np.zeros((sc.p.N, 3))
    for b in range(ss.B):
        f0 = []
        for s in range(3):
            o = twin(cid, s, b)
            assert o["stop"] == 0 and o["f(x)"] < 1e-9, (cid, s, b, o["stop"], o["f(x)"])
            f0.append(float(o["traj"]["f_before"][0]))
            ref = anchored_numpy_terms(sa.free_terms(sc.p), ss.anchor_terms(cid, s, b), sc.Y0[b], Z)[0]
            assert abs(f0[-1] - ref) <= 1e-12 * abs(ref), (cid, s, b, f0[-1], ref)
        for x, y in ((0, 1), (0, 2), (1, 2)):
            assert abs(f0[x] - f0[y]) > DIFFERS, (cid, b, f0)
        assert f0[0] > f0[2] and f0[1] > f0[2]               # spheres only add cost


# ---- 2. packing and argument checks, no device -----------------------------------------------------------------------
def test_packing_and_squared_radius_bits():
    from graphik_amd.engine import SceneSet, pack_scenes
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    robot, graph = make_graph("ur10_table")
    ap = AnchoredProblem(graph, host_only=True)
    table = ap.obstacles
    rng = np.random.RandomState(3)
    odd = np.concatenate([rng.randn(5, 3), rng.uniform(0.01, 0.3, (5, 1))], axis=1)
    obs, counts, stride = pack_scenes([table, odd, np.zeros((0, 4))])
    assert counts.dtype == np.int32 and counts.tolist() == [len(table), 5, 0] and stride == len(table) and obs.shape == (3, stride, 4)
    own = table.copy()
    own[:, 3] = own[:, 3] ** 2                              # AnchoredProblem.__init__'s line
    assert np.array_equal(obs[0].view(np.uint64), own.view(np.uint64))
    assert all(float(obs[1, k, 3]) == float(odd[k, 3]) * float(odd[k, 3]) for k in range(5))      # one rounded product
    assert np.all(np.isnan(obs[1, 5:])) and np.all(np.isnan(obs[2]))
    assert pack_scenes([odd], stride=9)[0].shape == (1, 9, 4)
    # torch input, and the object on the CPU device (no GPU touched): tensors, counts, stride, host copies
    import torch
    S = SceneSet([torch.from_numpy(table), odd, np.zeros((0, 4))], "cpu")
    assert S.n_scene == 3 and S.stride == stride and S.counts.tolist() == counts.tolist()
    assert S.obs.dtype == torch.float64 and S.n_obs.dtype == torch.int32 and tuple(S.obs.shape) == (3, stride, 4)
    assert np.array_equal(S.obs_host, obs, equal_nan=True) and np.array_equal(S.scenes[1], odd)
    d = S.desc(None)
    assert (d.n_scene, d.stride) == (3, stride) and d.d_obs == S.obs.data_ptr() and d.d_n_obs == S.n_obs.data_ptr() and not d.d_scene_id
    assert SceneSet([np.zeros((0, 4))], "cpu").desc(None).d_obs is None      # stride 0: no rows, a null pointer


def test_argument_checks_need_no_device(monkeypatch):
    from graphik_amd import engine
    from graphik_amd.engine import SceneSet
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    robot, graph = make_graph("ur10_table")
    ap = AnchoredProblem(graph, host_only=True)

    def no_device(*a, **k):
        raise AssertionError("a device object was created before the arguments were checked")
    monkeypatch.setattr(engine.SceneSet, "__init__", no_device)
    ok = np.array([[0.0, 0.0, 0.0, 0.1]])
    for bad, match in (([np.zeros((129, 4))], "at most 128"), ([ok, np.array([[0, 0, 0, -0.1]])], "radius"),
                       ([np.array([[0, 0, 0, np.nan]])], "radius"), ([np.array([[0, 0, 0, np.inf]])], "radius"),
                       ([np.array([[np.nan, 0, 0, 0.1]])], "centre"), ([np.array([[0, -np.inf, 0, 0.1]])], "centre"),
                       ([np.zeros((3, 3))], r"\[m, 4\]"), ([np.zeros(4)], r"\[m, 4\]"), ([np.zeros((2, 2, 4))], r"\[m, 4\]"),
                       ([], "at least one scene")):
        with pytest.raises(ValueError, match=match):
            ap.scene_set(bad)
    monkeypatch.undo()
    # scene ids, on a scene set that lives on the CPU device
    S3 = SceneSet([ok, 2 * ok, np.zeros((0, 4))], "cpu")
    S1 = SceneSet([ok], "cpu")
    assert S1.ids(None, (4,)) is None
    assert S3.ids([0, 2, 1, 1], (4,)).tolist() == [0, 2, 1, 1]
    assert tuple(S3.ids(np.zeros((4, 2), dtype=np.int64), (4, 2)).shape) == (4, 2)
    with pytest.raises(ValueError, match="scene_id is required"):
        S3.ids(None, (4,))
    for bad in ([0, 1, 3, 0], [0, -1, 0, 0], np.array([0, 1, 2, 1 << 40])):
        with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
            S3.ids(bad, (4,))
    with pytest.raises(ValueError, match="shape"):
        S3.ids([0, 1, 2], (4,))
    with pytest.raises(ValueError, match="integers"):
        S3.ids([0.5, 1, 2, 0], (4,))


def test_numpy_mirrors_take_a_scene():
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    robot, graph = make_graph("ur10_table")
    ap = AnchoredProblem(graph, host_only=True)
    q = np.random.RandomState(0).uniform(-1, 1, (5, robot.n))
    Y = ap.base.seed_points(q)
    assert np.array_equal(ap.clearance(Y), ap.clearance(Y, obstacles=ap.obstacles))
    assert np.array_equal(ap.link_clearance(Y), ap.link_clearance(Y, obstacles=ap.obstacles))
    moved = ap.obstacles + np.array([0.2, 0.0, 0.0, 0.0])
    assert not np.array_equal(ap.clearance(Y), ap.clearance(Y, obstacles=moved))
    assert not np.array_equal(ap.link_clearance(Y), ap.link_clearance(Y, obstacles=moved))
    assert np.all(np.isposinf(ap.clearance(Y, obstacles=np.zeros((0, 4))))) and np.all(np.isposinf(ap.link_clearance(Y, obstacles=[])))


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------
def _prototypes():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return {m.group(2): (m.group(1), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"\b(int|size_t|double|void)\s+(gik_\w+)\s*\(([^)]*)\)\s*;", hdr)}


def test_header_prototypes_equal_the_binding():
    """The new entries' prototypes in include/graphik_amd.h, argument by argument, against _ffi.SYMBOLS; the struct
    against _ffi.SceneSet; and the ABI version, which stays 12: entry points and one struct were added, nothing moved."""
    from graphik_amd import _ffi
    hdr = open(HDR).read()
    assert int(re.search(r"#define GIK_ABI_VERSION (\d+)", hdr).group(1)) == 12 and _ffi.ABI_VERSION == 12
    protos = _prototypes()
    for name in NEW_ENTRIES:
        ret, args = protos[name]
        res, argtypes = _ffi.SYMBOLS[name]
        assert ret == "int" and res is C.c_int
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for a, ct in zip(args, argtypes):
            if "*" in a:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, a)
                if "gik_scene_set" in a:
                    assert ct is C.POINTER(_ffi.SceneSet), (name, a)
                if "gik_anchored_retry_opts" in a:
                    assert ct is C.POINTER(_ffi.AnchoredRetryOpts), (name, a)
                if "gik_trace" in a:
                    assert ct is C.POINTER(_ffi.Trace), (name, a)
            else:
                assert re.match(r"int\s+\w+$", a) and ct is C.c_int, (name, a)
        assert sum("gik_scene_set" in a for a in args) == 1, name
    # the scene forms take their sibling's arguments plus the scene set (and, gik_anchored_ik_batch_scenes, the mode)
    for name, sibling, extra in (("gik_solve_batch_scenes", "gik_solve_batch", 1), ("gik_anchored_clearance_scenes", "gik_anchored_clearance", 1),
                                 ("gik_anchored_link_clearance_scenes", "gik_anchored_link_clearance", 1),
                                 ("gik_anchored_ik_batch_retry_scenes", "gik_anchored_ik_batch_retry", 1),
                                 ("gik_anchored_ik_batch_scenes", "gik_anchored_ik_batch_seeded", 2)):
        assert len(protos[name][1]) == len(protos[sibling][1]) + extra, name
    body = re.search(r"typedef struct \{([^}]*)\} gik_scene_set;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    decl = [(n.strip().lstrip("*"), "*" in n or t) for t, n in re.findall(r"\b(?:const\s+)?(double|int32_t)\s+([^;]+);", body)]
    assert [n for n, _ in decl] == [n for n, _ in _ffi.SceneSet._fields_] == ["n_scene", "stride", "d_obs", "d_n_obs", "d_scene_id"]
    assert C.sizeof(_ffi.SceneSet) == 32 and _ffi.SceneSet.d_obs.offset == 8 and _ffi.SceneSet.d_scene_id.offset == 24
    doc = re.search(r"per-goal obstacle scenes in the fixed-anchor solve.*?typedef struct", hdr, flags=re.S).group(0)
    assert "PRECONDITION" in doc and "BIT FOR BIT" in doc and "capturing stream" in doc


# ---- 4. where the kernels sit ------------------------------------------------------------------------------------------
ANCH_GROUP = """#define GIK_KERNELS_ANCH(X)                                    \\
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH>(SolveArgs))  \\
  X(void kat_wave_kernel<3, 9, W_ANCH>(KatArgs))               \\
  X(void rtr_wave_kernel<3, 20, W_THETA1 | W_ANCH>(SolveArgs)) \\
  X(void kat_wave_kernel<3, 20, W_ANCH>(KatArgs))
"""
ANCH_LINK_GROUP = """#define GIK_KERNELS_ANCH_LINK(X)                                        \\
  X(void rtr_wave_kernel<3, 9, W_THETA1 | W_ANCH | W_LINKS>(SolveArgs)) \\
  X(void kat_wave_kernel<3, 9, W_ANCH | W_LINKS>(KatArgs))
"""
SCENE_GROUP = ["rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH>", "rtr_wave_scene_kernel<3,20,W_THETA1|W_ANCH>",
               "rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH|W_LINKS>"]


def test_scene_kernels_sit_in_the_table():
    from graphik_amd import build
    import synth_graphs as sg
    text = open(INSTANCES_H).read()
    assert ANCH_GROUP in text and ANCH_LINK_GROUP in text          # the anchored groups: exactly these members, in this order
    assert sg.group_members("GIK_KERNELS_ANCH_SCENE") == SCENE_GROUP
    # one table: every anchored group is in GIK_ALL_KERNELS, the host unit expands that and no group on its own -- nor does
    # any header --, and every scene build is covered by a test that exists
    all_k = sg.macro_body("GIK_ALL_KERNELS")
    assert all(g in all_k for g in ("GIK_KERNELS_ANCH(X)", "GIK_KERNELS_ANCH_SCENE(X)", "GIK_KERNELS_ANCH_LINK(X)",
                                    "GIK_KERNELS_ANCH_SELF(X)", "GIK_KERNELS_ANCH_HALF(X)"))
    csrc = os.path.join(REPO, "graphik_amd", "csrc")
    for header in sorted(f for f in os.listdir(csrc) if f.endswith(".h")):
        assert not re.search(r"GIK_\w+\(GIK_EXTERN_TEMPLATE\)", open(os.path.join(csrc, header)).read()), header
    compiled, cov = sg.compiled_instances(), sg.coverage()
    for inst in SCENE_GROUP:
        assert compiled.count(inst) == 1 and cov.get(inst), inst
        assert all("::" in ref for ref in cov[inst]), cov[inst]
        for ref in cov[inst]:
            path, name = ref.split("::")
            assert re.search(r"^def %s\(" % re.escape(name.split("[")[0]), open(os.path.join(REPO, path)).read(), flags=re.M), ref
    assert "gik_k_anch_scene.hip" in build.SOURCES
    unit = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_k_anch_scene.hip")).read()
    assert "GIK_KERNELS_ANCH_SCENE(GIK_INSTANTIATE)" in unit
    host = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_host.hip")).read()
    assert re.findall(r"GIK_\w+\(GIK_EXTERN_TEMPLATE\)", host) == ["GIK_ALL_KERNELS(GIK_EXTERN_TEMPLATE)"]


# ---- 5. the host validation, walked by a stand-alone program -----------------------------------------------------------
def _build_walk(tmp_path, name, extra):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        hipcc_clang = "/opt/rocm/lib/llvm/bin/clang++"
        assert os.path.exists(hipcc_clang), "no C++ compiler on this machine"
        cxx = hipcc_clang
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(REPO, "graphik_amd", "csrc")] + extra +
                       [os.path.join(REPO, "tests", "host", "scene_set_walk.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def _run_walk(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(run.stdout)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-2000:]
    m = re.match(r"ok shapes (\d+) refused (\d+) clamped (\d+)\n", run.stdout)
    assert m and "FAILED" not in run.stdout, run.stdout
    shapes, refused, clamped = map(int, m.groups())
    assert shapes == 8 * 10 * 8 and 0 < refused < shapes and clamped == 4 * 4 * 14 * 14


def test_scene_set_walk(tmp_path):
    exe, r = _build_walk(tmp_path, "scene_set_walk", [])
    assert r.returncode == 0, r.stderr[-3000:]
    _run_walk(exe)


def test_scene_set_walk_under_the_sanitizers(tmp_path):
    """The same program with -fsanitize=address,undefined: a stand-alone program, nothing loaded into this interpreter."""
    exe, r = _build_walk(tmp_path, "scene_set_walk_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0, r.stderr[-3000:]
    _run_walk(exe)
