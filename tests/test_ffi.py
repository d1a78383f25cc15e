"""The C-ABI library builds for gfx950, loads, and exports every symbol include/graphik_amd.h
declares.  No compute (no GPU needed)."""
import os
import re

import pytest

from conftest import REPO


def test_header_symbols_are_bound_and_exported():
    from graphik_amd import _ffi, build
    build.build()
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gik_[a-z_]+)\s*\(", hdr))
    assert declared == set(_ffi.SYMBOLS), declared ^ set(_ffi.SYMBOLS)
    L = _ffi.lib()
    for name in declared:
        assert hasattr(L, name)
    assert L.gik_abi_version() == _ffi.ABI_VERSION


def test_struct_layouts_match_header():
    import ctypes as C
    from graphik_amd import _ffi
    # gik_stats: the header says 48 bytes; parse its field list and compare with the ctypes mirror
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gik_stats;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(double|int32_t)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in _ffi.Stats._fields_]
    assert sum(8 if t == "double" else 4 for t, _ in fields) == 48 == C.sizeof(_ffi.Stats)
    assert _ffi.STATS_I32["inner_executed"] == 8 and _ffi.STATS_F64["gradnorm"] == 1 and _ffi.STATS_F64["stepsize"] == 5
    # descriptor structs: same fields in the same order with the same scalar types as the header
    ctype_of = {"double": C.c_double, "int32_t": C.c_int32}
    for cname, mirror in (("gik_template_desc", _ffi.TemplateDesc), ("gik_pipeline_desc", _ffi.PipelineDesc),
                          ("gik_prepare_diag", _ffi.PrepareDiag)):
        nocomment = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, nocomment).group(1)
        decl = []
        for typ, names in re.findall(r"\b(?:const\s+)?(double|int32_t)\s+([^;]+);", body):
            for nm in names.split(","):
                nm = nm.strip()
                decl.append((nm.lstrip("*"), "ptr" if nm.startswith("*") else typ))
        assert [n for n, _ in decl] == [n for n, _ in mirror._fields_], (cname, decl)
        for (n, typ), (_, ct) in zip(decl, mirror._fields_):
            if typ == "ptr":
                assert C.sizeof(ct) == C.sizeof(C.c_void_p), (cname, n)
            else:
                assert ct is ctype_of[typ], (cname, n)
    assert C.sizeof(_ffi.Trace) == 8 + 6 * 8
    assert _ffi.TemplateDesc.N.offset == 4 and _ffi.TemplateDesc.term_i.offset == 16


def _mirrors():
    """C struct name -> ctypes mirror, for the eleven structs of the header."""
    from graphik_amd import _ffi
    return {"gik_template_desc": _ffi.TemplateDesc, "gik_template_info": _ffi.TemplateInfo, "gik_stats": _ffi.Stats,
            "gik_trace": _ffi.Trace, "gik_pipeline_desc": _ffi.PipelineDesc, "gik_anchored_desc": _ffi.AnchoredDesc,
            "gik_retry_opts": _ffi.RetryOpts, "gik_anchored_retry_opts": _ffi.AnchoredRetryOpts,
            "gik_link_desc": _ffi.LinkDesc, "gik_scene_set": _ffi.SceneSet, "gik_prepare_diag": _ffi.PrepareDiag}


def _header_prototypes():
    """include/graphik_amd.h without comments, preprocessor lines and struct bodies -> {name: (return type, [parameter
    types])}, every type as its words joined by one blank with each '*' a word of its own ("const double *")."""
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", " ", hdr, flags=re.M)
    hdr = re.sub(r'extern\s+"C"\s*\{', " ", hdr)
    hdr = re.sub(r"typedef\s+struct\s*\{[^}]*\}\s*\w+\s*;", " ", hdr)
    hdr = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", hdr)
    words = lambda text: " ".join(re.findall(r"\w+|\*", text))      # noqa: E731
    protos = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(gik_[a-z_]+)\s*\(([^)]*)\)\s*;", hdr):
        assert name not in protos, name
        types = []
        for p in ([] if words(params) == "void" else params.split(",")):
            w = words(p).split()
            assert len(w) >= 2, (name, p)      # (a type and the parameter's name)
            types.append(" ".join(w[:-1]))
        protos[name] = (words(ret), types)
    return protos


def _prototype_faults(symbols):
    """Every disagreement between the header's prototypes and a table like _ffi.SYMBOLS, as a list of strings."""
    import ctypes as C
    mirrors = _mirrors()
    scalar = {"int": C.c_int, "int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
    returns = dict(scalar, void=None)
    returns["const char *"] = C.c_char_p
    protos = _header_prototypes()
    faults = [f"{name}: only in one of header and table" for name in sorted(set(protos) ^ set(symbols))]
    for name in sorted(set(protos) & set(symbols)):
        ret, params = protos[name]
        res, args = symbols[name]
        if ret not in returns or returns[ret] is not res:
            faults.append(f"{name}: returns {ret!r}, bound as {res!r}")
        if len(params) != len(args):
            faults.append(f"{name}: {len(params)} parameters, bound with {len(args)}")
            continue
        for i, (typ, ct) in enumerate(zip(params, args)):
            w = [x for x in typ.split() if x != "const"]
            if w[-1] != "*":                                             # a scalar: exactly its type
                ok = len(w) == 1 and w[0] in scalar and ct is scalar[w[0]]
            elif w == ["gik_template", "*", "*"]:                        # the handle that create writes
                ok = ct is C.POINTER(C.c_void_p)
            elif w[0] in mirrors and w[0] != "gik_stats":                # a struct of the header: its mirror
                ok = w[1:] == ["*"] and ct is C.POINTER(mirrors[w[0]])
            elif w[0] in ("gik_template", "gik_stats", "void"):          # opaque handle, device array of records, stream
                ok = w[1:] == ["*"] and ct is C.c_void_p
            else:                                                        # an array of scalars, on the host or the device
                ok = w[1:] == ["*"] and w[0] in ("double", "float", "int32_t") and \
                    (ct is C.c_void_p or ct is C.POINTER({"double": C.c_double, "float": C.c_float, "int32_t": C.c_int32}[w[0]]))
            if not ok:
                faults.append(f"{name}: parameter {i} is {typ!r}, bound as {ct!r}")
    return faults


def test_prototypes_match_header():
    """Every gik_* prototype of the header against _ffi.SYMBOLS: the argument count, per argument a pointer (to the
    mirror of its struct where it has one) or exactly its scalar type, and the return type.  A pointer dropped from a
    long list would shift every later argument silently; the comparer is shown such a table and has to report it."""
    from graphik_amd import _ffi
    assert len(_header_prototypes()) == len(_ffi.SYMBOLS)
    assert _prototype_faults(_ffi.SYMBOLS) == []
    import ctypes as C
    res, args = _ffi.SYMBOLS["gik_anchored_retry_merge"]
    broken = list(args)
    broken.remove(C.c_void_p)
    faults = _prototype_faults(dict(_ffi.SYMBOLS, gik_anchored_retry_merge=(res, broken)))
    assert faults and all(f.startswith("gik_anchored_retry_merge:") for f in faults), faults


def test_struct_layouts_match_compiler(tmp_path):
    """sizeof and every offsetof of the eleven structs, as the host compiler lays the header out, against ctypes."""
    import ctypes as C
    import shutil
    import subprocess
    cc = next((c for c in ("cc", "gcc", "clang", "c++", "g++", "clang++") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host compiler (cc, gcc, clang, c++, g++, clang++) on this machine")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "graphik_amd.h"', "int main(void) {"]
    for cname, mirror in _mirrors().items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {field} %zu\\n", offsetof({cname}, {field}));' for field, _ in mirror._fields_]
    src = tmp_path / "layouts.c"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = str(tmp_path / "layouts")
    r = subprocess.run([cc, "-x", "c", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]      # (a field the header does not have fails here, by name)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in run.stdout.splitlines()}
    want = {}
    for cname, mirror in _mirrors().items():
        want[(cname, "sizeof")] = C.sizeof(mirror)
        want.update({(cname, field): getattr(mirror, field).offset for field, _ in mirror._fields_})
    assert got == want, sorted(set(got.items()) ^ set(want.items()))


def test_no_cpu_fallback_without_gpu():
    """Creating an engine object without a HIP device must fail loudly."""
    import torch
    from graphik_amd import _ffi
    from graphik_amd.engine import Template
    import numpy as np
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    om = np.zeros((4, 4))
    om[0, 1] = om[1, 0] = 1
    with pytest.raises(_ffi.GikError):
        Template.from_matrices(om, k=3, use_limits=False)


def test_product_does_not_import_oracle():
    """Nothing under graphik_amd/ may reference the CPU oracle."""
    pkg = os.path.join(REPO, "graphik_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(root, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and \
                    "gik_oracle" not in txt, f
