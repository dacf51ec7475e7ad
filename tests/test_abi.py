"""The C-ABI library loads and exports every symbol include/pdmpc.h declares (no compute calls: no GPU here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from pdmpc import abi, backend, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "pdmpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pdmpc_[a-z_]+)\s*\(", text)))


def test_header_declares_the_documented_entry_points():
    names = declared_functions()
    for must in ("pdmpc_create", "pdmpc_upload_mpa", "pdmpc_plan_batch", "pdmpc_get_last_stats", "pdmpc_destroy"):
        assert must in names


def test_library_exports_every_declared_symbol():
    lib = backend.load_library()
    for name in declared_functions():
        assert hasattr(lib, name), "libpdmpc_hip.so does not export %s" % name
    assert sorted(backend.EXPORTS) == declared_functions()
    assert b"gfx950" in lib.pdmpc_version()


def test_struct_layouts_match_the_header():
    # sizes the C compiler produces for include/pdmpc.h (natural alignment, no packing)
    assert ctypes.sizeof(abi.Config) == 32
    assert ctypes.sizeof(abi.Maneuver) == 8 * 3 + 8 + 3 * 2 * abi.VMAX * 8
    assert ctypes.sizeof(abi.PolygonSet) == 32
    assert ctypes.sizeof(abi.VehicleOut) == abi.VEHICLE_OUT_DTYPE.itemsize
    assert abi.VEHICLE_OUT_DTYPE.fields["y_predicted"][1] % 8 == 0


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdmpc.h")).read(), flags=re.S)


def header_prototypes():
    """include/pdmpc.h -> {name: (return spelling, [argument spellings])}; a spelling is the type with the argument's name dropped."""

    def spelling(arg):
        arg = re.sub(r"\s*\b\w+$", "", arg.strip()) if not arg.strip().endswith("*") else arg.strip()
        return re.sub(r"\s*\*", "*", re.sub(r"\s+", " ", arg))

    out = {}
    for ret, name, args in re.findall(r"^((?:const )?\w+\*?) (pdmpc_[a-z_]+)\(([^)]*)\);", header_text(), flags=re.M):
        out[name] = (ret, [] if args.strip() == "void" else [spelling(a) for a in args.split(",")])
    return out


P = ctypes.POINTER
OPAQUE = ("pdmpc_handle", "pdmpc_group", "pdmpc_controller", "pdmpc_sweep")
STRUCTS = {"pdmpc_config": abi.Config, "pdmpc_maneuver": abi.Maneuver, "pdmpc_mpa": abi.Mpa, "pdmpc_polygon_set": abi.PolygonSet,
           "pdmpc_vehicle_in": abi.VehicleIn, "pdmpc_vehicle_out": abi.VehicleOut, "pdmpc_stats": abi.Stats, "pdmpc_choice": abi.ChoiceStruct,
           "pdmpc_launch_query": abi.LaunchQuery, "pdmpc_launch_plan": abi.LaunchPlan, "pdmpc_fca_group": abi.FcaGroup, "pdmpc_controller_config": abi.ControllerConfig, "pdmpc_scenario": abi.ScenarioStruct}
# the ctypes type of every C spelling the header uses for a return value or an argument
C_TYPES = {"int": ctypes.c_int, "const char*": ctypes.c_char_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "double": ctypes.c_double, "void*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "void**": P(ctypes.c_void_p), "size_t*": P(ctypes.c_size_t),
           "int64_t*": P(ctypes.c_int64), "uint64_t*": P(ctypes.c_uint64)}
for c, t in (("double", abi.c_double_p), ("int32_t", abi.c_int32_p), ("uint8_t", abi.c_uint8_p), ("uint32_t", abi.c_uint32_p)):
    C_TYPES.update({c + "*": t, "const %s*" % c: t, "const %s**" % c: P(t)})
for c in OPAQUE:
    C_TYPES.update({c + "*": ctypes.c_void_p, c + "**": P(ctypes.c_void_p), c + "* const*": P(ctypes.c_void_p)})
for c, t in STRUCTS.items():
    C_TYPES.update({c + "*": P(t), "const %s*" % c: P(t), "const %s**" % c: P(P(t))})


def test_prototype_table_matches_the_header():
    """Every prototype of include/pdmpc.h is in pdmpc.prototypes with the ctypes type of its return value and of every argument."""
    declared = header_prototypes()
    assert sorted(declared) == declared_functions() and len(declared) >= 130
    assert sorted(prototypes.PROTOTYPES) == sorted(declared)
    for name, (ret, args) in declared.items():
        restype, argtypes = prototypes.PROTOTYPES[name]
        assert ret in C_TYPES, "%s: unknown return spelling %r" % (name, ret)
        assert restype is C_TYPES[ret], "%s returns %s" % (name, ret)
        assert len(argtypes) == len(args), "%s takes %d arguments" % (name, len(args))
        for i, (spelled, t) in enumerate(zip(args, argtypes)):
            assert spelled in C_TYPES, "%s: unknown argument spelling %r" % (name, spelled)
            assert t is C_TYPES[spelled], "%s: argument %d is %s" % (name, i, spelled)


def test_every_call_is_declared_and_only_in_the_table():
    lib = backend.load_library()
    for name, (restype, argtypes) in prototypes.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and fn.restype is restype, name
    pkg = os.path.join(ROOT, "p-dmpc_amd", "pdmpc")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py") and f != "prototypes.py":
            text = open(os.path.join(pkg, f)).read()
            assert ".argtypes" not in text and ".restype" not in text, "%s declares a prototype of its own" % f


def header_structs():
    """include/pdmpc.h -> {struct name: [field names]} for every struct it defines."""
    out = {}
    for body, name in re.findall(r"typedef struct(?: \w+)? \{(.*?)\} (\w+);", header_text(), flags=re.S):
        out[name] = [re.match(r"[\s*]*(\w+)", piece).group(1) for decl in body.split(";") if decl.strip()
                     for piece in re.sub(r"^\s*(?:const )?\w+", "", decl, count=1).split(",")]
    return out


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof of every struct of include/pdmpc.h, from the compiler the library is built with (host only), against
    the ctypes twins of pdmpc.abi."""
    structs = header_structs()
    assert set(structs) == set(STRUCTS), "a struct of the header without a twin in pdmpc.abi (or the other way round)"
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "pdmpc.h"', "int main() {"]
    for name, fields in structs.items():
        lines.append('    std::printf("%s sizeof %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    std::printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines) + "\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    assert hipcc, "the compiler the library is built with is not there"
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    got = {}
    for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines():
        name, field, value = line.split()
        got.setdefault(name, {})[field] = int(value)
    for name, fields in structs.items():
        twin = STRUCTS[name]
        assert [f for f, _ in twin._fields_] == fields, name
        assert ctypes.sizeof(twin) == got[name]["sizeof"], name
        for f in fields:
            assert getattr(twin, f).offset == got[name][f], "%s.%s" % (name, f)


def test_no_device_fails_loudly_without_cpu_fallback():
    """On a box without a GPU the backend must refuse to work instead of silently computing on the CPU."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from pdmpc.config import Config

    with pytest.raises(backend.BackendError) as e:
        backend.Handle(Config(Hp=5))
    assert "no CPU fallback" in str(e.value) or "no HIP device" in str(e.value)


def test_product_code_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under p-dmpc_amd/ may import, link, load or call it."""
    pkg = os.path.join(ROOT, "p-dmpc_amd")
    forbidden = re.compile(r"(from\s+oracle|import\s+oracle|libpdmpc_oracle|oracle_[a-z_]+\s*\(|oracle/|pdmpc_oracle\.cpp)")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".m")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                m = forbidden.search(text)
                assert m is None, "%s references the oracle: %r" % (os.path.join(dirpath, f), m.group(0))


def test_two_independent_packers_agree():
    """The product's marshalling (pdmpc.abi) and the oracle's own (oracle/packing.py) were written separately from
    include/pdmpc.h.  Same struct sizes, and the oracle plans identically from either one's structs — a wrong index in one of
    them (polygon order of dynamic_obstacles, transition[k][i][j], area rows) would show here and in every GPU parity test."""
    import ctypes as C

    import numpy as np

    import problems
    from oracle import oracle, packing
    from pdmpc import abi

    assert C.sizeof(packing.OVehicleIn) == C.sizeof(abi.VehicleIn)
    assert C.sizeof(packing.OManeuver) == C.sizeof(abi.Maneuver)
    assert C.sizeof(packing.OMpa) == C.sizeof(abi.Mpa)
    assert C.sizeof(packing.OConfig) == C.sizeof(abi.Config)
    assert packing.OUT_DTYPE == abi.VEHICLE_OUT_DTYPE
    for mode, kw in (("interx", {"n_hdv": 1}), ("sat", {})):
        options, mpa, iters = problems.problem_set(mode, 3, 6, Hp=6, **kw)
        options.max_nodes = 1 << 20
        m1, k1 = abi.pack_mpa(mpa)
        v1, kv1 = abi.pack_vehicles(iters, options.Hp)
        m2, k2 = packing.pack_mpa(mpa)
        v2, kv2 = packing.pack_vehicles(iters, options.Hp)
        a, _, _ = oracle.plan_batch_raw(options, m1, v1, len(iters))
        b, _, _ = oracle.plan_batch_raw(options, m2, v2, len(iters))
        assert a.tobytes() == b.tobytes()
        assert (a["status"] == 0).any()
