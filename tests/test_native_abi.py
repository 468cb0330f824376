"""The C-ABI library loads and exports every symbol include/tsfresh_amd.h declares; without a GPU it refuses to
compute instead of falling back to the CPU."""
import ctypes
import os
import re

import pytest

from tsfresh_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "tsfresh_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(tsfa_[a-z_0-9]+)\s*\(", _header())))


def _c_kind(c_type):
    """The kind of one C type of the header: a return type, or a parameter with its name stripped."""
    c_type = " ".join(c_type.replace("*", " * ").split())
    if c_type == "const char *":
        return "char_p"
    if "*" in c_type:
        return "ptr"
    return {"void": None, "int": "i32", "int32_t": "i32", "int64_t": "i64", "double": "f64", "size_t": "size_t"}[c_type]


def _declared_prototypes():
    """name -> (kind of the return value, [kind of every argument]) of `<return type> tsfa_name(<arguments>);`, in order."""
    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w \t]*?[\s*]+)(tsfa_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _header()):
        args = [] if args.strip() == "void" else [re.sub(r"\w+\s*$", "", a.strip()) for a in args.split(",")]
        assert name not in protos, name
        protos[name] = (_c_kind(ret), [_c_kind(a) for a in args])
    return protos


def _ctypes_kind(t):
    if t is None:
        return None
    if t is ctypes.c_size_t:
        return "size_t"
    if t is ctypes.c_char_p:
        return "char_p"
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "ptr"
    return {ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_double: "f64"}[t]


def _same_kind(c_kind, ctypes_kind):
    return c_kind == ctypes_kind or (c_kind == "char_p" and ctypes_kind == "ptr")   # a `const char *` may be bound either way


def _mismatches(declared, table):
    """Every function whose table entry differs from the header in arity, in the kind of an argument or of the return value."""
    bad = []
    for name, (ret, args) in declared.items():
        bound_ret, bound_args = table[name]
        if len(bound_args) != len(args):
            bad.append("%s: %d arguments bound, %d declared" % (name, len(bound_args), len(args)))
            continue
        if not _same_kind(ret, _ctypes_kind(bound_ret)):
            bad.append("%s: returns %s, bound as %s" % (name, ret, _ctypes_kind(bound_ret)))
        for i, (want, got) in enumerate(zip(args, map(_ctypes_kind, bound_args))):
            if not _same_kind(want, got):
                bad.append("%s: argument %d is %s, bound as %s" % (name, i, want, got))
    return bad


def test_prototype_table_agrees_with_the_header():
    """Needs neither the library nor a GPU: _native.PROTOTYPES against the declarations of include/tsfresh_amd.h."""
    declared = _declared_prototypes()
    assert set(declared) == set(_declared_symbols())   # the declaration pattern misses no function of the header
    assert list(_native.PROTOTYPES) == list(declared)  # the same functions, in the header's order
    assert _mismatches(declared, _native.PROTOTYPES) == []
    # the comparison can fail: one argument dropped, one int64_t bound as int32_t
    restype, argtypes = _native.PROTOTYPES["tsfa_roll_fill"]
    dropped = dict(_native.PROTOTYPES, tsfa_roll_fill=(restype, argtypes[:-1]))
    restype, argtypes = _native.PROTOTYPES["tsfa_pack_offsets"]
    assert argtypes[1] is ctypes.c_int64
    narrowed = dict(_native.PROTOTYPES, tsfa_pack_offsets=(restype, [argtypes[0], ctypes.c_int32, argtypes[2]]))
    assert _mismatches(declared, dropped) == ["tsfa_roll_fill: 14 arguments bound, 15 declared"]
    assert _mismatches(declared, narrowed) == ["tsfa_pack_offsets: argument 1 is i64, bound as i32"]


def test_library_exports_every_declared_symbol():
    lib = _native.load()
    declared = _declared_symbols()
    assert set(declared) == set(_native.EXPORTS), set(declared) ^ set(_native.EXPORTS)
    for sym in declared:
        assert getattr(lib, sym) is not None
    for name, (_, args) in _declared_prototypes().items():
        if args:
            assert getattr(lib, name).argtypes is not None, name


def test_version_and_registry():
    lib = _native.load()
    assert lib.tsfa_version() == 100
    from tsfresh_amd.feature_extraction.registry import CALCULATORS
    n = lib.tsfa_calc_count()
    names = {lib.tsfa_calc_name(i).decode() for i in range(n)}
    native = {k for k, c in CALCULATORS.items() if c.native}
    assert names == native, names ^ native
    for name in names:
        assert lib.tsfa_calc_name(lib.tsfa_calc_id(name.encode())).decode() == name
    assert lib.tsfa_calc_id(b"no_such_calculator") == -1


def test_no_gpu_means_error_not_cpu_fallback():
    if _native.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(_native.NativeError) as ei:
        _native.Plan([(_native.calc_id("mean"), (0, 0, 0, 0))])
    assert ei.value.code == _native.TSFA_ERR_NO_DEVICE
    assert "no CPU fallback" in str(ei.value)


def test_extract_features_fails_loudly_without_gpu():
    if _native.device_count() > 0:
        pytest.skip("a HIP device is present")
    import numpy as np
    import pandas as pd
    from tsfresh_amd import MinimalFCParameters, extract_features
    df = pd.DataFrame({"id": [1, 1, 2, 2], "t": [0, 1, 0, 1], "v": np.arange(4.0)})
    with pytest.raises(_native.NativeError):
        extract_features(df, column_id="id", column_sort="t", default_fc_parameters=MinimalFCParameters())
