"""ctypes binding of libtsfresh_amd.so (include/tsfresh_amd.h).

The library is built in-tree by `tsfresh_amd/csrc/Makefile` (or `__graft_entry__.build()`).  Loading fails loudly
when it is missing, and computing fails loudly when no HIP device is visible: there is no CPU fallback.
"""
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TSFA_LIB: diagnostics override (the phase-clock build of profiles/phase_ticks.py); the default is the in-tree library
LIB_PATH = os.environ.get("TSFA_LIB") or os.path.join(_HERE, "libtsfresh_amd.so")

TSFA_OK = 0
TSFA_ERR_INVALID = -1
TSFA_ERR_UNSUPPORTED = -2
TSFA_ERR_NO_DEVICE = -3
TSFA_ERR_HIP = -4
TSFA_ERR_TOO_LONG = -5
TSFA_F32, TSFA_F64, TSFA_I64, TSFA_I32 = 0, 1, 2, 3
TSFA_I8, TSFA_I16, TSFA_U8, TSFA_U16, TSFA_U32, TSFA_U64, TSFA_BOOL = 4, 5, 6, 7, 8, 9, 10
TSFA_F16, TSFA_BF16 = 11, 12   # tsfa_pack_dense only
TSFA_PACK_UNSORTED, TSFA_PACK_VALUE_NAN, TSFA_PACK_IN_ORDER = 1, 2, 4
TSFA_DENSE_BAD_LENGTH = 8
TSFA_DENSE_BAD_TIME = 16   # tsfa_pack_times
TSFA_DENSE_EMPTY_SERIES = 32   # tsfa_pack_dense_valid
TSFA_PACK_KEEP_SORT = 1
TSFA_HOST, TSFA_DEVICE = 0, 1
# enum tsfa_route: who evaluates the tail of a p-value cell (tsfa_relevance_tails_*)
(TSFA_ROUTE_NONE, TSFA_ROUTE_MWU_NORMAL, TSFA_ROUTE_FISHER, TSFA_ROUTE_KENDALL, TSFA_ROUTE_HOST_MWU_EXACT,
 TSFA_ROUTE_HOST_KS, TSFA_ROUTE_KS_EXACT) = range(7)
# enum tsfa_ks_tail: who evaluates the exact Kolmogorov-Smirnov tails (tsfa_relevance_tails_*_ks)
TSFA_KS_TAIL_HOST, TSFA_KS_TAIL_DEVICE = 0, 1



class FeatureSpec(ctypes.Structure):
    _fields_ = [("calc", ctypes.c_int32), ("reserved", ctypes.c_int32), ("p", ctypes.c_double * 4)]


class RelevanceCol(ctypes.Structure):
    _fields_ = [("n_unique", ctypes.c_int64), ("v_lo", ctypes.c_double), ("v_hi", ctypes.c_double),
                ("tie_term", ctypes.c_double)]


# the records of tsfa_relevance_col (above) and tsfa_relevance_real_col as numpy reads and writes them
_CLASS_COL_DTYPE = [("n_unique", "<i8"), ("v_lo", "<f8"), ("v_hi", "<f8"), ("tie_term", "<f8")]
_REAL_COL_DTYPE = [("n_unique", "<i8"), ("v_lo", "<f8"), ("v_hi", "<f8"), ("dis", "<i8"), ("xtie", "<i8"), ("ntie", "<i8"),
                   ("x0", "<f8"), ("x1", "<f8"), ("n_hi", "<i8"), ("ks_d", "<f8")]


class LaunchInfo(ctypes.Structure):
    """tsfa_launch_info: what one (kernel family, launch group) of the last extract launched (Plan.last_launches)."""
    _fields_ = [("family", ctypes.c_int32), ("length_class", ctypes.c_int32), ("max_len", ctypes.c_int32),
                ("threads", ctypes.c_int32), ("n_series", ctypes.c_int64), ("lds_bytes", ctypes.c_int64),
                ("long_build", ctypes.c_int32), ("variant", ctypes.c_int32)]


# enum tsfa_family (csrc/tsfa_specs.h), by number
FAMILY_NAMES = ("BASIC", "SORT", "SPECTRAL", "AR", "ENTROPY", "CWT", "SEQ", "TREND", "MPROFILE")


i32, i64, f64, ptr, size_t, char_p, P = (ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_char_p, ctypes.POINTER)

# name -> (return type, argument types) of every function include/tsfresh_amd.h declares, in the header's order: the ONE place a
# prototype is written (load() binds them all; tests/test_native_abi.py holds the table to the header).  Handles and buffers
# are `ptr` (they take a Python int, None or a ctypes object), out-parameters passed with byref are P(...).
PROTOTYPES = {
    "tsfa_version": (i32, []),
    "tsfa_device_count": (i32, []),
    "tsfa_last_error": (char_p, []),
    "tsfa_calc_id": (i32, [char_p]),
    "tsfa_calc_name": (char_p, [i32]),
    "tsfa_calc_count": (i32, []),
    "tsfa_plan_create": (i32, [P(FeatureSpec), i32, i32, P(ptr)]),
    "tsfa_plan_create_with_data": (i32, [P(FeatureSpec), i32, ptr, i64, i32, P(ptr)]),
    "tsfa_plan_n_cols": (i32, [ptr]),
    "tsfa_plan_destroy": (None, [ptr]),
    "tsfa_extract": (i32, [ptr, ptr, i32, ptr, i64, ptr, i64, i32, ptr]),
    "tsfa_extract_timed": (i32, [ptr, ptr, i32, ptr, ptr, i64, ptr, i64, i32, ptr]),
    "tsfa_extract_windows": (i32, [ptr, ptr, i32, ptr, ptr, ptr, i64, ptr, i64, i32, ptr]),
    "tsfa_extract_chunks": (i32, [ptr, i64, ptr, i32]),
    "tsfa_plan_set_profiling": (i32, [ptr, i32]),
    "tsfa_plan_last_timings": (i32, [ptr, P(char_p), P(ctypes.c_float), i32]),
    "tsfa_plan_last_launches": (i32, [ptr, P(LaunchInfo), i32]),
    "tsfa_plan_set_option": (i32, [ptr, char_p, f64]),
    "tsfa_plan_set_length_hint": (i32, [ptr, i64, i64]),
    "tsfa_pack_scan": (i32, [ptr, i32, ptr, i32, ptr, i32, i64, P(i32), P(i64)]),
    "tsfa_pack_offsets": (i32, [ptr, i64, i64]),
    "tsfa_pack_device": (i32, [ptr, i32, ptr, i32, ptr, i32, i64, i32, i32, i32, P(ptr)]),
    "tsfa_pack_device_n_rows": (i64, [ptr]),
    "tsfa_pack_device_n_groups": (i64, [ptr]),
    "tsfa_pack_device_flags": (i32, [ptr]),
    "tsfa_pack_device_n_passes": (i32, [ptr]),
    "tsfa_pack_device_values": (i32, [ptr, P(ptr), P(i32)]),
    "tsfa_pack_device_offsets": (ptr, [ptr]),
    "tsfa_pack_device_ids": (ptr, [ptr]),
    "tsfa_pack_device_copy_ids": (i32, [ptr, ptr]),
    "tsfa_pack_device_copy_offsets": (i32, [ptr, ptr]),
    "tsfa_pack_device_copy_sort": (i32, [ptr, ptr]),
    "tsfa_pack_device_destroy": (None, [ptr]),
    "tsfa_pack_set_create": (i32, [ptr, i32, ptr, i32, ptr, i32, i64, i32, i32, i32, P(ptr)]),
    "tsfa_pack_set_n_kinds": (i32, [ptr]),
    "tsfa_pack_set_copy_kinds": (i32, [ptr, ptr]),
    "tsfa_pack_set_flags": (i32, [ptr]),
    "tsfa_pack_set_n_passes": (i32, [ptr]),
    "tsfa_pack_set_values": (i32, [ptr, ptr, i32, i32, P(ptr)]),
    "tsfa_pack_set_rows": (i32, [ptr, ptr, i32, i64, i64, i64, P(ptr)]),
    "tsfa_pack_set_hours": (i32, [ptr, ptr, i32, i64, i64, ptr, ptr]),
    "tsfa_pack_set_destroy": (None, [ptr]),
    "tsfa_pack_dense": (i32, [ptr, i32, i64, i64, i64, i64, i64, i64, ptr, i32, ptr, i64, ptr, ptr, i32, ptr]),
    "tsfa_pack_times": (i32, [ptr, i32, i64, i64, i64, i64, i64, ptr, ptr, ptr, i32, ptr]),
    "tsfa_pack_dense_valid": (i32, [ptr, i32, i64, i64, i64, i64, i64, i64, ptr, i32, ptr, i32, i64, i64, ptr, i64, ptr, ptr, ptr,
                                    ptr, i64, ptr, i32, ptr]),
    "tsfa_roll_windows": (i32, [ptr, i32, i64, i64, i64, P(ptr)]),
    "tsfa_windows_n_windows": (i64, [ptr]),
    "tsfa_windows_starts": (ptr, [ptr]),
    "tsfa_windows_ends": (ptr, [ptr]),
    "tsfa_windows_copy_series": (i32, [ptr, ptr]),
    "tsfa_windows_copy_timeshifts": (i32, [ptr, ptr]),
    "tsfa_windows_copy_starts": (i32, [ptr, ptr]),
    "tsfa_windows_copy_ends": (i32, [ptr, ptr]),
    "tsfa_roll_shift_values": (i32, [ptr, ptr, ptr]),
    "tsfa_windows_destroy": (None, [ptr]),
    "tsfa_roll_count": (i32, [ptr, i64, i64, i32, i64, i64, i64, ptr, P(i64), i32, ptr]),
    "tsfa_roll_fill": (i32, [ptr, i64, ptr, i64, i64, i32, i64, i64, i64, ptr, ptr, ptr, ptr, i32, ptr]),
    "tsfa_host_alloc": (i32, [P(ptr), size_t]),
    "tsfa_host_free": (i32, [ptr]),
    "tsfa_device_alloc": (i32, [P(ptr), size_t, i32]),
    "tsfa_device_free": (i32, [ptr, i32]),
    "tsfa_device_copy": (i32, [ptr, ptr, size_t, i32, i32]),
    "tsfa_gather_columns": (i32, [ptr, i64, i64, ptr, i64, ptr, i32]),
    "tsfa_scatter_columns": (i32, [ptr, i64, ptr, ptr, i64, i64, i32]),
    "tsfa_relevance_classes": (i32, [ptr, i64, i64, i64, i32, ptr, i32, i32, ptr, ptr, ptr]),
    "tsfa_relevance_classes_ks": (i32, [ptr, i64, i64, i64, i32, ptr, i32, i32, ptr, ptr, ptr, ptr]),
    "tsfa_relevance_real": (i32, [ptr, i64, i64, i64, i32, ptr, ptr, ptr, i32, ptr]),
    "tsfa_ks_outer_prob": (f64, [i64, i64, i64, i64]),
    "tsfa_impute": (i32, [ptr, i64, i64, i64, i32, i32, ptr, ptr, ptr, ptr]),
    "tsfa_relevance_tails_classes": (i32, [ptr, i64, i64, i64, i32, ptr, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, P(i64)]),
    "tsfa_relevance_tails_real": (i32, [ptr, i64, i64, i64, i32, ptr, ptr, ptr, i64, f64, f64, i32, ptr, ptr, ptr, ptr, P(i64)]),
    "tsfa_ks_tails": (i32, [ptr, ptr, ptr, i64, i32, ptr, ptr]),
    "tsfa_relevance_tails_classes_ks": (i32, [ptr, i64, i64, i64, i32, ptr, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr,
                                              ptr, P(i64)]),
    "tsfa_relevance_tails_real_ks": (i32, [ptr, i64, i64, i64, i32, ptr, ptr, ptr, i64, f64, f64, i32, i32, ptr, ptr, ptr, ptr,
                                           ptr, ptr, P(i64)]),
    "tsfa_relevance_fdr": (i32, [ptr, ptr, i64, i32, f64, f64, i32, i32, i32, ptr, ptr, ptr, ptr]),
    "tsfa_compact_mask": (i32, [ptr, i64, ptr, P(i64), i32]),
    "tsfa_gather_columns_device": (i32, [ptr, i64, i64, ptr, i64, ptr, i64, i32]),
}
# every symbol include/tsfresh_amd.h declares
EXPORTS = tuple(PROTOTYPES)


class NativeError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("tsfresh_amd native error {}: {}".format(code, message))
        self.code = code


_lib = None


def load():
    """Load (once) and return the ctypes handle; raises ImportError if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "{} is missing: build it with `make -C tsfresh_amd/csrc` (hipcc --offload-arch=gfx950). "
            "tsfresh_amd has no CPU fallback.".format(LIB_PATH))
    lib = ctypes.CDLL(LIB_PATH)
    # A symbol the library lacks is skipped: an older build given through TSFA_LIB may predate it, and using it then raises
    # AttributeError with the symbol's name.  (The in-tree library is held to every symbol by tests/test_native_abi.py.)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _check(lib, rc):
    if rc != TSFA_OK:
        raise NativeError(rc, lib.tsfa_last_error().decode("utf-8", "replace"))


class _Owner:
    """Owns the library handle `_h` (made through `_lib`) until `close()`, which hands it to the function named `_destroy`."""

    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        # at interpreter exit the HIP runtime may already be gone: leak rather than call into it
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass


def set_library_option(name, value):
    """Library-wide option (tsfa_plan_set_option with a NULL plan), e.g. "relevance_batch"."""
    lib = load()
    _check(lib, lib.tsfa_plan_set_option(None, name.encode("ascii"), float(value)))


def device_count():
    return int(load().tsfa_device_count())


def calc_id(name):
    return int(load().tsfa_calc_id(name.encode("ascii")))


# Page-locking memory is slow (~0.1 ms per MB), so freed blocks are kept for reuse, by power-of-two size class, up to
# TSFRESH_AMD_PINNED_POOL_MB (default 4096) in total; a result matrix handed to the caller returns here when the
# caller's DataFrame dies.
_PIN_POOL = {}
_PIN_POOL_BYTES = [0]
_PIN_LOCK = __import__("threading").RLock()   # re-entrant: a cyclic GC pass under the lock may finalize another _PinnedBlock


def _pin_pool_cap():
    return int(os.environ.get("TSFRESH_AMD_PINNED_POOL_MB", "4096")) << 20


class _PinnedBlock:
    """Owner of one tsfa_host_alloc allocation; numpy arrays built on it keep it alive through their base chain."""

    def __init__(self, nbytes):
        lib = load()
        size = 1 << max(20, int(nbytes - 1).bit_length()) if nbytes > (1 << 20) else (1 << 20)
        with _PIN_LOCK:
            free = _PIN_POOL.get(size)
            ptr = free.pop() if free else None
            if ptr is not None:
                _PIN_POOL_BYTES[0] -= size
        if ptr is None:
            p = ctypes.c_void_p()
            _check(lib, lib.tsfa_host_alloc(ctypes.byref(p), size))
            ptr = p.value
        self._lib, self.ptr, self.nbytes, self.size = lib, ptr, int(nbytes), size

    def __del__(self):
        try:
            ptr, self.ptr = getattr(self, "ptr", None), None
            if not ptr:
                return
            with _PIN_LOCK:
                if _PIN_POOL_BYTES[0] + self.size <= _pin_pool_cap():
                    _PIN_POOL.setdefault(self.size, []).append(ptr)
                    _PIN_POOL_BYTES[0] += self.size
                    return
            self._lib.tsfa_host_free(ptr)
        except Exception:  # interpreter shutdown
            pass


def release_pinned_pool():
    """Give the pooled page-locked blocks back to the system."""
    lib = load()
    with _PIN_LOCK:
        for size, ptrs in _PIN_POOL.items():
            for ptr in ptrs:
                lib.tsfa_host_free(ptr)
        _PIN_POOL.clear()
        _PIN_POOL_BYTES[0] = 0


def pinned_empty(shape, dtype):
    """np.empty(shape, dtype) in page-locked host memory (tsfa_host_alloc): the copy engines reach it directly, so the
    chunked H2D / kernels / D2H pipeline of tsfa_extract(TSFA_HOST) runs at PCIe rate.  Returned to the pool with the
    last view."""
    dtype = np.dtype(dtype)
    shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    block = _PinnedBlock(n * dtype.itemsize)
    buf = (ctypes.c_char * max(block.nbytes, 1)).from_address(block.ptr)
    buf._tsfa_owner = block  # array -> memoryview -> buf -> block: the allocation lives as long as any view of it
    return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)


_PACK_TYPES = {np.dtype(np.float32): TSFA_F32, np.dtype(np.float64): TSFA_F64, np.dtype(np.int64): TSFA_I64,
               np.dtype(np.int32): TSFA_I32}


def pack_scan(ids, sort_values, values):
    """One multi-threaded pass over the rows of a long frame (tsfa_pack_scan): -> (flags, offsets or None).
    Returns None when a column has a layout / element type the native scan does not take (the caller uses numpy)."""
    cols = []
    for a in (ids, sort_values, values):
        if a is None:
            cols.append((None, 0))
            continue
        if isinstance(a, np.ndarray) and a.dtype.kind in "mM" and a.dtype.itemsize == 8:
            a = a.view(np.int64)  # datetime64 / timedelta64 sort keys compare like their integer ticks (no NaT: checked)
        if not isinstance(a, np.ndarray) or a.ndim != 1 or not a.flags.c_contiguous or a.dtype not in _PACK_TYPES:
            return None
        cols.append((a.ctypes.data, _PACK_TYPES[a.dtype]))   # (a view shares the caller's memory)
    lib = load()
    flags, groups = ctypes.c_int32(0), ctypes.c_int64(0)
    n = len(ids)
    _check(lib, lib.tsfa_pack_scan(cols[0][0], cols[0][1], cols[1][0], cols[1][1], cols[2][0], cols[2][1], n,
                                   ctypes.byref(flags), ctypes.byref(groups)))
    if flags.value & TSFA_PACK_UNSORTED:
        return flags.value, None
    offsets = np.empty(groups.value + 1, dtype=np.int64)
    _check(lib, lib.tsfa_pack_offsets(offsets.ctypes.data, groups.value, n))
    return flags.value, offsets


# element types tsfa_pack_device takes (ids: the integer ones; sort keys: those and the two float types; values: all)
_DEVICE_PACK_TYPES = {np.dtype(np.float32): TSFA_F32, np.dtype(np.float64): TSFA_F64, np.dtype(np.int64): TSFA_I64,
                      np.dtype(np.int32): TSFA_I32, np.dtype(np.int8): TSFA_I8, np.dtype(np.int16): TSFA_I16,
                      np.dtype(np.uint8): TSFA_U8, np.dtype(np.uint16): TSFA_U16, np.dtype(np.uint32): TSFA_U32,
                      np.dtype(np.uint64): TSFA_U64, np.dtype(np.bool_): TSFA_BOOL}


def pack_column(a):
    """A column as tsfa_pack_device reads it: -> (C-contiguous 1-D ndarray, tsfa_dtype code), or None for an element type /
    shape the device packer does not take.  datetime64 / timedelta64 are viewed as their int64 ticks (they compare alike);
    a strided column (one column of a DataFrame block) is copied once."""
    if not isinstance(a, np.ndarray) or a.ndim != 1:
        return None
    if a.dtype.kind in "mM" and a.dtype.itemsize == 8:
        a = a.view(np.int64)
    if not a.dtype.isnative:
        return None
    code = _DEVICE_PACK_TYPES.get(a.dtype)
    if code is None:
        return None
    return np.ascontiguousarray(a), code


class DevicePack(_Owner):
    """Owns a `tsfa_pack*`: one kind of a frame in ANY row order, grouped by id and ordered by the sort column on the device
    (tsfa_pack_device).  The ragged sample buffer and the offsets stay in HBM and go to `Plan.extract_pack` / the
    `pack=` form of `extract_into` as device pointers; only the unique ids (`.ids`) come back at once, `.offsets`, `.sort`
    and `.values_host()` when asked for.  ids / sort / values: what `pack_column` returned (sort may be None)."""

    _destroy = "tsfa_pack_device_destroy"

    def __init__(self, ids, sort, values, device=0, keep_sort=False):
        lib = load()
        (ids_a, ids_t), (val_a, val_t) = ids, values
        sort_a, sort_t = sort if sort is not None else (None, 0)
        if len(val_a) != len(ids_a) or (sort_a is not None and len(sort_a) != len(ids_a)):
            raise ValueError("the id, sort and value columns must have one entry per row")
        handle = ctypes.c_void_p()
        _check(lib, lib.tsfa_pack_device(
            ids_a.ctypes.data, ids_t, None if sort_a is None else sort_a.ctypes.data, sort_t, val_a.ctypes.data, val_t,
            len(ids_a), TSFA_HOST, TSFA_PACK_KEEP_SORT if (keep_sort and sort_a is not None) else 0, int(device),
            ctypes.byref(handle)))
        self._adopt(lib, handle, device, ids_a.dtype, None if sort_a is None or not keep_sort else sort_a.dtype)

    def _adopt(self, lib, handle, device, ids_dtype, sort_dtype, copy_ids=True):
        """Take over a `tsfa_pack*` (one made by tsfa_pack_device, or a view handed out by a DevicePackSet).
        copy_ids=False (the device-pointer path): `.ids` stays None, the ids stay in HBM at `.ids_ptr`."""
        self._lib, self._h, self.device = lib, handle, int(device)
        self.n_rows = int(lib.tsfa_pack_device_n_rows(handle))
        self.n_series = int(lib.tsfa_pack_device_n_groups(handle))
        self.flags = int(lib.tsfa_pack_device_flags(handle))
        self.n_passes = int(lib.tsfa_pack_device_n_passes(handle))
        vptr, vtype = ctypes.c_void_p(), ctypes.c_int32()
        _check(lib, lib.tsfa_pack_device_values(handle, ctypes.byref(vptr), ctypes.byref(vtype)))
        self.values_ptr, self.values_type = vptr.value, int(vtype.value)
        self.values_dtype = np.dtype(np.float32 if self.values_type == TSFA_F32 else np.float64)
        self.offsets_ptr = lib.tsfa_pack_device_offsets(handle)
        self._sort_dtype = sort_dtype
        self._offsets = self._sort = None
        self.ids_dtype = np.dtype(ids_dtype)
        self.ids = None
        if copy_ids:
            self.ids = np.empty(self.n_series, dtype=ids_dtype)
            _check(lib, lib.tsfa_pack_device_copy_ids(handle, self.ids.ctypes.data))

    @property
    def ids_ptr(self):
        """Device pointer (int) of the n_series unique ids, ascending, in the id column's own dtype (tsfa_pack_device_ids)."""
        return self._lib.tsfa_pack_device_ids(self._h)

    @property
    def value_nan(self):
        return bool(self.flags & TSFA_PACK_VALUE_NAN)

    @property
    def was_in_order(self):
        return bool(self.flags & TSFA_PACK_IN_ORDER)

    @property
    def offsets(self):
        if self._offsets is None:
            out = np.empty(self.n_series + 1, dtype=np.int64)
            _check(self._lib, self._lib.tsfa_pack_device_copy_offsets(self._h, out.ctypes.data))
            self._offsets = out
        return self._offsets

    @property
    def sort(self):
        """The sort column in packed order (None unless the pack was made with keep_sort=True)."""
        if self._sort is None and self._sort_dtype is not None:
            out = np.empty(self.n_rows, dtype=self._sort_dtype)
            _check(self._lib, self._lib.tsfa_pack_device_copy_sort(self._h, out.ctypes.data))
            self._sort = out
        return self._sort

    def values_host(self):
        """A host copy of the ragged sample buffer (tsfa_device_copy)."""
        out = np.empty(self.n_rows, dtype=self.values_dtype)
        _check(self._lib, self._lib.tsfa_device_copy(out.ctypes.data, self.values_ptr, out.nbytes, 0, self.device))
        return out


class DevicePackSet(_Owner):
    """Owns a `tsfa_pack_set*`: a frame of several kinds in ANY row order, sorted ONCE by (kind, id, sort) on the device
    (tsfa_pack_set_create).  `values(column)` gathers one value column through the stored permutation and returns one
    DevicePack per kind, in ascending order of the kind values (`.kinds`): views into one gathered buffer that share the
    set's offsets and ids.  The views and the set may be closed in any order; a buffer goes with its last holder.
    ids / sort / kinds: what `pack_column` returned; sort may be None, kinds may be None (one kind: a wide frame, one
    `values` call per value column, or one `rows` call for a value matrix).
    space=TSFA_DEVICE (with n_rows): the columns are already in HBM on `device`, each given as (device pointer (int),
    tsfa_dtype code, numpy dtype) of a contiguous column; they are used in place, nothing is staged, the views keep their
    ids in HBM (`DevicePack.ids_ptr`, `.ids` is None) and `values` / `rows` / `hours` take device pointers."""

    _destroy = "tsfa_pack_set_destroy"

    def __init__(self, ids, sort, kinds, device=0, keep_sort=False, space=TSFA_HOST, n_rows=None):
        lib = load()
        # either form of the three key columns -> (pointer or None, tsfa_dtype code, numpy dtype) each
        if space == TSFA_DEVICE:
            cols = [c if c is not None and c[0] else (None, 0, None) for c in (ids, sort, kinds)]
            if n_rows is None:
                raise ValueError("space=TSFA_DEVICE needs n_rows")
        else:
            cols = [(None, 0, None) if c is None else (c[0].ctypes.data, c[1], c[0].dtype) for c in (ids, sort, kinds)]
            space, n_rows = TSFA_HOST, len(ids[0])
            if any(c is not None and len(c[0]) != n_rows for c in (sort, kinds)):
                raise ValueError("the id, sort and kind columns must have one entry per row")
        (ids_p, ids_t, ids_dtype), (sort_p, sort_t, sort_dtype), (kind_p, kind_t, kind_dtype) = cols
        keep_sort = bool(keep_sort) and sort_p is not None
        handle = ctypes.c_void_p()
        _check(lib, lib.tsfa_pack_set_create(ids_p, int(ids_t), sort_p, int(sort_t), kind_p, int(kind_t), int(n_rows), int(space),
                                             TSFA_PACK_KEEP_SORT if keep_sort else 0, int(device), ctypes.byref(handle)))
        self.space = int(space)
        self._lib, self._h, self.device = lib, handle, int(device)
        self.n_rows = int(n_rows)
        self.n_kinds = int(lib.tsfa_pack_set_n_kinds(handle))
        self.flags = int(lib.tsfa_pack_set_flags(handle))
        self.n_passes = int(lib.tsfa_pack_set_n_passes(handle))
        self._ids_dtype = np.dtype(ids_dtype)
        self._sort_dtype = np.dtype(sort_dtype) if keep_sort else None
        self.kinds = None
        if kind_p is not None:
            self.kinds = np.empty(self.n_kinds, dtype=kind_dtype)   # (the library's host copy: nothing crosses the bus here)
            _check(lib, lib.tsfa_pack_set_copy_kinds(handle, self.kinds.ctypes.data))

    @property
    def was_in_order(self):
        return bool(self.flags & TSFA_PACK_IN_ORDER)

    def _views(self, handles):
        packs = []
        for h in handles:
            pack = DevicePack.__new__(DevicePack)   # a view: no tsfa_pack_device call
            packs.append(pack)
            pack._adopt(self._lib, h, self.device, self._ids_dtype, self._sort_dtype, copy_ids=self.space == TSFA_HOST)
        return packs

    def values(self, column):
        """column: what `pack_column` returned for a value column of n_rows entries -- for a set made with
        space=TSFA_DEVICE (device pointer (int), tsfa_dtype code) of a contiguous column -> [DevicePack per kind]."""
        if not self._h:
            raise ValueError("the pack set is closed")
        handles = (ctypes.c_void_p * self.n_kinds)()
        if self.space == TSFA_DEVICE:
            val_p, val_t = column
            _check(self._lib, self._lib.tsfa_pack_set_values(self._h, val_p, int(val_t), TSFA_DEVICE, handles))
            return self._views(handles)
        val_a, val_t = column
        if len(val_a) != self.n_rows:
            raise ValueError("the value column must have one entry per row")
        _check(self._lib, self._lib.tsfa_pack_set_values(self._h, val_a.ctypes.data, val_t, TSFA_HOST, handles))
        return self._views(handles)

    def rows(self, values_ptr, value_type, n_cols, stride_row, stride_col):
        """tsfa_pack_set_rows: the (n_rows, n_cols) value matrix at the device pointer `values_ptr` (element strides
        stride_row / stride_col) through the permutation in one pass -> [DevicePack per column], views into one buffer
        that share the set's offsets and ids.  Only for a set without a kind column."""
        if not self._h:
            raise ValueError("the pack set is closed")
        handles = (ctypes.c_void_p * int(n_cols))()
        _check(self._lib, self._lib.tsfa_pack_set_rows(self._h, values_ptr, int(value_type), int(n_cols), int(stride_row),
                                                       int(stride_col), handles))
        return self._views(handles)

    def hours(self, t_ptr, t_type, ticks_per_second, stride, hours_ptr, flags_ptr):
        """tsfa_pack_set_hours on raw device pointers (ints): the n_rows row-aligned stamps at t_ptr (TSFA_I64 ticks or
        TSFA_F64 seconds, element stride `stride`) -> float64 hours since the first stamp of each (kind, id) group at
        hours_ptr, in the set's sorted order over all kinds; flags_ptr: one int32 the call ORs TSFA_DENSE_BAD_TIME into."""
        if not self._h:
            raise ValueError("the pack set is closed")
        _check(self._lib, self._lib.tsfa_pack_set_hours(self._h, t_ptr, int(t_type), int(ticks_per_second), int(stride),
                                                        hours_ptr, flags_ptr))


def pack_dense(x_ptr, x_type, shape, strides, values_ptr, channel_stride_out, offsets_ptr, flags_ptr, device=0,
               lengths_ptr=None, lengths_type=0, stream=None):
    """tsfa_pack_dense on raw device pointers (ints): the array of logical `shape` (n_batch, n_channels, n_time) and element
    `strides` at x_ptr -> the ragged layout in caller-provided buffers: channel c at values_ptr + c * channel_stride_out
    elements (float64 for TSFA_F64 input, float32 otherwise), n_batch + 1 int64 offsets shared by the channels, one int32
    flag word the call ORs into.  lengths_ptr: n_batch int32 / int64 (lengths_type TSFA_I32 / TSFA_I64) or None.
    stream: a hipStream_t as an int (the call only enqueues) or None (the call returns when the work is done)."""
    lib = load()
    (n_batch, n_channels, n_time), (sb, sc, st) = shape, strides
    _check(lib, lib.tsfa_pack_dense(
        x_ptr, int(x_type), int(n_batch), int(n_channels), int(n_time), int(sb), int(sc), int(st), lengths_ptr or None,
        int(lengths_type), values_ptr, int(channel_stride_out), offsets_ptr, flags_ptr, int(device), stream or None))


def pack_times(t_ptr, t_type, ticks_per_second, shape, strides, offsets_ptr, hours_ptr, flags_ptr, device=0, stream=None):
    """tsfa_pack_times on raw device pointers (ints): the stamps of logical `shape` (n_batch, n_time) and element `strides`
    at t_ptr -- TSFA_I64 ticks, ticks_per_second of them per second, or TSFA_F64 seconds -- become float64 hours since each
    series' first stamp at hours_ptr, in the ragged layout of the n_batch + 1 int64 offsets `pack_dense` wrote at
    offsets_ptr.  flags_ptr: one int32 the call ORs TSFA_DENSE_BAD_TIME into (a NaT / NaN stamp inside a length).
    stream: a hipStream_t as an int (the call only enqueues) or None (the call returns when the work is done)."""
    lib = load()
    (n_batch, n_time), (sb, st) = shape, strides
    _check(lib, lib.tsfa_pack_times(t_ptr, int(t_type), int(ticks_per_second), int(n_batch), int(n_time), int(sb), int(st),
                                    offsets_ptr, hours_ptr, flags_ptr, int(device), stream or None))


def pack_dense_valid_scratch_bytes(n_batch, n_time):
    """The scratch tsfa_pack_dense_valid asks for: 200 bytes per work item of 1024 steps of one series."""
    return 200 * int(n_batch) * ((int(n_time) + 1023) // 1024)


def pack_dense_valid(x_ptr, x_type, shape, strides, values_ptr, channel_stride_out, offsets_ptr, steps_ptr, scratch_ptr,
                     scratch_bytes, flags_ptr, device=0, lengths_ptr=None, lengths_type=0, t_ptr=None, t_type=0,
                     t_strides=(0, 0), stamps_ptr=None, stream=None):
    """tsfa_pack_dense_valid on raw device pointers (ints): `pack_dense` without the steps a wide frame loses to dropna() -- a
    step of a series goes, for every channel, when any channel's sample is NaN or (with t_ptr: int64 ticks or float64
    seconds of logical shape (n_batch, n_time) and element strides t_strides) its stamp is NaT / NaN.  offsets_ptr receives
    the exclusive scan of the kept counts, steps_ptr (int32, n_batch * n_time cells) the original step index of every kept
    sample, stamps_ptr (with t_ptr: n_batch * n_time elements) the kept stamps as a right-padded (n_batch, n_time) array
    for `pack_times`.  scratch_ptr: `pack_dense_valid_scratch_bytes` of device memory.  flags_ptr: one int32 the call ORs
    TSFA_DENSE_BAD_LENGTH and TSFA_DENSE_EMPTY_SERIES into.  stream: a hipStream_t as an int (the call only enqueues) or
    None (the call returns when the work is done)."""
    lib = load()
    (n_batch, n_channels, n_time), (sb, sc, st), (tsb, tst) = shape, strides, t_strides
    _check(lib, lib.tsfa_pack_dense_valid(
        x_ptr, int(x_type), int(n_batch), int(n_channels), int(n_time), int(sb), int(sc), int(st), lengths_ptr or None,
        int(lengths_type), t_ptr or None, int(t_type), int(tsb), int(tst), values_ptr, int(channel_stride_out), offsets_ptr,
        steps_ptr, stamps_ptr or None, scratch_ptr, int(scratch_bytes), flags_ptr, int(device), stream or None))


class DensePack:
    """One channel of a tsfa_pack_dense result, as `Plan.extract_into(pack=...)` and `extract_parts_into(pack=...)` read a
    pack: the channel's stretch of the value buffer, the offsets every channel shares, the series count.  A view: the
    buffers belong to `owner` (whatever must stay alive while the view is used), nothing is freed here."""

    def __init__(self, values_ptr, values_type, offsets_ptr, n_series, device, owner=None):
        self.values_ptr, self.values_type = int(values_ptr), int(values_type)
        self.offsets_ptr, self.n_series, self.device = int(offsets_ptr), int(n_series), int(device)
        self.values_dtype = np.dtype(np.float32 if self.values_type == TSFA_F32 else np.float64)
        self.owner = owner

    def close(self):
        self.owner = None


class BorrowedMatrix:
    """Row-major float64 [n_rows, >= n_cols] device memory someone else owns (a torch tensor), with the attributes the
    extract paths read of a DeviceMatrix: `.ptr`, `.ld`, `.shape`, `.device`.  Frees nothing; `owner` keeps the memory's
    owner alive for as long as the wrapper lives."""

    def __init__(self, ptr, n_rows, n_cols, device, ld=None, owner=None):
        self.ptr, self.shape, self.device = int(ptr), (int(n_rows), int(n_cols)), int(device)
        self.ld = int(n_cols if ld is None else ld)
        if self.ld < self.shape[1]:
            raise ValueError("the leading dimension is below the number of columns")
        self.owner = owner


def roll_count(offsets_ptr, n_series, rolling_direction=1, max_timeshift=None, min_timeshift=0, steps=1, scanned_ptr=None,
               series_len=0, device=0, stream=None):
    """tsfa_roll_count on raw device pointers (ints) -> the number of windows of the batch whose n_series + 1 int64 offsets
    lie at offsets_ptr.  scanned_ptr: n_series uint32 of the caller's (a ragged batch: they receive the exclusive scan of the
    per-series counts, which `roll_fill` reads; the call waits for its stream), or None for a uniform batch of series_len
    samples per series (the closed form: nothing is launched or read back, offsets_ptr may be None)."""
    lib = load()
    total = ctypes.c_int64(0)
    _check(lib, lib.tsfa_roll_count(offsets_ptr or None, int(n_series), int(series_len), int(rolling_direction),
                                    int(max_timeshift or 0), int(min_timeshift), int(steps), scanned_ptr or None,
                                    ctypes.byref(total), int(device), stream or None))
    return int(total.value)


def roll_fill(offsets_ptr, n_series, n_windows, starts_ptr, ends_ptr, series_ptr, timeshifts_ptr, rolling_direction=1,
              max_timeshift=None, min_timeshift=0, steps=1, scanned_ptr=None, series_len=0, device=0, stream=None):
    """tsfa_roll_fill on raw device pointers (ints): the n_windows windows `roll_count` counted for the same arguments, as
    four int64 arrays of the caller's -- starts / ends (indices into a channel's value buffer), series, timeshifts -- in
    (series, ascending timeshift) order.  stream: a hipStream_t as an int (the call only enqueues) or None (the call
    returns when the work is done)."""
    lib = load()
    _check(lib, lib.tsfa_roll_fill(offsets_ptr or None, int(n_series), scanned_ptr or None, int(series_len), int(n_windows),
                                   int(rolling_direction), int(max_timeshift or 0), int(min_timeshift), int(steps),
                                   starts_ptr or None, ends_ptr or None, series_ptr or None, timeshifts_ptr or None, int(device),
                                   stream or None))


class DeviceWindows(_Owner):
    """Owns a `tsfa_windows*`: the rolled windows of one DevicePack, built on the device from the pack's offsets
    (tsfa_roll_windows).  The starts and ends stay in HBM and go to `Plan.extract_windows_pack` as device pointers; the host
    gets the series index and the timeshift of every window (`.series`, `.timeshifts`: what the window ids are built from),
    `.shift_values()` (the kept sort column's value that names each window) and, only when asked, `.starts` / `.ends`.
    steps: the reference's prediction_steps -- the longest series of the whole frame, which another kind may own.
    The pack must stay open for as long as the windows are used."""

    _destroy = "tsfa_windows_destroy"

    def __init__(self, pack, rolling_direction=1, max_timeshift=None, min_timeshift=0, steps=None):
        lib = load()
        if steps is None:
            steps = int(np.diff(pack.offsets).max()) if pack.n_series else 1
        handle = ctypes.c_void_p()
        _check(lib, lib.tsfa_roll_windows(pack._h, int(rolling_direction), int(max_timeshift or 0), int(min_timeshift),
                                          int(steps), ctypes.byref(handle)))
        self._lib, self._h, self._pack, self.device = lib, handle, pack, pack.device
        self.rolling_direction = int(rolling_direction)
        self.n_windows = int(lib.tsfa_windows_n_windows(handle))
        self.starts_ptr = lib.tsfa_windows_starts(handle)
        self.ends_ptr = lib.tsfa_windows_ends(handle)
        self._host = {}

    def _copy(self, what):
        if what not in self._host:
            out = np.empty(self.n_windows, dtype=np.int64)
            fn = getattr(self._lib, "tsfa_windows_copy_" + what)
            _check(self._lib, fn(self._h, out.ctypes.data))
            self._host[what] = out
        return self._host[what]

    @property
    def series(self):
        return self._copy("series")

    @property
    def timeshifts(self):
        return self._copy("timeshifts")

    @property
    def starts(self):
        return self._copy("starts")

    @property
    def ends(self):
        return self._copy("ends")

    def shift_values(self):
        """sort[ends - 1] (positive direction) / sort[starts] (negative) of the pack's kept sort column, gathered on the
        device: n_windows elements of the column's dtype come back, not the column."""
        if self._pack._sort_dtype is None:
            raise ValueError("the pack was made without keep_sort=True: it holds no sort column")
        out = np.empty(self.n_windows, dtype=self._pack._sort_dtype)
        _check(self._lib, self._lib.tsfa_roll_shift_values(self._h, self._pack._h, out.ctypes.data))
        return out


def _result_matrix(n_rows, n_cols):
    """The feature matrix of a host-side extraction: page-locked when it is large enough for the copy-out to matter."""
    if n_rows * n_cols * 8 >= (4 << 20) and os.environ.get("TSFRESH_AMD_PINNED", "1") != "0":
        return pinned_empty((n_rows, n_cols), np.float64)
    return np.empty((n_rows, n_cols), dtype=np.float64)


def _samples(values):
    """The samples as tsfa_extract* read them: -> (C-contiguous ndarray, float32 as it is and anything else as float64; its
    TSFA_F32 / TSFA_F64 code)."""
    values = np.ascontiguousarray(values)
    if values.dtype == np.float32:
        return values, TSFA_F32
    return np.ascontiguousarray(values, dtype=np.float64), TSFA_F64


class Plan(_Owner):
    """Owns a `tsfa_plan*`: the compiled list of output columns of one kind on one device."""

    _destroy = "tsfa_plan_destroy"

    def __init__(self, specs, device=0):
        """specs: iterable of (calc_id, (p0, p1, p2, p3)).  A parameter tuple longer than four carries an ARRAY-valued
        parameter in p[4:] (query_similarity_count's query: registry._query_similarity_encode); those samples go to the plan's
        float64 pool and p[2] becomes their offset (tsfa_plan_create_with_data)."""
        lib = load()
        specs = list(specs)
        arr = (FeatureSpec * max(len(specs), 1))()
        pool = []
        for i, (cid, p) in enumerate(specs):
            arr[i].calc = int(cid)
            arr[i].reserved = 0
            for k in range(4):
                arr[i].p[k] = float(p[k])
            if len(p) > 4:
                arr[i].p[2] = float(len(pool))
                pool.extend(float(v) for v in p[4:])
        handle = ctypes.c_void_p()
        if pool:
            pool_arr = np.ascontiguousarray(pool, dtype=np.float64)
            _check(lib, lib.tsfa_plan_create_with_data(arr, len(specs), pool_arr.ctypes.data, len(pool_arr), int(device),
                                                       ctypes.byref(handle)))
        else:
            _check(lib, lib.tsfa_plan_create(arr, len(specs), int(device), ctypes.byref(handle)))
        self._lib = lib
        self._h = handle
        self.n_cols = len(specs)
        self.device = int(device)

    def set_option(self, name, value=1.0):
        """A launch option of this plan (include/tsfresh_amd.h: tsfa_plan_set_option): an alternative route to the same
        numbers, or a diagnostic pre-fill.  Environment variables do not reach the kernels."""
        _check(self._lib, self._lib.tsfa_plan_set_option(self._h, name.encode("ascii"), float(value)))

    def set_profiling(self, enable=True):
        _check(self._lib, self._lib.tsfa_plan_set_profiling(self._h, 1 if enable else 0))

    def set_length_hint(self, min_len, max_len):
        """Promise the length range of every following batch (skips the per-call length scan and its host sync)."""
        _check(self._lib, self._lib.tsfa_plan_set_length_hint(self._h, int(min_len), int(max_len)))

    def last_timings(self):
        cap = 32
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_float * cap)()
        n = self._lib.tsfa_plan_last_timings(self._h, names, ms, cap)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    def last_launches(self):
        """One dict per (kernel family, launch group) of the last extract on this plan, in launch order: family (a name of
        FAMILY_NAMES), length_class, max_len, n_series, threads, lds_bytes, long_build, variant (include/tsfresh_amd.h:
        tsfa_plan_last_launches).  Read-only."""
        fn = self._lib.tsfa_plan_last_launches
        n = fn(self._h, None, 0)
        arr = (LaunchInfo * max(n, 1))()
        n = min(n, fn(self._h, arr, n))
        return [dict({name: int(getattr(arr[i], name)) for name, _ in LaunchInfo._fields_}, family=FAMILY_NAMES[arr[i].family])
                for i in range(n)]

    def extract_host(self, values, offsets, times=None, out=None):
        """values: 1-D float32/float64 ndarray; offsets: int64 ndarray (n_series + 1) -> float64 [n_series, n_cols].
        times: float64 ndarray laid out like `values` (hours since each series' first timestamp) for plans that
        hold linear_trend_timewise columns.  out: optional C-contiguous-row float64 [n_series, >= n_cols] target (a row
        slice of a larger matrix); default: a new page-locked matrix."""
        values, dt = _samples(values)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n_series = offsets.shape[0] - 1
        if out is None:
            out = _result_matrix(n_series, self.n_cols)
        elif (out.dtype != np.float64 or out.ndim != 2 or out.shape[0] != n_series or out.shape[1] < self.n_cols
              or out.strides[1] != 8 or out.strides[0] % 8):
            raise ValueError("out must be a float64 [n_series, >= n_cols] matrix with contiguous rows")
        ld = out.strides[0] // 8 if n_series else self.n_cols
        if n_series == 0 or self.n_cols == 0:
            return out
        if values.size == 0:
            raise ValueError("every series must hold at least one sample")
        tptr = None
        if times is not None:
            times = np.ascontiguousarray(times, dtype=np.float64)
            if times.shape != values.shape:
                raise ValueError("times must have one entry per sample")
            tptr = times.ctypes.data
        _check(self._lib, self._lib.tsfa_extract_timed(self._h, values.ctypes.data, dt, tptr, offsets.ctypes.data, n_series,
                                                       out.ctypes.data, ld, TSFA_HOST, None))
        return out

    def extract_windows_host(self, values, starts, ends, times=None):
        """Window views of one shared buffer: series s = values[starts[s]:ends[s]] (views may overlap) ->
        float64 [n_windows, n_cols].  The rolled (forecasting) layout without materialising the windows."""
        values, dt = _samples(values)
        starts = np.ascontiguousarray(starts, dtype=np.int64)
        ends = np.ascontiguousarray(ends, dtype=np.int64)
        if starts.shape != ends.shape or starts.ndim != 1:
            raise ValueError("starts and ends must be 1-D arrays of the same length")
        n = starts.shape[0]
        out = _result_matrix(n, self.n_cols)
        if n == 0 or self.n_cols == 0:
            return out
        if starts.min() < 0 or ends.max() > values.shape[0]:
            raise ValueError("a window reaches outside the value buffer")
        tptr = None
        if times is not None:
            times = np.ascontiguousarray(times, dtype=np.float64)
            tptr = times.ctypes.data
        _check(self._lib, self._lib.tsfa_extract_windows(self._h, values.ctypes.data, dt, tptr, starts.ctypes.data, ends.ctypes.data,
                                                         n, out.ctypes.data, self.n_cols, TSFA_HOST, None))
        return out

    def extract_pack(self, pack, out=None):
        """The series of a DevicePack -> float64 [n_series, n_cols] on the host: the samples never visit the host
        (tsfa_extract with the pack's device pointers into a device matrix that comes back in one copy)."""
        if out is None:
            out = _result_matrix(pack.n_series, self.n_cols)
        if pack.n_series == 0 or self.n_cols == 0:
            return out
        dm = DeviceMatrix(pack.n_series, self.n_cols, self.device)
        try:
            self.extract_into(None, None, dm, pack=pack)
            dm.to_host(out=out)
        finally:
            dm.free()
        return out

    def extract_windows_pack(self, pack, windows, out=None, chunk_rows=None):
        """The windows of a DeviceWindows over the samples of its DevicePack -> float64 [n_windows, n_cols] on the host:
        tsfa_extract_windows with the pack's value pointer and the handle's starts / ends, nothing is uploaded.  The device
        result matrix comes back in row chunks (chunk_rows windows each; default: the cuts of the TSFA_HOST pipeline, tsfa_extract_chunks, up to 16), so a
        large window count does not need one n_windows x n_cols allocation next to the samples.
        out: optional C-contiguous float64 [n_windows, n_cols] target."""
        n = windows.n_windows
        if pack.device != self.device or windows.device != self.device:
            raise ValueError("the pack and the windows must live on the plan's device")
        if out is None:
            out = _result_matrix(n, self.n_cols)
        elif out.dtype != np.float64 or out.shape != (n, self.n_cols) or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 [n_windows, n_cols] matrix")
        if n == 0 or self.n_cols == 0:
            return out
        if chunk_rows is None:
            # the cuts of the TSFA_HOST pipeline, from the library: the same launches as extract_windows_host, bit-equal features
            edges = (ctypes.c_int64 * 17)()
            n_chunks = self._lib.tsfa_extract_chunks(self._h, n, edges, 17)
            if n_chunks < 0:
                _check(self._lib, n_chunks)
            cuts = [(int(edges[c]), int(edges[c + 1])) for c in range(n_chunks)]
        else:
            chunk_rows = max(1, min(int(chunk_rows), n))
            cuts = [(r0, min(r0 + chunk_rows, n)) for r0 in range(0, n, chunk_rows)]
        dm = DeviceMatrix(max(r1 - r0 for r0, r1 in cuts), self.n_cols, self.device)
        try:
            for r0, r1 in cuts:
                rows = r1 - r0
                _check(self._lib, self._lib.tsfa_extract_windows(
                    self._h, pack.values_ptr, pack.values_type, None, windows.starts_ptr + 8 * r0, windows.ends_ptr + 8 * r0,
                    rows, dm.ptr, dm.ld, TSFA_DEVICE, None))
                part = out[r0:r0 + rows]
                _check(self._lib, self._lib.tsfa_device_copy(part.ctypes.data, dm.ptr, part.nbytes, 0, self.device))
        finally:
            dm.free()
        return out

    def extract_windows_into(self, values_ptr, values_type, starts_ptr, ends_ptr, n_windows, matrix, col0=0, times_ptr=None):
        """Device pointers (ints) in, columns [col0, col0 + n_cols) of the DeviceMatrix / BorrowedMatrix `matrix` out: window
        w is the view [starts[w], ends[w]) of the value buffer at values_ptr (TSFA_F32 / TSFA_F64), all of it on the matrix'
        device -- one tsfa_extract_windows call with TSFA_DEVICE pointers, nothing is uploaded and the rows stay in HBM.
        times_ptr: float64 hours laid out like the value buffer (`pack_times`), for plans that hold linear_trend_timewise
        columns; the kernel rebases them on each window's first stamp."""
        n_windows = int(n_windows)
        if matrix.device != self.device or matrix.shape[0] != n_windows or col0 < 0 or col0 + self.n_cols > matrix.shape[1]:
            raise ValueError("the device matrix does not hold [n_windows, col0 + n_cols] cells on the plan's device")
        if n_windows == 0 or self.n_cols == 0:
            return
        _check(self._lib, self._lib.tsfa_extract_windows(self._h, values_ptr, int(values_type), times_ptr or None, starts_ptr, ends_ptr,
                                                         n_windows, matrix.ptr + 8 * col0, matrix.ld, TSFA_DEVICE, None))

    def extract_into(self, values, offsets, matrix, col0=0, times=None, pack=None, times_ptr=None):
        """Host arrays in, columns [col0, col0 + n_cols) of the DeviceMatrix `matrix` out: the samples are copied to the
        device once and the feature rows stay there (tsfa_extract / tsfa_extract_timed with TSFA_DEVICE pointers).
        pack: a DevicePack on the matrix' device instead of `values` / `offsets` -- nothing is uploaded.
        times_ptr (with pack): a device pointer (int) to float64 hours laid out like the pack's samples (`pack_times`)."""
        if times_ptr is not None and pack is None:
            raise ValueError("times_ptr goes with pack=: host arrays bring their times as `times`")
        if pack is not None:
            if pack.device != matrix.device or matrix.shape[0] != pack.n_series or col0 < 0 or col0 + self.n_cols > matrix.shape[1]:
                raise ValueError("the device matrix does not hold [n_series, col0 + n_cols] cells on the pack's device")
            if pack.n_series == 0 or self.n_cols == 0:
                return
            _check(self._lib, self._lib.tsfa_extract_timed(
                self._h, pack.values_ptr, pack.values_type, times_ptr or None, pack.offsets_ptr, pack.n_series,
                matrix.ptr + 8 * col0, matrix.ld, TSFA_DEVICE, None))
            return
        values, dt = _samples(values)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n_series = offsets.shape[0] - 1
        if matrix.shape[0] != n_series or col0 < 0 or col0 + self.n_cols > matrix.shape[1]:
            raise ValueError("the device matrix does not hold [n_series, col0 + n_cols] cells")
        if n_series == 0 or self.n_cols == 0:
            return
        if values.size == 0:
            raise ValueError("every series must hold at least one sample")
        bufs = [_DeviceBuffer(self._lib, values, matrix.device), _DeviceBuffer(self._lib, offsets, matrix.device)]
        try:
            tptr = None
            if times is not None:
                times = np.ascontiguousarray(times, dtype=np.float64)
                if times.shape != values.shape:
                    raise ValueError("times must have one entry per sample")
                bufs.append(_DeviceBuffer(self._lib, times, matrix.device))
                tptr = bufs[2].ptr
            _check(self._lib, self._lib.tsfa_extract_timed(self._h, bufs[0].ptr, dt, tptr, bufs[1].ptr, n_series,
                                                           matrix.ptr + 8 * col0, matrix.ld, TSFA_DEVICE, None))
        finally:
            for bf in bufs:
                bf.free()

    def extract_device(self, values_ptr, dtype, offsets_ptr, n_series, out_ptr, ld_out, stream=None):
        """Raw device-pointer entry (ints): used with torch tensors (`.data_ptr()`) by bench.py / the sharded path."""
        _check(self._lib, self._lib.tsfa_extract(self._h, values_ptr, int(dtype), offsets_ptr, int(n_series), out_ptr, int(ld_out),
                                                 TSFA_DEVICE, stream or None))


class DeviceMatrix:
    """Row-major float64 [n_rows, n_cols] in the HBM of one device (tsfa_device_alloc): the feature matrix of the chain
    extract -> impute -> select when it never leaves the GPU (convenience.extract_relevant_features(device_resident=True)).
    Owns its memory; `to_host(cols)` fetches the named column indices (tsfa_gather_columns) or everything."""

    def __init__(self, n_rows, n_cols, device=0):
        self._lib = load()
        self.shape = (int(n_rows), int(n_cols))
        self.device = int(device)
        self._ptr = ctypes.c_void_p()
        _check(self._lib, self._lib.tsfa_device_alloc(ctypes.byref(self._ptr), max(1, 8 * self.shape[0] * self.shape[1]),
                                                      self.device))

    @property
    def ptr(self):
        return self._ptr.value

    @property
    def ld(self):
        return self.shape[1]

    def free(self):
        if getattr(self, "_ptr", None) is not None and self._ptr.value:
            self._lib.tsfa_device_free(self._ptr, self.device)
            self._ptr = ctypes.c_void_p()

    def __del__(self):
        import sys
        if sys is not None and not sys.is_finalizing():
            try:
                self.free()
            except Exception:
                pass

    def to_host(self, cols=None, out=None):
        n, m = self.shape
        if cols is None:
            if out is None:
                out = np.empty((n, m), dtype=np.float64)
            elif out.dtype != np.float64 or out.shape != (n, m) or not out.flags.c_contiguous:
                raise ValueError("out must be a C-contiguous float64 matrix of the device matrix' shape")
            _check(self._lib, self._lib.tsfa_device_copy(out.ctypes.data, self._ptr, out.nbytes, 0, self.device))
            return out
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        out = np.empty((n, cols.shape[0]), dtype=np.float64)
        _check(self._lib, self._lib.tsfa_gather_columns(self._ptr, n, m, cols.ctypes.data, cols.shape[0], out.ctypes.data,
                                                        self.device))
        return out


def extract_parts_into(parts, values, offsets, matrix, col0=0, times=None, pack=None, times_ptr=None):
    """Several native plans over ONE upload of the samples: parts = [(Plan, column indices in the caller's order)].  Every
    part's block is extracted into a transient device matrix and scattered (tsfa_scatter_columns) into columns
    col0 + cols of `matrix` (a DeviceMatrix): the composite plans of feature_extraction/extraction.py (several ADF lag
    selections, more than 128 CWT columns) without an upload per part, and with the matrix staying in HBM.
    pack: a DevicePack on the matrix' device instead of `values` / `offsets` -- no upload at all; times_ptr: with it, a
    device pointer (int) to float64 hours laid out like the pack's samples (`pack_times`), handed to every part."""
    lib = load()
    device = matrix.device
    if times_ptr is not None and pack is None:
        raise ValueError("times_ptr goes with pack=: host arrays bring their times as `times`")
    if pack is not None:
        if pack.device != device or pack.n_series != matrix.shape[0]:
            raise ValueError("the device matrix does not hold the pack's series on the pack's device")
        n_series = pack.n_series
    else:
        values, dt = _samples(values)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n_series = offsets.shape[0] - 1
    if n_series == 0:
        return
    if pack is None and values.size == 0:
        raise ValueError("every series must hold at least one sample")
    bufs, tmp = [], None
    try:
        if pack is not None:
            vptr, dt, optr, tptr = pack.values_ptr, pack.values_type, pack.offsets_ptr, times_ptr or None
        else:   # one upload of the samples, the offsets and the times for all parts
            host = [values, offsets] + ([] if times is None else [np.ascontiguousarray(times, dtype=np.float64)])
            for a in host:
                bufs.append(_DeviceBuffer(lib, a, device))
            vptr, optr, tptr = bufs[0].ptr, bufs[1].ptr, (None if times is None else bufs[2].ptr)
        tmp = DeviceMatrix(n_series, max(plan.n_cols for plan, _ in parts), device)
        for plan, cols in parts:
            if plan.n_cols == 0:
                continue
            _check(lib, lib.tsfa_extract_timed(plan._h, vptr, dt, tptr, optr, n_series, tmp.ptr, plan.n_cols, TSFA_DEVICE, None))
            idx = np.ascontiguousarray(np.asarray(cols, dtype=np.int64) + int(col0), dtype=np.int32)
            _check(lib, lib.tsfa_scatter_columns(matrix.ptr, matrix.ld, idx.ctypes.data, tmp.ptr, n_series, plan.n_cols, device))
    finally:
        for bf in bufs:
            bf.free()
        if tmp is not None:
            tmp.free()


def extract_parts_windows_into(parts, values_ptr, values_type, starts_ptr, ends_ptr, n_windows, matrix, col0=0, times_ptr=None):
    """The window twin of `extract_parts_into(pack=...)`: several native plans over the same device buffers.  Every part's
    block of the windows [starts[w], ends[w]) of the value buffer at values_ptr is extracted into a transient device matrix
    and scattered (tsfa_scatter_columns) into columns col0 + cols of `matrix` (a DeviceMatrix or a BorrowedMatrix).
    times_ptr: as in `Plan.extract_windows_into`, handed to every part."""
    lib = load()
    n_windows = int(n_windows)
    if matrix.shape[0] != n_windows:
        raise ValueError("the device matrix does not hold one row per window")
    if col0 < 0 or any(len(cols) and int(col0) + int(max(cols)) >= matrix.shape[1] for _, cols in parts):
        raise ValueError("the device matrix does not hold the parts' columns from col0 on")
    if n_windows == 0:
        return
    tmp = DeviceMatrix(n_windows, max(plan.n_cols for plan, _ in parts), matrix.device)
    try:
        for plan, cols in parts:
            if plan.n_cols == 0:
                continue
            plan.extract_windows_into(values_ptr, values_type, starts_ptr, ends_ptr, n_windows,
                                      BorrowedMatrix(tmp.ptr, n_windows, plan.n_cols, matrix.device, owner=tmp),
                                      times_ptr=times_ptr)
            idx = np.ascontiguousarray(np.asarray(cols, dtype=np.int64) + int(col0), dtype=np.int32)
            _check(lib, lib.tsfa_scatter_columns(matrix.ptr, matrix.ld, idx.ctypes.data, tmp.ptr, n_windows, plan.n_cols,
                                                 matrix.device))
    finally:
        tmp.free()


class _DeviceBuffer:
    """A transient device copy of a host array (inputs of Plan.extract_into)."""

    def __init__(self, lib, array, device):
        self._lib, self.device = lib, device
        self._ptr = ctypes.c_void_p()
        _check(lib, lib.tsfa_device_alloc(ctypes.byref(self._ptr), max(1, array.nbytes), device))
        _check(lib, lib.tsfa_device_copy(self._ptr, array.ctypes.data, array.nbytes, 1, device))

    @property
    def ptr(self):
        return self._ptr.value

    def free(self):
        if self._ptr.value:
            self._lib.tsfa_device_free(self._ptr, self.device)
            self._ptr = ctypes.c_void_p()


def _matrix_args(X):
    """(pointer, n_rows, n_cols, ld, space, keepalive) of a host ndarray or a DeviceMatrix."""
    if isinstance(X, DeviceMatrix):
        return X.ptr, X.shape[0], X.shape[1], X.ld, TSFA_DEVICE, X
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X must be two-dimensional")
    return X.ctypes.data, X.shape[0], X.shape[1], X.shape[1], TSFA_HOST, X


def relevance_classes(X, y_codes, n_classes, device=0, with_ks=False):
    """Per-column relevance statistics of the row-major float64 matrix X against class codes (tsfa_relevance_classes).
    -> (n_unique int64[m], v_lo[m], v_hi[m], tie_term[m], rank_sums[m, C], hi_counts[m, C]) (+ ks_d[m, C] with_ks)."""
    lib = load()
    xptr, n, m, ld, space, _keep = _matrix_args(X)
    y_codes = np.ascontiguousarray(y_codes, dtype=np.int32)
    if y_codes.shape != (n,):
        raise ValueError("one class code per row")
    cols = np.zeros(max(m, 1), dtype=_CLASS_COL_DTYPE)
    rank_sums = np.zeros((m, n_classes), dtype=np.float64)
    hi_counts = np.zeros((m, n_classes), dtype=np.int64)
    args = (xptr, n, m, ld, space, y_codes.ctypes.data, int(n_classes), int(device), cols.ctypes.data, rank_sums.ctypes.data,
            hi_counts.ctypes.data)
    if with_ks:
        ks_d = np.zeros((m, n_classes), dtype=np.float64)
        _check(lib, lib.tsfa_relevance_classes_ks(*args, ks_d.ctypes.data))
    else:
        _check(lib, lib.tsfa_relevance_classes(*args))
    rec = cols[:m]
    res = (rec["n_unique"].copy(), rec["v_lo"].copy(), rec["v_hi"].copy(), rec["tie_term"].copy(), rank_sums, hi_counts)
    return res + (ks_d,) if with_ks else res


def relevance_real(X, y, device=0):
    """Per-column statistics of the row-major float64 matrix X against a real-valued target (tsfa_relevance_real).
    -> (structured array with the fields of tsfa_relevance_real_col, dense ranks of y)."""
    lib = load()
    xptr, n, m, ld, space, _keep = _matrix_args(X)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.shape != (n,):
        raise ValueError("one target value per row")
    # the target is one vector: its dense ranks / sorted order are prepared here once for all columns
    y_rank, y_perm, y_end = target_order(y)
    cols = np.zeros(max(m, 1), dtype=_REAL_COL_DTYPE)
    _check(lib, lib.tsfa_relevance_real(xptr, n, m, ld, space, y_rank.ctypes.data, y_perm.ctypes.data, y_end.ctypes.data,
                                        int(device), cols.ctypes.data))
    return cols[:m], y_rank


def impute_matrix(X, device=0):
    """In-place impute of the C-contiguous-row float64 matrix X on the device (tsfa_impute).
    -> (col_max, col_min, col_median of the finite values, number of finite cells per column)."""
    lib = load()
    if isinstance(X, DeviceMatrix):
        xptr, (n, m), ld, space = X.ptr, X.shape, X.ld, TSFA_DEVICE
        device = X.device
    else:
        if not (isinstance(X, np.ndarray) and X.dtype == np.float64 and X.ndim == 2 and X.flags.writeable
                and (X.shape[1] == 0 or X.strides[1] == 8) and X.strides[0] % 8 == 0 and X.strides[0] >= 8 * X.shape[1]):
            raise ValueError("impute_matrix needs a writeable float64 matrix with contiguous rows")
        n, m = X.shape
        xptr, ld, space = X.ctypes.data, (X.strides[0] // 8 if n else m), TSFA_HOST
    cmax, cmin, cmed = (np.zeros(m) for _ in range(3))
    cnt = np.zeros(m, dtype=np.int32)
    _check(lib, lib.tsfa_impute(xptr, n, m, ld, space, int(device), cmax.ctypes.data, cmin.ctypes.data, cmed.ctypes.data,
                                cnt.ctypes.data))
    return cmax, cmin, cmed, cnt


def impute_ptr(x_ptr, n_rows, n_cols, ld, space, device=0):
    """tsfa_impute in place on the float64 matrix at x_ptr (host or device memory by `space`), leading dimension ld."""
    lib = load()
    _check(lib, lib.tsfa_impute(x_ptr, int(n_rows), int(n_cols), int(ld), int(space), int(device), None, None, None, None))


def ks_outer_prob(m, n, g, h):
    return float(load().tsfa_ks_outer_prob(int(m), int(n), int(g), int(h)))


# ---- selection on the device (tsfa_relevance_tails_* / tsfa_relevance_fdr / tsfa_compact_mask / tsfa_gather_columns_device):
# the matrix and every output are device pointers (ints, e.g. torch's `.data_ptr()`) owned by the caller ----

def _ks_tail_code(ks_tail):
    if ks_tail not in ("host", "device"):
        raise ValueError("ks_tail must be 'host' or 'device', not {!r}".format(ks_tail))
    return TSFA_KS_TAIL_DEVICE if ks_tail == "device" else TSFA_KS_TAIL_HOST


def ks_tails(n1_ptr, n2_ptr, d_ptr, n_cells, p_ptr, route_ptr, device=0):
    """tsfa_ks_tails: the exact Kolmogorov-Smirnov tails of n_cells triples (n1 int64, n2 int64, d float64: device arrays) into
    the device arrays p [n_cells] float64 and route [n_cells] uint8 (TSFA_ROUTE_KS_EXACT, or NaN and TSFA_ROUTE_HOST_KS)."""
    lib = load()
    _check(lib, lib.tsfa_ks_tails(n1_ptr, n2_ptr, d_ptr, int(n_cells), int(device), p_ptr, route_ptr))


def relevance_tails_classes(x_ptr, n_rows, n_cols, ld, y_codes, n_classes, p_ptr, route_ptr, type_ptr, device=0, with_ks=False,
                            want_stats=False, ks_tail="host", ks_d_ptr=None):
    """The class tables of the device matrix at x_ptr, left on the device: p [m, C] float64, route [m, C] uint8, type [m]
    uint8 -> (host-route cells, statistics).  statistics (want_stats): what `relevance_classes` returns, for the caller's
    host routes; None otherwise (nothing but the cell count is copied).  ks_tail="device" (tsfa_relevance_tails_classes_ks)
    serves the exact Kolmogorov-Smirnov tails on the device; ks_d_ptr: an optional device array [m, C] float64 that receives
    the Kolmogorov-Smirnov distances (with_ks), and the statistics then come without them."""
    ks_code = _ks_tail_code(ks_tail)
    lib = load()
    y_codes = np.ascontiguousarray(y_codes, dtype=np.int32)
    if y_codes.shape != (n_rows,):
        raise ValueError("one class code per row")
    n_host = ctypes.c_int64(0)
    cols = rank_sums = hi_counts = ks_d = None
    if want_stats:
        cols = np.zeros(max(n_cols, 1), dtype=_CLASS_COL_DTYPE)
        rank_sums = np.zeros((n_cols, n_classes), dtype=np.float64)
        hi_counts = np.zeros((n_cols, n_classes), dtype=np.int64)
        ks_d = np.zeros((n_cols, n_classes), dtype=np.float64) if (with_ks and ks_d_ptr is None) else None
    stats_ptrs = [None if a is None else a.ctypes.data for a in (cols, rank_sums, hi_counts, ks_d)]
    head = (x_ptr, int(n_rows), int(n_cols), int(ld), TSFA_DEVICE, y_codes.ctypes.data, int(n_classes), int(bool(with_ks)))
    if ks_code == TSFA_KS_TAIL_HOST and ks_d_ptr is None:
        _check(lib, lib.tsfa_relevance_tails_classes(*head, int(device), p_ptr, route_ptr, type_ptr, *stats_ptrs,
                                                     ctypes.byref(n_host)))
    else:
        _check(lib, lib.tsfa_relevance_tails_classes_ks(*head, ks_code, int(device), p_ptr, route_ptr, type_ptr, *stats_ptrs,
                                                        ks_d_ptr, ctypes.byref(n_host)))
    stats = None
    if want_stats:
        stats = (cols["n_unique"][:n_cols].copy(), cols["tie_term"][:n_cols].copy(), rank_sums, hi_counts, ks_d)
    return int(n_host.value), stats


def target_order(y):
    """(dense ranks, ascending order, tie-group ends) of a real target: what tsfa_relevance_real takes."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = y.shape[0]
    _, inverse = np.unique(y, return_inverse=True)
    y_rank = np.ascontiguousarray(inverse, dtype=np.int32)
    y_perm = np.ascontiguousarray(np.argsort(y, kind="stable"), dtype=np.int32)
    ys = y[y_perm]
    y_end = np.ones(n, dtype=np.uint8)
    if n > 1:
        y_end[:-1] = ys[1:] != ys[:-1]
    return y_rank, y_perm, y_end


def relevance_tails_real(x_ptr, n_rows, n_cols, ld, y, tie_statistics, p_ptr, route_ptr, type_ptr, device=0, want_stats=False,
                         ks_tail="host", n_hi_ptr=None, ks_d_ptr=None):
    """The table of a real target for the device matrix at x_ptr, left on the device: p [m], route [m], type [m] ->
    (host-route cells, records).  tie_statistics: callable dense ranks -> (ytie, y0, y1).  records (want_stats): the
    structured array `relevance_real` returns.  ks_tail="device" (tsfa_relevance_tails_real_ks) serves the exact
    Kolmogorov-Smirnov tails on the device; n_hi_ptr / ks_d_ptr: optional device arrays [m] (int64 / float64) that receive
    the two-valued columns' statistics."""
    ks_code = _ks_tail_code(ks_tail)
    lib = load()
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.shape != (n_rows,):
        raise ValueError("one target value per row")
    y_rank, y_perm, y_end = target_order(y)
    ytie, y0, y1 = tie_statistics(y_rank)
    n_host = ctypes.c_int64(0)
    cols = np.zeros(max(n_cols, 1), dtype=_REAL_COL_DTYPE) if want_stats else None
    cols_ptr = None if cols is None else cols.ctypes.data
    head = (x_ptr, int(n_rows), int(n_cols), int(ld), TSFA_DEVICE, y_rank.ctypes.data, y_perm.ctypes.data, y_end.ctypes.data,
            int(ytie), float(y0), float(y1))
    if ks_code == TSFA_KS_TAIL_HOST and n_hi_ptr is None and ks_d_ptr is None:
        _check(lib, lib.tsfa_relevance_tails_real(*head, int(device), p_ptr, route_ptr, type_ptr, cols_ptr, ctypes.byref(n_host)))
    else:
        _check(lib, lib.tsfa_relevance_tails_real_ks(*head, ks_code, int(device), p_ptr, route_ptr, type_ptr, cols_ptr, n_hi_ptr,
                                                     ks_d_ptr, ctypes.byref(n_host)))
    return int(n_host.value), (None if cols is None else cols[:n_cols])


def relevance_fdr(p_ptr, type_ptr, n_cols, n_tables, alpha, c_m, n_significant, multiclass, rel_table_ptr, relevant_ptr,
                  n_significant_ptr, p_min_ptr, device=0):
    """tsfa_relevance_fdr: the step-up per table and the combination of the tables, device arrays in and out."""
    lib = load()
    _check(lib, lib.tsfa_relevance_fdr(p_ptr, type_ptr, int(n_cols), int(n_tables), float(alpha), float(c_m), int(n_significant),
                                       int(bool(multiclass)), int(device), rel_table_ptr, relevant_ptr, n_significant_ptr,
                                       p_min_ptr))


def compact_mask(mask_ptr, n, indices_ptr, device=0):
    """tsfa_compact_mask: ascending int32 indices of the non-zero bytes of the device mask -> their count."""
    lib = load()
    count = ctypes.c_int64(0)
    _check(lib, lib.tsfa_compact_mask(mask_ptr, int(n), indices_ptr, ctypes.byref(count), int(device)))
    return int(count.value)


def gather_columns_device(x_ptr, n_rows, ld, cols_ptr, n_sel, out_ptr, ld_out, device=0):
    """tsfa_gather_columns_device: out[r, c] = X[r, cols[c]] within HBM."""
    lib = load()
    _check(lib, lib.tsfa_gather_columns_device(x_ptr, int(n_rows), int(ld), cols_ptr, int(n_sel), out_ptr, int(ld_out), int(device)))
