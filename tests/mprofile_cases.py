"""Inputs shared by the matrix_profile tests (CPU emulation and device): small ragged batches that hold every shape at which
k_mprofile (tsfresh_amd/csrc/fam_mprofile.h) can go wrong, and their brute-force reference, computed once per process."""
import functools

import numpy as np

import mprofile_ref

WINDOWS = (4, 5, 8, 36, 64, 65)
LENGTHS = (63, 64, 65, 129, 257, 1000, 1024)
KINDS = ("noise", "walk", "round1", "ints", "repeat", "flat_stretch", "const")


def columns(windows=WINDOWS):
    return [(w, f) for w in windows for f in mprofile_ref.FEATURES]


def fc_parameters(windows=WINDOWS):
    return {"matrix_profile": [{"windows": w, "feature": f} for w, f in columns(windows)]}


def edge_lengths():
    """n with L = n - w + 1 equal to ceil(w/4) + 1 (no admissible pair: NaN), + 2 (one pair) and + 3, per window."""
    return sorted({mprofile_ref.exclusion(w) + k + w - 1 for w in WINDOWS for k in (1, 2, 3)})


def series(kind, n, rng):
    if kind == "noise":
        return rng.standard_normal(n)
    if kind == "walk":
        return np.cumsum(rng.integers(0, 2, n) * 2.0 - 1.0)
    if kind == "round1":
        return np.round(rng.standard_normal(n), 1)
    if kind == "ints":
        return rng.integers(0, 5, n).astype(np.float64)
    if kind == "repeat":      # a planted exact repeat: P ~ 0 for the windows inside it
        x = rng.standard_normal(n)
        m = min(n // 3, 80)
        x[n - m:] = x[:m]
        return x
    if kind == "flat_stretch":   # a flat stretch longer than the largest window that fits
        x = rng.standard_normal(n)
        m = min(n // 2, 80)
        s = n // 4
        x[s:s + m] = 0.75
        return x
    if kind == "const":
        return np.full(n, 3.25)
    raise ValueError(kind)


def _batch(parts, dtype):
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return np.concatenate(parts).astype(dtype), offsets


@functools.lru_cache(maxsize=None)
def small_batch():
    """float64: every edge length and every general length with the kinds in rotation, and every kind at 257 samples
    (more than one wavefront's diagonals, a restart of the recurrence for the small windows)."""
    rng = np.random.default_rng(20260417)
    parts, k = [], 0
    for n in edge_lengths() + list(LENGTHS):
        parts.append(series(KINDS[k % (len(KINDS) - 1)], n, rng))   # (const: below)
        k += 1
    for kind in KINDS:
        parts.append(series(kind, 257, rng))
    return _batch(parts, np.float64)


@functools.lru_cache(maxsize=None)
def small_batch_f32():
    """float32 input: the general lengths, noise and a rounded series."""
    rng = np.random.default_rng(20260418)
    parts = [series("noise" if i % 2 == 0 else "round1", n, rng) for i, n in enumerate(LENGTHS)]
    return _batch(parts, np.float32)


def reference(values, offsets, cols):
    """Brute force (tests/mprofile_ref.py) of the columns on every series: [n_series x len(cols)]."""
    values = np.asarray(values).astype(np.float64)
    out = np.empty((len(offsets) - 1, len(cols)))
    for s in range(len(offsets) - 1):
        x = values[offsets[s]:offsets[s + 1]]
        prof = {}
        for c, (w, f) in enumerate(cols):
            if w not in prof:
                prof[w] = mprofile_ref.profile(x, w)
            out[s, c] = mprofile_ref.feature(prof[w], f)
    return out


@functools.lru_cache(maxsize=None)
def small_reference():
    return reference(*small_batch(), columns())


@functools.lru_cache(maxsize=None)
def small_reference_f32():
    return reference(*small_batch_f32(), columns())


def mismatches(got, want, cols, offsets):
    """Cells outside tests/mprofile_ref.py's tolerance: [(series, its length, window, feature, got, want)]."""
    bad = []
    for s in range(want.shape[0]):
        for c, (w, f) in enumerate(cols):
            if not mprofile_ref.close(got[s, c], want[s, c], w):
                bad.append((s, int(offsets[s + 1] - offsets[s]), w, f, got[s, c], want[s, c]))
    return bad
