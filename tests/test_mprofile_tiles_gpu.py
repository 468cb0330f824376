"""matrix_profile's tiled route (tsfresh_amd/csrc/tsfa_mprofile_tiles.hip, plan option mp_tiles, launch record variant 1): the
sweep of a series cut into tiles of 256 rows by TILE_D diagonals and spread over the chip.  A tile starts every diagonal at
the row where the one-workgroup body restarts it, so every cell must equal the g++ build of that body (emul_mprofile_lib)
bit for bit; the brute force of the definition (mprofile_ref) holds both to the reference."""
import numpy as np
import pytest

import emul_mprofile_lib
import mprofile_cases as cases
import mprofile_ref
from engines import hip_engine

pytestmark = pytest.mark.gpu

TILE_D = 1024   # fam_mprofile.h: TSFA_MP_TILE_D
DIAGONALS = (1, 2, 63, 64, 65, 255, 256, 257, 513, TILE_D - 1, TILE_D, 1025)
EDGE_KINDS = ("noise", "walk", "repeat", "flat_stretch")


def _check(values, offsets, cols, options):
    """The device's cells on the tiles against the emulation (==, NaN where it has NaN) and the brute force."""
    records = []
    _, got = hip_engine(cases.fc_parameters(tuple(dict.fromkeys(w for w, _ in cols))), values, offsets, options=options,
                        launches=records)
    got = np.array(got)
    mp = [r for r in records if r["family"] == "MPROFILE"]
    assert mp and all(r["variant"] == 1 and r["long_build"] == 0 for r in mp), mp
    want = emul_mprofile_lib.emul_mprofile(cols, values, offsets)
    diff = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(diff) == 0, (len(diff), [(int(s), int(c), got[s, c], want[s, c]) for s, c in diff[:6]])
    return got


@pytest.mark.parametrize("batch,reference", [(cases.small_batch, cases.small_reference),
                                             (cases.small_batch_f32, cases.small_reference_f32)], ids=["f64", "f32"])
def test_small_batches_forced_onto_tiles(gpu, batch, reference):
    values, offsets = batch()
    got = _check(values, offsets, cases.columns(), {"mp_tiles": 1})
    bad = cases.mismatches(got, reference(), cases.columns(), offsets)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("w", [4, 36])
def test_tile_edges(gpu, w, dtype):
    """Series with 1 .. 1025 diagonals: one cell, a lane's four diagonals partly empty, a wavefront, a tile and a row block
    just filled and just exceeded -- a second diagonal block of one diagonal, a row block of one row, keys merged from
    several tiles."""
    rng = np.random.default_rng(20261127 + w)
    lengths = [nd + mprofile_ref.exclusion(w) + w for nd in DIAGONALS]   # nd = L - ceil(w/4) - 1, L = n - w + 1
    parts = [cases.series(EDGE_KINDS[k % len(EDGE_KINDS)], n, rng) for k, n in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    values = np.concatenate(parts).astype(dtype)
    cols = cases.columns((w,))
    got = _check(values, offsets, cols, {"mp_tiles": 1})
    bad = cases.mismatches(got, cases.reference(values, offsets, cols), cols, offsets)
    assert not bad, (len(bad), bad[:8])


def test_auto_takes_the_tiles_beyond_the_lds_layout(gpu):
    w = 36
    parts = []
    for n, seed in ((emul_mprofile_lib.longest_in_lds(8) + 1, 31), (9000, 32)):
        x = np.random.default_rng(seed).standard_normal(n)
        x[n - 700:n - 600] = x[400:500]
        parts.append(x)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    values = np.concatenate(parts)
    cols = cases.columns((w,))
    got = _check(values, offsets, cols, None)   # default options
    records = []
    _, one_workgroup = hip_engine(cases.fc_parameters((w,)), values, offsets, options={"mp_tiles": 0}, launches=records)
    mp = [r for r in records if r["family"] == "MPROFILE"]
    assert mp and all(r["variant"] == 0 and r["long_build"] == 1 for r in mp), mp
    assert np.array_equal(got, np.array(one_workgroup), equal_nan=True)
    bad = cases.mismatches(got, cases.reference(values, offsets, cols), cols, offsets)
    assert not bad, bad


def test_mp_tiles_takes_auto_never_and_always(gpu):
    from tsfresh_amd import _native
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    plan = _native.Plan(compile_fc_parameters(cases.fc_parameters((36,))).native_specs(_native.calc_id), device=0)
    try:
        for v in (-1, 0, 1):
            plan.set_option("mp_tiles", v)
        for v in (2, 0.5, -2):
            with pytest.raises(Exception):
                plan.set_option("mp_tiles", v)
    finally:
        plan.close()
