"""Generate tests/golden/ref_distributor.npz: what the REAL reference's `extract_features(distributor=...)` pipeline does
around a distributor, for tests/test_distributor.py::test_the_real_reference_pipeline_drives_the_distributor.

    python tests/golden/gen_golden_distributor.py REFERENCE_TREE     # the directory that holds the tsfresh package

The reference runs in the main interpreter with pywt / statsmodels / stumpy stubbed (as in gen_golden_main.py), and
the five calculators that need them are left out of the parameters.  Recorded:
  * the input frame (ids, lengths, columns "a" and "b"),
  * the call the reference's `_do_extraction` makes on the distributor: the (id, kind, length) order of the chunks it
    hands over, the keys of `function_kwargs` and `chunk_size`,
  * the frame it returns for that input with its own serial distributor (n_jobs=0): index, its dtype, columns, values.
"""
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
NEED_THIRD_PARTY = ("cwt_coefficients", "agg_autocorrelation", "partial_autocorrelation", "augmented_dickey_fuller",
                    "ar_coefficient")


class _Raiser(types.ModuleType):
    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)

        def _fail(*a, **k):
            raise RuntimeError("stubbed third-party module %s.%s was called" % (self.__name__, item))
        return _fail


def frame():
    """The input of the test: five ids of 60-128 samples, a white-noise column and a random-walk column."""
    rng = np.random.default_rng(12)
    frames = []
    for sid, n in zip([11, 3, 7, 5, 9], [60, 75, 64, 90, 128]):
        frames.append(pd.DataFrame({"id": sid, "time": np.arange(n), "a": rng.standard_normal(n),
                                    "b": np.cumsum(rng.standard_normal(n))}))
    return pd.concat(frames, ignore_index=True)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "tsfresh")):
        raise SystemExit(__doc__)
    for mod in ("pywt", "stumpy", "statsmodels", "statsmodels.tools", "statsmodels.tools.sm_exceptions", "statsmodels.tsa",
                "statsmodels.tsa.ar_model", "statsmodels.tsa.stattools", "statsmodels.stats", "statsmodels.stats.multitest"):
        sys.modules[mod] = _Raiser(mod)
    sys.modules["statsmodels.tools.sm_exceptions"].MissingDataError = type("MissingDataError", (Exception,), {})
    sys.path.insert(0, sys.argv[1])
    from tsfresh.feature_extraction import extract_features
    from tsfresh.feature_extraction import settings
    from tsfresh.utilities.distribution import MapDistributor

    class Recorder(MapDistributor):
        def map_reduce(self, map_function, data, function_kwargs=None, chunk_size=None, data_length=None):
            chunks = list(data)
            self.call = {"chunks": [(c[0], c[1], len(c[2])) for c in chunks], "kwargs": sorted(function_kwargs),
                         "chunk_size": chunk_size}
            return super().map_reduce(map_function, chunks, function_kwargs, chunk_size, data_length)

    df = frame()
    params = settings.ComprehensiveFCParameters()
    for k in NEED_THIRD_PARTY:
        del params[k]
    rec = Recorder(disable_progressbar=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        via = extract_features(df, column_id="id", column_sort="time", default_fc_parameters=params, distributor=rec)
        want = extract_features(df, column_id="id", column_sort="time", default_fc_parameters=params, n_jobs=0,
                                disable_progressbar=True)
    pd.testing.assert_frame_equal(via, want)
    assert rec.call["chunk_size"] is None
    out = os.path.join(HERE, "ref_distributor.npz")
    np.savez_compressed(
        out, df_id=df["id"].to_numpy(), df_time=df["time"].to_numpy(), df_a=df["a"].to_numpy(), df_b=df["b"].to_numpy(),
        call_ids=np.array([c[0] for c in rec.call["chunks"]]), call_kinds=np.array([c[1] for c in rec.call["chunks"]]),
        call_lengths=np.array([c[2] for c in rec.call["chunks"]]), call_kwargs=np.array(rec.call["kwargs"]),
        index=want.index.to_numpy(), index_dtype=np.array(str(want.index.dtype)), columns=np.array(list(want.columns)),
        values=want.to_numpy(dtype=np.float64))
    print("wrote", out, want.shape)


if __name__ == "__main__":
    main()
