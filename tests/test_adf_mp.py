"""tests/adf_mp.py is the reference of tests/test_dd_passes_gpu.py: its pinv functions are pinned here to the full-rank
60-digit solver of the same file and to the output of the real statsmodels (tests/golden/ref_conda*.npz)."""
import os

import numpy as np
import pytest

import goldens
from adf_mp import adf_pvalue, adfuller_aic_mp, adfuller_pinv_mp, autoreg_params_mp, autoreg_params_pinv_mp

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WELL_CONDITIONED = ["randn_f32_300_0", "randn_f32_300_1", "randn_f32_300_2", "walk_f32_256", "ints_dup_100", "decimals_200",
                    "randn_f64_37", "sine_noise_512", "short_45", "big_scale_128"]


def test_pinv_rule_equals_the_full_rank_solver_on_full_rank_series():
    rng = np.random.default_rng(20261017)
    for x in (rng.standard_normal(120), np.cumsum(rng.standard_normal(150)), 40.0 + rng.standard_normal(90)):
        t, lag = adfuller_aic_mp(x)
        t2, lag2, facts = adfuller_pinv_mp(x, "AIC")
        assert lag2 == lag and abs(t2 - t) <= 1e-13 * abs(t), (t, t2, lag, lag2)
        assert not facts["perfect"] and min(min(r) for r in facts["ratios"]) > 1e-11
        beta, _, rank, _, _ = autoreg_params_pinv_mp(x, 10)
        assert rank == 11
        np.testing.assert_allclose(beta, autoreg_params_mp(x, 10), rtol=1e-12, atol=0)


@pytest.mark.parametrize("label", WELL_CONDITIONED)
def test_every_lag_selection_reproduces_statsmodels(label):
    main = goldens.load("main")
    other = np.load(os.path.join(G, "ref_conda_adf.npz"))
    i = main["labels"].index(label)
    assert [str(l) for l in other["labels"]][i] == label
    x = main["series"][i]
    for autolag in ("AIC", "BIC", "t-stat", None):
        names, row = (main["names"], main["matrix"][i]) if autolag == "AIC" else (list(other["names"]), other["matrix"][i])
        want = {a: row[names.index('value__augmented_dickey_fuller__attr_"%s"__autolag_"%s"' % (a, autolag))]
                for a in ("teststat", "pvalue", "usedlag")}
        t, lag, facts = adfuller_pinv_mp(x, autolag)
        assert lag == want["usedlag"], (autolag, lag, want)
        assert abs(t - want["teststat"]) <= 1e-6 * abs(want["teststat"]), (autolag, t, want)
        assert abs(adf_pvalue(t) - want["pvalue"]) <= 1e-6 * abs(want["pvalue"]) + 1e-9, (autolag, adf_pvalue(t), want)
        assert len(facts["ratios"]) >= 1 and not facts["perfect"]
