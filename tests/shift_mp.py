"""TEST INFRASTRUCTURE: a core of the level-invariant columns restated from their definitions in 50-digit arithmetic
(mpmath) and evaluated on the SHIFTED series x = c + b -- in 50 digits a level of 2^30 costs nine of them and nothing
else.  tests/test_shift_invariance.py compares the oracle's float64 values on the base b with these: the truth the
invariance tests use (oracle(b), tests/shift_cases.py) is then anchored in the definitions and not in the oracle's own
arithmetic.  The style follows tests/adf_mp.py and tests/polyfit_mp.py."""
import mpmath as mp

DPS = 50
LAGS = range(1, 10)
BINS = range(1, 6)


def core_columns(x):
    """x: float64 samples -> {column name: mp.mpf} of
    variance, standard_deviation (np.var / np.std, ddof 0), skewness, kurtosis (pandas' bias-corrected G1 and G2),
    autocorrelation lags 1 .. 9 (fc.py:1919), cid_ce with both normalisations (fc.py:567), mean_second_derivative_central
    (fc.py:644), linear_trend slope / rvalue / stderr (scipy.stats.linregress against 0 .. n - 1) and fft_coefficient real /
    imag / abs of bins 1 .. 5 by a direct DFT (np.fft.rfft's sign convention: exp(-2 pi i k t / n))."""
    with mp.workdps(DPS):
        x = [mp.mpf(float(v)) for v in x]
        n = len(x)
        mean = mp.fsum(x) / n
        d = [v - mean for v in x]
        m2, m3, m4 = (mp.fsum(v ** p for v in d) / n for p in (2, 3, 4))
        out = {"value__variance": m2, "value__standard_deviation": mp.sqrt(m2)}
        out["value__skewness"] = mp.sqrt(mp.mpf(n) * (n - 1)) / (n - 2) * m3 / m2 ** mp.mpf(1.5)
        out["value__kurtosis"] = (mp.mpf(n - 1) / ((n - 2) * (n - 3))) * ((n + 1) * m4 / m2 ** 2 - 3 * (n - 1))
        for lag in LAGS:
            out["value__autocorrelation__lag_%d" % lag] = mp.fsum(d[t] * d[t + lag] for t in range(n - lag)) / ((n - lag) * m2)
        ce = mp.sqrt(mp.fsum((x[t + 1] - x[t]) ** 2 for t in range(n - 1)))
        out["value__cid_ce__normalize_False"] = ce
        out["value__cid_ce__normalize_True"] = ce / mp.sqrt(m2)
        out["value__mean_second_derivative_central"] = (x[-1] - x[-2] - x[1] + x[0]) / (2 * (n - 2))
        tbar = mp.mpf(n - 1) / 2
        sxx = mp.fsum((t - tbar) ** 2 for t in range(n))
        sxy = mp.fsum((t - tbar) * d[t] for t in range(n))
        syy = m2 * n
        r = sxy / mp.sqrt(sxx * syy)
        out['value__linear_trend__attr_"slope"'] = sxy / sxx
        out['value__linear_trend__attr_"rvalue"'] = r
        out['value__linear_trend__attr_"stderr"'] = mp.sqrt((1 - r * r) * syy / sxx / (n - 2))
        for k in BINS:
            re = mp.fsum(x[t] * mp.cospi(mp.mpf(2 * k * t) / n) for t in range(n))
            im = -mp.fsum(x[t] * mp.sinpi(mp.mpf(2 * k * t) / n) for t in range(n))
            out['value__fft_coefficient__attr_"real"__coeff_%d' % k] = re
            out['value__fft_coefficient__attr_"imag"__coeff_%d' % k] = im
            out['value__fft_coefficient__attr_"abs"__coeff_%d' % k] = mp.sqrt(re * re + im * im)
        return out
