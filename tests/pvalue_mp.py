"""TEST INFRASTRUCTURE: the p-value of scipy.stats.linregress restated in many-digit arithmetic (mpmath), for
tests/test_pvalue_floor.py.  The style follows tests/shift_mp.py and tests/adf_mp.py.

  regression_mp(t, y)      r, t-statistic and 1 - r^2 of the float64 samples, by centred sums in DPS digits -- the definition,
                           term by term (tests/pvalue_cases.py reaches the same r^2 through exact integer sums; the CPU test
                           compares the two)
  t_from_r2_mp(r2, sign, df)  the reference's t = r sqrt(df / ((1 - r + TINY)(1 + r + TINY))), TINY = 1e-20
  pvalue_sum_mp(t, df)     p = 2 sf(|t|, df) = 1 - A(t | df) by the FINITE sums of Abramowitz & Stegun 26.7.3 (odd df, with the
                           arctangent) and 26.7.4 (even df).  1 - A cancels to the size of p: the working precision is raised by
                           the digits of 1 / p.
  pvalue_quad_mp(t, df)    the same p as the incomplete beta integral I_x(df / 2, 1 / 2), x = df / (df + t^2), after the change of
                           variable u = x exp(-w / a), a = df / 2:
                               p = x^a / (a B(a, 1/2)) * integral_0^inf exp(-w) (1 - x exp(-w / a))^(-1/2) dw
                           -- the integrand is smooth on the scale max(1, t^2 / 2) whatever df is, where the density itself is a
                           spike of width 1 / a at u = x.  It shares nothing with the sums but x: Gamma functions and a
                           tanh-sinh rule here, rational recurrences and an arctangent there.

mpmath.betainc(..., regularized=True) is not used: it raised a convergence error at 60 digits on part of this grid."""
import mpmath as mp

DPS = 60
TINY = 1.0e-20      # scipy/stats/_stats_py.py, linregress


def regression_mp(t, y):
    """-> (r, t-statistic, 1 - r^2) as mp.mpf; r = 0 where a variance is 0 (scipy: `if ssxm == 0.0 or ssym == 0.0: r = 0.0`)."""
    with mp.workdps(DPS):
        t = [mp.mpf(float(v)) for v in t]
        y = [mp.mpf(float(v)) for v in y]
        n = len(y)
        tm, ym = mp.fsum(t) / n, mp.fsum(y) / n
        sxx = mp.fsum((a - tm) ** 2 for a in t)
        syy = mp.fsum((b - ym) ** 2 for b in y)
        sxy = mp.fsum((a - tm) * (b - ym) for a, b in zip(t, y))
        if sxx == 0 or syy == 0:
            return mp.mpf(0), mp.mpf(0), mp.mpf(1)
        r2 = sxy * sxy / (sxx * syy)
        return mp.sign(sxy) * mp.sqrt(r2), t_from_r2_mp(r2, int(mp.sign(sxy)), n - 2), 1 - r2


def t_from_r2_mp(r2, sign, df):
    """(1 - r + TINY)(1 + r + TINY) = 1 - r^2 + 2 TINY + TINY^2: no difference of r from 1 is ever formed."""
    with mp.workdps(DPS):
        r2, tiny = mp.mpf(r2), mp.mpf(TINY)
        return sign * mp.sqrt(r2 * df / (1 - r2 + 2 * tiny + tiny * tiny))


def pvalue_quad_mp(t, df, dps=30):
    with mp.workdps(dps + 10):
        t = mp.mpf(t)
        if t == 0:
            return mp.mpf(1)
        a = mp.mpf(df) / 2
        x = mp.mpf(df) / (df + t * t)
        scale = max(mp.mpf(1), t * t / 2)
        knots = [0] + [scale * k for k in (mp.mpf(1) / 4, 1, 4)] + [16, 64, 200]
        knots = sorted(set(k for k in knots if k <= 200))
        integral = mp.quad(lambda w: mp.exp(-w) / mp.sqrt(1 - x * mp.exp(-w / a)), knots)      # exp(-200) = 1e-87 is left out
        log_front = a * mp.log(x) - mp.log(a) - (mp.loggamma(a) + mp.loggamma(mp.mpf(1) / 2) - mp.loggamma(a + mp.mpf(1) / 2))
        return mp.exp(log_front) * integral


def pvalue_sum_mp(t, df, log10_p=0.0, dps=30):
    """log10_p: a rough log10 of the answer (pvalue_quad_mp's, or 0): the digits the cancellation of 1 - A costs."""
    with mp.workdps(dps + 20 + int(max(0.0, -log10_p))):
        t = abs(mp.mpf(t))
        if t == 0:
            return mp.mpf(1)
        df = int(df)
        c2 = mp.mpf(df) / (df + t * t)            # cos^2 theta, theta = atan(t / sqrt(df))
        s = t / mp.sqrt(df + t * t)                 # sin theta
        if df % 2 == 0:
            term = total = mp.mpf(1)
            for j in range(1, df // 2):
                term *= c2 * (2 * j - 1) / (2 * j)
                total += term
            return 1 - s * total
        theta = mp.atan(t / mp.sqrt(df))
        inner = mp.mpf(0)
        if df > 1:
            term = inner = mp.mpf(1)
            for j in range(1, (df - 3) // 2 + 1):
                term *= c2 * (2 * j) / (2 * j + 1)
                inner += term
            inner *= s * mp.sqrt(c2)
        return 1 - 2 * (theta + inner) / mp.pi
