"""TEST INFRASTRUCTURE: statsmodels' adfuller(autolag="AIC") and AutoReg(trend="c") evaluated in 60-digit arithmetic
(mpmath) on the float64 data -- "what the reference's algorithm returns when its SVD does not run out of digits".
Used to adjudicate between the kernels' double-double pass and the oracle's float64 SVD on ill-conditioned designs.
adfuller_aic_mp / autoreg_params_mp: full-rank designs only (a dependent column raises); the *_pinv_mp functions restate
statsmodels' pseudo-inverse rule and serve every design."""
import functools
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 60


def _ls(X, y):
    """-> (beta, ssr, (X^T X)^-1) by Cholesky of the normal equations in 60 digits."""
    n, p = len(X), len(X[0])
    G = mp.matrix(p, p)
    g = mp.matrix(p, 1)
    for a in range(p):
        for c in range(a + 1):
            G[a, c] = G[c, a] = mp.fsum(X[t][a] * X[t][c] for t in range(n))
        g[a] = mp.fsum(X[t][a] * y[t] for t in range(n))
    Ginv = G ** -1
    beta = Ginv * g
    ssr = mp.fsum((y[t] - mp.fsum(X[t][a] * beta[a] for a in range(p))) ** 2 for t in range(n))
    return beta, ssr, Ginv


def adfuller_aic_mp(x):
    x = [mp.mpf(float(v)) for v in x]
    n = len(x)
    maxlag = min(n // 2 - 2, int(math.ceil(12.0 * (n / 100.0) ** 0.25)))
    d = [x[i + 1] - x[i] for i in range(n - 1)]
    d = [mp.mpf(float(v)) for v in d]  # np.diff rounds to float64

    def design(lags, const_first):
        rows = range(lags, len(d))
        Z = [[x[t]] + [d[t - j] for j in range(1, lags + 1)] for t in rows]
        y = [d[t] for t in rows]
        cols = list(zip(*Z))
        has_const = any(all(v == c[0] for v in c) and c[0] != 0 for c in cols)
        if not has_const:
            Z = [([mp.mpf(1)] + r) if const_first else (r + [mp.mpf(1)]) for r in Z]
        return Z, y, (0 if has_const else 1)

    Z, y, hc = design(maxlag, True)
    startlag = hc + 1
    nobs = len(y)
    best = None
    for lag in range(startlag, startlag + maxlag + 1):
        _, ssr, _ = _ls([r[:lag] for r in Z], y)
        aic = nobs * mp.log(ssr / nobs) + nobs * (mp.log(2 * mp.pi) + 1) + 2 * lag
        if best is None or (aic, lag) < best:
            best = (aic, lag)
    usedlag = best[1] - startlag
    Z, y, hc = design(usedlag, False)
    beta, ssr, Ginv = _ls(Z, y)
    sigma2 = ssr / (len(y) - len(Z[0]))
    return float(beta[0] / mp.sqrt(sigma2 * Ginv[0, 0])), usedlag


def autoreg_params_mp(x, k):
    x = [mp.mpf(float(v)) for v in x]
    n = len(x)
    X = [[mp.mpf(1)] + [x[t - j] for j in range(1, k + 1)] for t in range(k, n)]
    beta, _, _ = _ls(X, [x[t] for t in range(k, n)])
    return np.array([float(b) for b in beta])


# ---------------------------------------------------------------------------------------------------------------------
# statsmodels' pinv semantics in many digits: singular values <= 1e-15 s_max dropped, rank = #{s > s_max p eps}
# ---------------------------------------------------------------------------------------------------------------------
def _gram_mp(cols, y):
    """-> (X^T X, X^T y, y^T y) of the design whose COLUMNS are `cols` (float64 data, current mpmath precision)."""
    cm = [[mp.mpf(float(v)) for v in c] for c in cols]
    ym = [mp.mpf(float(v)) for v in y]
    p = len(cm)
    G = mp.matrix(p, p)
    g = mp.matrix(p, 1)
    for a in range(p):
        for c in range(a + 1):
            G[a, c] = G[c, a] = mp.fdot(cm[a], cm[c])
        g[a] = mp.fdot(cm[a], ym)
    return G, g, mp.fdot(ym, ym)


def _zero_below():
    """What the working precision cannot tell from 0: a quantity that is exactly 0 comes out of `dps` digits as ~10^-dps
    (times the squared condition number of the Gram matrix, at most 1e32 for float64 data that is not exactly
    dependent); half the digits leave both a wide margin."""
    return mp.mpf(10) ** (-(mp.mp.dps // 2))


def _pinv_gram_mp(G, g, yy, p):
    """The pinv fit of the LEADING p columns of a design given by its Gram matrix (current mpmath precision).
    -> (beta, ssr, rank, diag of pinv(X) pinv(X)^T, s / s_max descending); ssr = y^T y - 2 beta^T X^T y + beta^T X^T X beta
    (exact for any beta), and an ssr the precision cannot tell from 0 is returned as the exact 0."""
    Gp, gp = G[:p, :p], g[:p, 0]
    lam, V = mp.eigsy(Gp)
    lmax = max(lam)
    if lmax <= 0:
        return [mp.mpf(0)] * p, yy, 0, [mp.mpf(0)] * p, [0.0] * p
    smax = mp.sqrt(lmax)
    eps = mp.mpf(2) ** -52
    beta = [mp.mpf(0)] * p
    cov = [mp.mpf(0)] * p
    rank = 0
    ratios = []
    for i in range(p):
        s = mp.sqrt(lam[i]) if lam[i] > 0 else mp.mpf(0)
        ratios.append(float(s / smax))
        if s > smax * p * eps:
            rank += 1
        if s > mp.mpf("1e-15") * smax:
            w = mp.fsum(V[a, i] * gp[a] for a in range(p)) / lam[i]
            for a in range(p):
                beta[a] += V[a, i] * w
                cov[a] += V[a, i] ** 2 / lam[i]
    bm = mp.matrix(beta)
    ssr = yy - 2 * mp.fdot(beta, list(gp)) + (bm.T * Gp * bm)[0]
    if ssr <= _zero_below() * yy:
        ssr = mp.mpf(0)
    return beta, ssr, rank, cov, sorted(ratios, reverse=True)


def pinv_ols_mp(X, y, dps=120):
    """OLS(y, X).fit(method="pinv") evaluated in `dps` digits from the eigen-decomposition of X^T X (the squared
    condition number needs the digits).  -> (beta, ssr, rank, cov00, s / s_max) as floats / float arrays."""
    old = mp.mp.dps
    mp.mp.dps = dps
    try:
        cols = [list(c) for c in zip(*X)]
        G, g, yy = _gram_mp(cols, y)
        beta, ssr, rank, cov, ratios = _pinv_gram_mp(G, g, yy, len(cols))
        return [float(v) for v in beta], float(ssr), rank, float(cov[0]), ratios
    finally:
        mp.mp.dps = old


def autoreg_params_pinv_mp(x, k):
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    rows = np.arange(k, n)
    X = np.column_stack([np.ones(n - k)] + [x[rows - j] for j in range(1, k + 1)])
    return pinv_ols_mp(X.tolist(), x[rows].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# adfuller with every lag selection, on the pinv fit above: oracle/third_party.py's restatement, digit for digit
# ---------------------------------------------------------------------------------------------------------------------
def _t_mp(beta_j, ssr, dof, cov_jj, scale):
    """beta_j / sqrt(ssr / dof * cov_jj) with the perfect fit's rule (tests/test_degenerate.py,
    test_perfect_fit_behaviour_is_pinned): the residual is the exact 0 it is, so t is x / 0 = +-inf or 0 / 0 = nan.
    scale: the size of a coefficient that counts (|y| / |column|), against which `beta_j` is 0 or not."""
    if ssr == 0 or dof <= 0 or cov_jj == 0:
        if abs(beta_j) <= _zero_below() * scale:
            return mp.nan
        return mp.inf if beta_j > 0 else -mp.inf
    return beta_j / mp.sqrt(ssr / dof * cov_jj)


def _relative_gap(a, b):
    if mp.isinf(a) or mp.isinf(b):
        return 0.0 if a == b else float("inf")
    return float(abs(a - b) / max(abs(a), abs(b), mp.mpf(1)))


@functools.lru_cache(maxsize=256)
def _lag_search_mp(xbytes, dps):
    """The nested fits of _autolag, shared by the three lag selections (call with mp.mp.dps == dps).
    -> (startlag, nobs, y^T y, [(lag, ssr, rank, t of the last coefficient, s / s_max)] for lag = startlag ..)"""
    from oracle.third_party import _add_const
    x = np.frombuffer(xbytes, dtype=np.float64)
    nobs = len(x)
    maxlag = min(nobs // 2 - 2, int(math.ceil(12.0 * (nobs / 100.0) ** 0.25)))
    d = np.diff(x)
    rows = np.arange(maxlag, len(d))
    Z = np.column_stack([x[rows]] + [d[rows - j] for j in range(1, maxlag + 1)])
    y = d[rows]
    full = _add_const(Z, prepend=True)
    startlag = full.shape[1] - Z.shape[1] + 1
    G, g, yy = _gram_mp(full.T, y)
    fits = []
    for lag in range(startlag, startlag + maxlag + 1):
        beta, ssr, rank, cov, ratios = _pinv_gram_mp(G, g, yy, lag)
        col = mp.sqrt(G[lag - 1, lag - 1])
        t = _t_mp(beta[-1], ssr, len(y) - rank, cov[-1], mp.sqrt(yy) / col if col > 0 else mp.mpf(1))
        fits.append((lag, ssr, rank, t, ratios))
    return startlag, len(y), yy, fits


def adfuller_pinv_mp(x, autolag="AIC", dps=120):
    """statsmodels' adfuller(x, autolag=autolag) with every regression solved by the many-digit pinv rule.
    -> (teststat, usedlag, facts); facts, for judging whether the case has ONE answer:
         "ratios": [s / s_max of every design that was solved: the nested lag-search fits, then the final regression]
         "best", "second": the two smallest criterion values ("AIC" / "BIC"; None otherwise)
         "gap": their relative distance, |second - best| / max(|.|, 1); "t-stat": the smallest relative distance of an
                examined |t| from the stop value, 0 where an examined t is 0 / 0 of a perfect fit of y != 0; inf where
                nothing is decided (None, or the first perfect fit wins)
         "perfect": a regression that decided the answer has ssr == 0 (the t value is then +-inf or nan)
    Criterion values that agree to half the working digits are the tie they are in exact arithmetic (an added column
    that depends on the earlier ones changes neither ssr nor rank): the smaller lag wins, as `(ic, lag) < best` does,
    and the gap is 0."""
    mode = None if autolag is None else str(autolag).lower()
    if mode not in (None, "aic", "bic", "t-stat"):
        raise ValueError("autolag must be one of 'AIC', 'BIC', 't-stat' or None")
    from oracle.third_party import ADF_TSTAT_STOP, _add_const
    x = np.asarray(x, dtype=np.float64)
    nobs = len(x)
    maxlag = min(nobs // 2 - 2, int(math.ceil(12.0 * (nobs / 100.0) ** 0.25)))
    if maxlag < 0:
        raise ValueError("sample size is too short to use selected regression component")
    d = np.diff(x)

    def design(lags):
        rows = np.arange(lags, len(d))
        return np.column_stack([x[rows]] + [d[rows - j] for j in range(1, lags + 1)]), d[rows]

    old = mp.mp.dps
    mp.mp.dps = dps
    try:
        facts = {"ratios": [], "best": None, "second": None, "gap": float("inf"), "perfect": False}
        if mode is None:
            usedlag = maxlag
        else:
            startlag, n1, yy, fits = _lag_search_mp(x.tobytes(), dps)
            if mode == "t-stat":
                for lag, ssr, rank, t, ratios in reversed(fits):
                    facts["ratios"].append(ratios)
                    bestlag = lag
                    if ssr == 0:
                        facts["perfect"] = True
                        if mp.isnan(t) and yy != 0:
                            # 0 / 0 with a last coefficient that is 0 only in exact arithmetic: whether the search stops
                            # here hangs on a quantity every finite precision returns as round-off (x / 0 = inf stops);
                            # with y = 0 every product is an exact 0 in any arithmetic
                            facts["gap"] = 0.0
                    elif not mp.isnan(t):
                        facts["gap"] = min(facts["gap"], float(abs(abs(t) - ADF_TSTAT_STOP) / ADF_TSTAT_STOP))
                    if not mp.isnan(t) and abs(t) >= ADF_TSTAT_STOP:
                        break
            else:
                ics = []
                for lag, ssr, rank, _, ratios in fits:
                    facts["ratios"].append(ratios)
                    pen = 2 if mode == "aic" else mp.log(n1)
                    ic = -mp.inf if ssr == 0 else n1 * mp.log(2 * mp.pi) + n1 * mp.log(ssr / n1) + n1 + pen * rank
                    ics.append((ic, lag))
                best = min(ics)
                for ic, lag in ics:      # a tie to half the digits is a tie: the first lag of it
                    if _relative_gap(ic, best[0]) <= float(_zero_below()):
                        best = (ic, lag)
                        break
                rest = sorted(v for v in ics if v[1] != best[1])
                bestlag = best[1]
                facts["best"] = float(best[0])
                facts["second"] = float(rest[0][0]) if rest else None
                if mp.isinf(best[0]):
                    facts["perfect"] = True      # the first perfect lag wins whatever follows
                elif rest:
                    gap = _relative_gap(rest[0][0], best[0])
                    facts["gap"] = 0.0 if gap <= float(_zero_below()) else gap
            usedlag = bestlag - startlag
        Z, y = design(usedlag)
        X = _add_const(Z[:, :usedlag + 1], prepend=False)
        G, g, yy = _gram_mp(X.T, y)
        beta, ssr, rank, cov, ratios = _pinv_gram_mp(G, g, yy, X.shape[1])
        facts["ratios"].append(ratios)
        if ssr == 0:
            facts["perfect"] = True
        col = mp.sqrt(G[0, 0])
        t = _t_mp(beta[0], ssr, len(y) - rank, cov[0], mp.sqrt(yy) / col if col > 0 else mp.mpf(1))
        return float(t), int(usedlag), facts
    finally:
        mp.mp.dps = old


def adf_pvalue(teststat):
    """The oracle's MacKinnon function of a many-digit test statistic (there is no second implementation of it)."""
    from oracle.third_party import mackinnonp_c
    return float("nan") if math.isnan(teststat) else float(mackinnonp_c(teststat))
