"""Truth, inputs and bars for every rfft route of k_spectral (fam_spectral.h), shared by tests/test_spectral_routes_emul.py
(the g++ build of the kernel sources) and tests/test_spectral_routes_gpu.py (the HIP kernels).

fam_spectral.h computes the full-length rfft behind fft_coefficient and fft_aggregated by five algorithms, chosen by length
alone (route_of below restates the choice).  tests/parity.py compares them with numpy's FFT under a floor of
1e-10 sum|x|, which for 1000 samples near 2^30 is 100 on bins of about 30 -- and numpy's own FFT is as noisy there as a
route that does not centre its input, so parity cannot see such a route.  Here every bin is compared with the EXACT DFT:

  * EXACT SHIFTS (the idea of tests/shift_cases.py).  base lies on a dyadic grid and is small, a level L is a multiple of
    the grid, so x = L + base and x - L == base hold without rounding in the dtype the device reads (asserted).  Bins
    k >= 1 of x are then those of base, bin 0 is sum(x).
  * dft_bins: direct summation in np.longdouble with the phase index reduced in integers.
  * a bar per route, derived below (none of them is read off the kernel), in terms of S_c = sum|x - mean(x)|, which does not
    move with the level: that the error of a centred route stays inside the same bar at every level IS its level invariance.

No input of this grid is skipped and there is no exclusion predicate."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
# This module needs a longdouble that is wider than double: x87 extended precision (64-bit significand, eps = 2^-63 =
# 1.08e-19, what np.finfo(np.longdouble) reports on x86-64 Linux, where this suite runs) or better.  A sum of n <= 65 536
# terms rounded to 2^-64 relative each, added pairwise (np.sum), is good to about 17 * 2^-64 S_c = 9e-19 S_c, and at the
# very worst (n 2^-64 S_c = 3.6e-15 S_c) to 1/28 of the tightest bar below (1e-13 S_c).
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than double here: the truth would be as noisy as the kernel"

EPS = 2.0 ** -53
TWO_PI = 8 * np.arctan(LD(1))


def dft_bins(x, ks):
    """X_k = sum_j x_j exp(-2 pi i j k / n) for the bins `ks` of a float32 / float64 series, by direct summation in
    np.longdouble (eps = 2^-63 on this suite's hosts: asserted at import).  The phase index j k is reduced modulo n in
    integers, so no argument of cos / sin exceeds one turn.  O(n) per bin.  -> (real, imag) longdouble arrays."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64) and x.ndim == 1
    n = len(x)
    xl = x.astype(LD)
    j = np.arange(n, dtype=np.int64)
    re, im = np.empty(len(ks), dtype=LD), np.empty(len(ks), dtype=LD)
    for i, k in enumerate(ks):
        assert 0 <= int(k) <= n // 2
        ph = ((j * int(k)) % n).astype(LD) * (TWO_PI / LD(n))
        re[i] = np.sum(xl * np.cos(ph))
        im[i] = -np.sum(xl * np.sin(ph))
        if k == 0 or 2 * int(k) == n:
            im[i] = 0   # (sin of a multiple of pi: exactly zero in the DFT, 1e-19-small here)
    return re, im


# ---- routes ------------------------------------------------------------------------------------------------------------
GOERTZEL_MIN, BLUESTEIN_MIN_ODD, BLUESTEIN_MIN_EVEN = 257, 1281, 897   # fam_spectral.h / tsfa_specs.h
MODES = ("default", "bluestein_off", "bluestein_min_257")
# the plan options of a mode (tests/engines.py: hip_engine) and the emulation's twins (tests/emul/emul.cpp)
MODE_OPTIONS = {"default": {}, "bluestein_off": {"bluestein": 0}, "bluestein_min_257": {"bluestein_min": 257}}
MODE_ENV = {"default": {}, "bluestein_off": {"TSFA_EMUL_BLUESTEIN": "0"}, "bluestein_min_257": {"TSFA_EMUL_BLUESTEIN_MIN": "257"}}


def route_of(n, mode="default"):
    """The algorithm fam_spectral_series picks for n samples: restated from its conditions, not asked of the kernel."""
    assert mode in MODES
    if n >= 4 and n & (n - 1) == 0 and n <= 65536:
        return "radix2"
    if n <= 256:
        return "direct"
    if n > 32768:
        return "reinsch"
    lo = 257 if mode == "bluestein_min_257" else (BLUESTEIN_MIN_ODD if n & 1 else BLUESTEIN_MIN_EVEN)
    return "chirpz" if (mode != "bluestein_off" and n >= lo) else "goertzel"


# the smallest lengths on both sides of every decision in the code
LENGTHS = {
    "lds": (3, 5, 6, 7, 100, 255,                                  # direct
            4, 8, 16, 256, 512, 1024, 2048, 4096, 8192,            # radix-2: a single first stage and none
            257, 258, 895, 896, 897, 1279, 1280,                   # Goertzel, up to both crossovers
            898, 1281, 1282, 2053, 4098, 8197),                    # chirp-z: even with M / T = 2 and 4, odd with 4 and 8
    "long": (16384, 12001, 32766, 32767,                           # the long-series build: radix-2, chirp-z
             32768, 65536,                                         # radix-2 at the twiddle table's end
             32769, 32770),                                        # Reinsch
}
LEVELS = {"float64": (0.0, 1024.0, -393216.0, 2.0 ** 24, 2.0 ** 30), "float32": (0.0, 1024.0, -98304.0)}
# the grid on which L + base is exact: |x| < 2^31 has ulp 2^-22 in float64, |x| < 2^17 has 2^-7 in float32
GRID = {"float64": 2.0 ** -20, "float32": 2.0 ** -6}
LIMIT = 8.0
KINDS = ("iid", "walk")
BINS = (0, 1, 2, 3, 7, 50, 99)   # and n/2 - 1, n/2 of every length


def base_series(kind, n, dtype_name):
    """Seeded N(0, 1), or a random walk scaled to unit spread, rounded to the dtype's grid."""
    rng = np.random.default_rng([20261020, KINDS.index(kind), n])
    e = rng.standard_normal(n)
    if kind == "walk":
        w = np.cumsum(e)
        e = (w - w.mean()) / max(float(w.std()), 1e-300)
    grid = GRID[dtype_name]
    b = np.round(e / grid) * grid
    assert np.max(np.abs(b)) < LIMIT
    return b


class Case:
    """One series x = level + base (exactly), its exact bins and its scales."""

    def __init__(self, kind, n, dtype_name, level):
        self.kind, self.n, self.dtype_name, self.level = kind, int(n), dtype_name, float(level)
        dt = np.dtype(dtype_name)
        self.b = base_series(kind, n, dtype_name)
        self.x = (self.level + self.b).astype(dt)
        assert np.array_equal(self.x.astype(np.float64), self.level + self.b)
        assert np.array_equal((self.x - dt.type(self.level)).astype(np.float64), self.b)   # x - L == base, in the dtype
        xl = self.x.astype(LD)
        mean = np.sum(xl) / LD(n)
        # the sum of x exactly (n 2^30 on a grid of 2^-20 has more than the 64 bits of a longdouble): integers on the grid
        sum_b = int(np.sum(np.round(self.b / GRID[dtype_name]).astype(np.int64)))   # < 2^39
        self.sum_exact = Fraction(self.level) * n + Fraction(sum_b) * Fraction(GRID[dtype_name])
        self.sum_x = LD(self.level * n) + LD(sum_b * GRID[dtype_name])    # (both parts exact in float64, one rounding to 2^-64)
        assert Fraction(self.level * n) == Fraction(self.level) * n
        self.S = float(np.sum(np.abs(xl)))
        self.S_c = float(np.sum(np.abs(xl - mean)))
        self.amax = float(np.max(np.abs(xl - mean)))
        self.bins = sorted({k for k in BINS + (n // 2 - 1, n // 2) if 0 <= k <= n // 2})
        self._truth = None
        self._spectrum = None

    @property
    def label(self):
        return "%s_%d_%s_%+g" % (self.kind, self.n, self.dtype_name, self.level)

    def truth(self):
        """{k: (real, imag)} longdouble: bins >= 1 from base (the shift is exact), bin 0 the sum of x."""
        if self._truth is None:
            re, im = _base_bins(self.kind, self.n, self.dtype_name, tuple(k for k in self.bins if k >= 1))
            self._truth = {k: (re[i], im[i]) for i, k in enumerate(k for k in self.bins if k >= 1)}
            self._truth[0] = (self.sum_x, LD(0))
        return self._truth

    def spectrum(self):
        """|X_k| of every bin from ONE np.fft.rfft(base), bin 0 restored (float64: numpy's FFT of the centred, small base is
        good to about log2(n) eps S_c per bin, a thousandth of the tightest bar)."""
        if self._spectrum is None:
            a = np.abs(np.fft.rfft(self.b)).astype(LD)
            a[0] = abs(self.sum_x)
            self._spectrum = a
        return self._spectrum


_bins_cache = {}


def _base_bins(kind, n, dtype_name, ks):
    key = (kind, n, dtype_name, ks)
    if key not in _bins_cache:
        _bins_cache[key] = dft_bins(base_series(kind, n, dtype_name), ks)   # (every level of a base shares them)
    return _bins_cache[key]


_batches = {}


def batch(dtype_name, build):
    """The ragged batch of (dtype, build): every length of LENGTHS[build] at every level of the dtype, N(0,1) and the walk
    alternating over (length, level) so that each length sees both and the batch stays small.  Built once per session."""
    key = (dtype_name, build)
    if key not in _batches:
        _batches[key] = [Case(KINDS[(i + j) % 2], n, dtype_name, level)
                         for i, n in enumerate(LENGTHS[build]) for j, level in enumerate(LEVELS[dtype_name])]
    return _batches[key]


def pack(cases, dtype):
    values = np.concatenate([c.x.astype(dtype) for c in cases])
    offsets = np.concatenate([[0], np.cumsum([c.n for c in cases])]).astype(np.int64)
    return values, offsets


def params(cases):
    """fft_coefficient real / imag / abs of every bin some series of the batch is asked for (a series shorter than a bin
    must answer NaN) and the four fft_aggregated columns."""
    ks = sorted({k for c in cases for k in c.bins})
    return {"fft_coefficient": [{"attr": a, "coeff": k} for a in ("real", "imag", "abs") for k in ks],
            "fft_aggregated": [{"aggtype": t} for t in ("centroid", "variance", "skew", "kurtosis")]}


# ---- bars: |error| of a bin (real, imag and abs alike: each is bounded by the modulus of the complex error) ------------------
def bar_direct(c, k):
    """Direct DFT of x - mean, X_k = sum_j (x_j - c) w_jk with |w| = 1 from a float64 table.

    The standard bound of an n-term inner product summed in any order is gamma_n sum|x_j - c| |w_jk| <= n eps S_c (Higham,
    Accuracy and Stability, 3.1); the subtraction x_j - c (1 eps), the two real products of a complex twiddle (1 eps) and
    the table entry itself (sincospi: 2 eps) and the second-order terms add at most 8 eps S_c: (n + 8) eps S_c.  Bin 0 is
    that sum plus n c: its bar is the same expression in S = sum|x| (|n c| <= S, one product and one addition)."""
    return (c.n + 8) * EPS * (c.S if k == 0 else c.S_c)


def bar_radix2(c, k):
    """Radix-2 Cooley-Tukey on x itself: log2(n) stages, each multiplying by a float64 twiddle (table value 1 eps, complex
    product and butterfly sum < 4 eps with the second-order terms: mu <= 8 eps per stage to keep it simple), the error
    of a bin <= log2(n) mu sum|x| (Higham 24.2 in its 1-norm form: every output is a sum over all inputs with unit-modulus
    weights, each input passes log2(n) roundings).  8 log2(n) eps S.  LEVEL-PROPORTIONAL BY DESIGN: the transform runs on
    x, not on x - mean; centring it would change the bits of the headline path (the benchmark's 1024-sample series) and
    is out of scope, so this bar is in S, not S_c, and says nothing about level invariance."""
    return 8.0 * np.log2(c.n) * EPS * c.S


def bar_chirpz(c, k):
    """The project's device bar for this route (test_chirp_z_transform_on_every_tile_shape_and_in_several_launches:
    1e-13 sum|x|), with the centred scale in its place: three FFTs of up to 65 536 points on x - mean.  Bin 0: + n c."""
    return 1e-13 * (c.S if k == 0 else c.S_c)


def sweep_law(c, k):
    """eps n^2 / (2 pi k') max|x - mean|, k' = min(k, n/2 - k) clamped to 1: the kernel's own law for the Goertzel recurrence
    (the comment above its Reinsch branch said "eps n^2 / (2 pi k)"): each of the n steps rounds a state of size up to
    max|x| / |sin th|, 1 / |sin th| ~ n / (2 pi k').  It is a scale, not a bound: its constant is not known a priori and is
    measured on the restatements below (RESTATEMENT_WORST), never on the kernel."""
    kp = max(min(k, c.n / 2.0 - k), 1.0)
    return EPS * c.n * c.n / (2.0 * np.pi * kp) * c.amax


# Worst error / sweep_law of the float64 numpy restatements below (centred input, np.mean), over every case of batch() that
# can reach the route in some mode (both dtypes, every level), measured on the CPU by `python tests/spectral_truth.py`
# (profiles/spectral_route_accuracy.md holds the output).  The kernel may take 4 x that: it differs from the restatement
# only in how the mean is summed.  Over the whole grid the figure is 1.13e3 for the bins >= 1 of the Goertzel sweep (at
# 32 766 samples) and 2.1e3 for its bin 0 (th = 0 makes the recurrence a double prefix sum; 12 001 samples), 0.0293 and
# 0.0866 for Reinsch's form.  The law is not Goertzel's law at the bins next to 0 and n/2 (there the loss is eps n / th^2,
# n / (2 pi k') times the law: the comment above the Reinsch branch), so the figure grows with n, and ONE figure would
# leave 257 samples a hundred times the room they need.  It is therefore held PER LENGTH, and apart for bin 0:
# {n: (bins >= 1, bin 0)}, which asks more of every length but the worst.
RESTATEMENT_WORST = {
    "goertzel": {257: (10.5, 26.8), 258: (15.3, 59.4), 895: (98.7, 299.0), 896: (35.0, 30.8), 897: (65.8, 168.0), 898: (51.4, 211.0),
                 1279: (21.4, 57.4), 1280: (41.2, 150.0), 1281: (28.9, 90.5), 1282: (63.1, 167.0), 2053: (203.0, 366.0),
                 4098: (127.0, 793.0), 8197: (257.0, 874.0), 12001: (1.06e3, 2.1e3), 32766: (1.13e3, 760.0), 32767: (957.0, 284.0)},
    "reinsch": {32769: (0.0293, 0.0866), 32770: (0.0152, 0.0397)},
}
SWEEP_ALLOWANCE = 4.0


def _bar_sweep(route, c, k):
    """SWEEP_ALLOWANCE x RESTATEMENT_WORST[length] x the law.  Bin 0 is the swept sum of x - c PLUS n c (c: the rounded
    strided mean; any constant serves, so its own error cancels): the product n c and the final addition round once each,
    on values of at most sum|x| + the sweep's part: 4 eps S more."""
    bar = SWEEP_ALLOWANCE * RESTATEMENT_WORST[route][c.n][1 if k == 0 else 0] * sweep_law(c, k)
    return bar + (4.0 * EPS * c.S if k == 0 else 0.0)


def bar_goertzel(c, k):
    return _bar_sweep("goertzel", c, k)


def bar_reinsch(c, k):
    return _bar_sweep("reinsch", c, k)


BAR = {"direct": bar_direct, "radix2": bar_radix2, "chirpz": bar_chirpz, "goertzel": bar_goertzel, "reinsch": bar_reinsch}


# ---- float64 restatements of the two recurrences (from the formulas in the comments of blk_rfft) ---------------------------
def goertzel_restated(x, ks, add_back=True):
    """s_j = x_j + 2 cos(th) s_{j-1} - s_{j-2}, X_k = s_{n-1} e^{i th} - s_{n-2}, th = 2 pi k / n, on x - mean; bin 0: + n mean
    (add_back=False: without, the transform of x - mean alone)."""
    x = np.asarray(x, dtype=np.float64)
    n, mean = len(x), float(np.mean(x))
    ks = np.asarray(ks, dtype=np.float64)
    th = 2.0 * np.pi * ks / n
    c2, s1, s2 = 2.0 * np.cos(th), np.zeros(len(ks)), np.zeros(len(ks))
    for v in (x - mean):
        s1, s2 = (v + c2 * s1) - s2, s1
    re = s1 * np.cos(th) - s2 + np.where(ks == 0, n * mean if add_back else 0.0, 0.0)
    return re, np.where((ks == 0) | (2 * ks == n), 0.0, s1 * np.sin(th))


def reinsch_restated(x, ks, add_back=True):
    """Reinsch's form: cos(th) >= 0: d_j = x_j - 4 sin^2(th/2) s_{j-1} + d_{j-1}, s_j = s_{j-1} + d_j;
    cos(th) < 0: d_j = x_j + 4 cos^2(th/2) s_{j-1} - d_{j-1}, s_j = d_j - s_{j-1}; X_k = s (cos th -+ 1) +- d + i s sin th."""
    x = np.asarray(x, dtype=np.float64)
    n, mean = len(x), float(np.mean(x))
    ks = np.asarray(ks, dtype=np.float64)
    th = 2.0 * np.pi * ks / n
    pos = np.cos(th) >= 0.0
    kap = np.where(pos, -4.0 * np.sin(th / 2) ** 2, 4.0 * np.cos(th / 2) ** 2)
    sg = np.where(pos, 1.0, -1.0)
    s, d = np.zeros(len(ks)), np.zeros(len(ks))
    for v in (x - mean):
        d = (v + kap * s) + sg * d
        s = sg * s + d
    re = 0.5 * kap * s + sg * d + np.where(ks == 0, n * mean if add_back else 0.0, 0.0)
    return re, np.where((ks == 0) | (2 * ks == n), 0.0, s * np.sin(th))


RESTATED = {"goertzel": goertzel_restated, "reinsch": reinsch_restated}


def restatement_ratio(route, c):
    """(worst |error| / sweep_law over the bins >= 1 of one case, the same for bin 0).  Bin 0 is taken WITHOUT its n mean
    part (whose rounding is the level's, 4 eps S in the bar, not the sweep's): the swept sum of x - mean against
    sum(x) - n mean in exact rational arithmetic."""
    ks = list(c.bins)
    x = c.x.astype(np.float64)
    re, im = RESTATED[route](x, ks, add_back=False)
    t = dict(c.truth())
    t[0] = (LD(float(c.sum_exact - c.n * Fraction(float(np.mean(x))))), LD(0))
    r = [max(abs(float(LD(re[i]) - t[k][0])), abs(float(LD(im[i]) - t[k][1]))) / sweep_law(c, k) for i, k in enumerate(ks)]
    assert ks[0] == 0
    return max(r[1:]), r[0]


def measure_restatements():
    """-> {route: {n: (bins >= 1, bin 0)}} over every case of batch() that can reach the route in some mode."""
    out = {}
    for route in ("goertzel", "reinsch"):
        w = out.setdefault(route, {})
        for dtype_name in ("float64", "float32"):
            for build in ("lds", "long"):
                for c in batch(dtype_name, build):
                    if route in {route_of(c.n, m) for m in MODES}:
                        a, b = restatement_ratio(route, c)
                        w[c.n] = (max(w.get(c.n, (0.0, 0.0))[0], a), max(w.get(c.n, (0.0, 0.0))[1], b))
    return out


# ---- fft_aggregated ----------------------------------------------------------------------------------------------------
def aggregated_truth_and_tolerance(c, route):
    """-> {aggtype: (truth, tolerance, variance)}: the moments of the true |X_k| over the bin index k (fc.py:1123) in
    longdouble, and the route's per-bin bar delta_k propagated to first order.

    With a_k = |X_k|, s_p = sum_k k^p a_k and m_p = s_p / s_0:  d m_p / d a_k = (k^p - m_p) / s_0.  For a column
    f(m_1 .. m_4), |delta f| <= sum_k |sum_p (df / dm_p) (k^p - m_p)| delta_k / s_0, where
        centroid  f = m_1
        variance  f = m_2 - m_1^2                           df/dm_1 = -2 m_1, df/dm_2 = 1
        skew      f = N v^-1.5, N = m_3 - 3 m_1 m_2 + 2 m_1^3    dN = (-3 m_2 + 6 m_1^2, -3 m_1, 1, 0),  v = variance
        kurtosis  f = K v^-2,   K = m_4 - 4 m_1 m_3 + 6 m_2 m_1^2 - 3 m_1 (the reference's own formula, fc.py:1123)
                                                            dK = (-4 m_3 + 12 m_1 m_2 - 3, 6 m_1^2, -4 m_1, 1)
    and df = dN v^-1.5 - 1.5 N v^-2.5 dv,  df = dK v^-2 - 2 K v^-3 dv.

    To that comes what ANY float64 evaluation of these formulas costs, whatever the bins: each s_p is a sum of nf = n/2 + 1
    positive terms (hypot, k^p, the product: 4 eps; the sum in any order: nf eps relative, Higham 4.2), so m_p = s_p / s_0
    is good to 2 (nf + 8) eps m_p, and the monomials of f in the m_p carry that through: sum_p |df / dm_p| m_p 2 (nf + 8) eps
    (the handful of roundings of the closing arithmetic are relative errors of those same monomials, inside the + 8).
    The emulation adds the bins in sequence, the device in a tree; the term is the worst case of either."""
    a = c.spectrum()
    k = np.arange(len(a), dtype=LD)
    delta = np.array([BAR[route](c, int(kk)) for kk in (0, 1)], dtype=LD)   # (bars depend on k through bin 0 alone ...
    dk = np.full(len(a), delta[1], dtype=LD)
    if route in ("goertzel", "reinsch"):                                   #  ... but for the sweeps' law)
        dk = np.array([BAR[route](c, int(kk)) for kk in range(len(a))], dtype=LD)
    dk[0] = delta[0]
    s0 = np.sum(a)
    m = [None] + [np.sum(k ** p * a) / s0 for p in (1, 2, 3, 4)]
    v = m[2] - m[1] * m[1]
    dv = (-2 * m[1], LD(1), LD(0), LD(0))
    N = m[3] - 3 * m[1] * m[2] + 2 * m[1] ** 3
    dN = (-3 * m[2] + 6 * m[1] ** 2, -3 * m[1], LD(1), LD(0))
    K = m[4] - 4 * m[1] * m[3] + 6 * m[2] * m[1] ** 2 - 3 * m[1]
    dK = (-4 * m[3] + 12 * m[1] * m[2] - 3, 6 * m[1] ** 2, -4 * m[1], LD(1))

    u_eval = 2.0 * (len(a) + 8) * EPS

    def tol(df):
        g = sum(df[p - 1] * (k ** p - m[p]) for p in (1, 2, 3, 4))
        return float(np.sum(np.abs(g) * dk) / s0 + sum(abs(df[p - 1]) * m[p] for p in (1, 2, 3, 4)) * u_eval)
    out = {"centroid": (float(m[1]), tol((LD(1), LD(0), LD(0), LD(0))), float(v)), "variance": (float(v), tol(dv), float(v))}
    if v > 0:
        out["skew"] = (float(N / v ** LD(1.5)), tol(tuple(dN[i] / v ** LD(1.5) - LD(1.5) * N / v ** LD(2.5) * dv[i] for i in range(4))), float(v))
        out["kurtosis"] = (float(K / (v * v)), tol(tuple(dK[i] / (v * v) - 2 * K / v ** 3 * dv[i] for i in range(4))), float(v))
    else:
        out["skew"] = out["kurtosis"] = (float("nan"), 0.0, float(v))
    return out


# ---- the comparison ----------------------------------------------------------------------------------------------------
def check(names, got, cases, mode, worst=None, what="x"):
    """got: [len(cases), len(names)] of params(cases).  -> list of mismatches.  worst, a dict, receives
    {(route, level, "bins" | "aggregated"): largest error / bar}."""
    bad = []
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (len(cases), len(names)), got.shape
    cols = []
    for nm in names:
        if "fft_coefficient" in nm:
            cols.append(("bin", nm.split('attr_"')[1].split('"')[0], int(nm.split("coeff_")[1].split("__")[0])))
        else:
            cols.append(("agg", nm.split('aggtype_"')[1].split('"')[0], None))
    for i, c in enumerate(cases):
        route = route_of(c.n, mode)
        t = c.truth()
        agg = aggregated_truth_and_tolerance(c, route)
        for j, (what_col, attr, k) in enumerate(cols):
            g = got[i, j]
            where = "%s(%s, %s, %s) %s" % (what, c.label, mode, route, names[j])
            if what_col == "bin":
                if k > c.n // 2:
                    if not np.isnan(g):
                        bad.append("%s: got %r for a bin beyond n/2" % (where, g))
                    continue
                if k not in t:
                    continue   # (a bin asked for another length's sake)
                re, im = t[k]
                want = {"real": re, "imag": im, "abs": np.sqrt(re * re + im * im)}[attr]
                err, bar = abs(float(LD(g) - want)), BAR[route](c, k)
                key = (route, c.level, "bins")
            else:
                want, bar, var = agg[attr]
                if attr in ("skew", "kurtosis") and np.isnan(g):
                    # the kernel (like the reference) returns NaN where its variance is below 0.5
                    if not var < 0.5 + agg["variance"][1]:
                        bad.append("%s: got NaN at a true variance of %r" % (where, var))
                    continue
                err = abs(g - want)
                key = (route, c.level, "aggregated")
            if worst is not None and bar > 0:
                worst[key] = max(worst.get(key, 0.0), err / bar)
            if not err <= bar:
                bad.append("%s: got %r want %r, error %.3g = %.3g x the bar" % (where, g, float(want), err, err / bar if bar > 0 else np.inf))
    return bad


def reference_worst(cases, mode, worst):
    """np.fft.rfft(x) itself under the same bars (profiles/spectral_route_accuracy.md: what parity compares against)."""
    for c in cases:
        route, t = route_of(c.n, mode), c.truth()
        X = np.fft.rfft(c.x.astype(np.float64))
        for k in c.bins:
            err = max(abs(float(LD(X[k].real) - t[k][0])), abs(float(LD(X[k].imag) - t[k][1])))
            key = (route, c.level, "bins")
            worst[key] = max(worst.get(key, 0.0), err / BAR[route](c, k))


def worst_table(worsts, headers):
    """worsts: list of dicts of check().  -> markdown rows: route, level, one 'bins / aggregated' cell per dict."""
    keys = sorted({(r, lv) for w in worsts for (r, lv, _) in w}, key=lambda rl: (rl[0], abs(rl[1])))
    out = ["| route | level | " + " | ".join(headers) + " |", "|---|---|" + "---|" * len(headers)]
    for r, lv in keys:
        cells = ["%s / %s" % tuple("%.2g" % w[(r, lv, part)] if (r, lv, part) in w else "-" for part in ("bins", "aggregated")) for w in worsts]
        out.append("| %s | %+g | %s |" % (r, lv, " | ".join(cells)))
    return "\n".join(out)


# ---- Welch -------------------------------------------------------------------------------------------------------------
WELCH_LENGTHS = (3, 7, 100, 255, 256, 257, 384, 1000)   # blk_rfft's routes below 256, the batched 128-point path from 256 on
WELCH_LEVELS = {"float64": (0.0, 2.0 ** 24), "float32": (0.0, -98304.0)}   # (float32 has no grid at 2^24: its highest level)
WELCH_BINS = (2, 5, 8)
WELCH_PARAMS = {"spkt_welch_density": [{"coeff": k} for k in WELCH_BINS]}


def welch_cases(dtype_name="float64"):
    """Each length at both levels with the SAME base (N(0,1) and the walk alternate over the lengths)."""
    return [Case(KINDS[i % 2], n, dtype_name, level) for i, n in enumerate(WELCH_LENGTHS) for level in WELCH_LEVELS[dtype_name]]


def welch_reference(series):
    from scipy.signal import welch
    return welch(np.asarray(series, dtype=np.float64), nperseg=min(len(series), 256))[1]


def check_welch(names, got, cases, what="x", worst=None):
    """spkt_welch_density against scipy.signal.welch on the exactly centred base: the constant detrend makes the density
    level-free, so one truth serves every level.  Bar: 1e-12 relative + 1e-13 max(pxx)."""
    bad = []
    for i, c in enumerate(cases):
        pxx = welch_reference(c.b)
        for j, nm in enumerate(names):
            k = int(nm.split("coeff_")[1].split("__")[0])
            g = got[i][j]
            if k >= len(pxx):
                if not np.isnan(g):
                    bad.append("%s(%s) %s: got %r beyond the last bin" % (what, c.label, nm, g))
                continue
            bar = 1e-12 * abs(pxx[k]) + 1e-13 * float(np.max(pxx))
            err = abs(g - pxx[k])
            if worst is not None:
                worst[c.level] = max(worst.get(c.level, 0.0), err / bar)
            if not err <= bar:
                bad.append("%s(%s) %s: got %r want %r, error %.3g = %.3g x the bar" % (what, c.label, nm, g, pxx[k], err, err / bar))
    return bad


if __name__ == "__main__":
    # the measured constants of the sweep bars: worst error / law of the restatements over the grid
    for route, w in measure_restatements().items():
        print(route, "worst over the grid: bins >= 1 %.4g, bin 0 %.4g" % (max(v[0] for v in w.values()), max(v[1] for v in w.values())))
        print("    {" + ", ".join("%d: (%.3g, %.3g)" % (n, w[n][0], w[n][1]) for n in sorted(w)) + "}")
