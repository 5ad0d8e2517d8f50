"""Exact arithmetic for the moment and determinant kernels -- TEST INFRASTRUCTURE ONLY.

float32 frames are exact rationals.  Scaled by one power of two they are Python integers, so the
sums the statistics records hold (n, sum x_i, sum x_i x_j) are exact integers, and so is

    A = n M - s s^T        (cov = A / (n (n - 1)) / 4^k  for frames = integers / 2^k).

det A comes from fraction-free (Bareiss) elimination in integers; logarithms, the (n (n - 1))^39
and scaling terms, the assembly of BIC / GLR (change_detection.bic_from_terms / glr_from_terms)
and KL2 (numpy_engine.kl2_frames, with exact means) are done in mpmath at MP_BITS bits.  No
floating-point rounding enters before the final conversion to a double (or a (hi, lo) pair of
doubles), so the values are the truth every floating-point formulation is measured against.
"""
import math

import mpmath
import numpy as np

DIM = 39
MP_BITS = 256           # logs and assembly (>= 200)
MP_BITS_INV = 448       # inverses for KL2 (>= 400)
_LIMB = 20              # bits per limb of the int64 products: 2^40 per product, 2^12 rows per block
_ROWS = 4096


class Moments(object):
    """n, s[i] = sum x_i, m[i][j] = sum x_i x_j of integer frames x = frames * 2^k."""
    __slots__ = ('n', 's', 'm', 'k')

    def __init__(self, n, s, m, k):
        self.n, self.s, self.m, self.k = n, s, m, k

    def __add__(self, o):
        assert self.k == o.k
        d = len(self.s)
        return Moments(self.n + o.n, [a + b for a, b in zip(self.s, o.s)],
                       [[self.m[i][j] + o.m[i][j] for j in range(d)] for i in range(d)], self.k)

    def scatter(self):
        """A = n M - s s^T (integers)."""
        d = len(self.s)
        return [[self.n * self.m[i][j] - self.s[i] * self.s[j] for j in range(d)] for i in range(d)]


class ExactFrames(object):
    """The frames of one buffer as integers: frames[t, j] = x[t][j] / 2^k exactly."""

    def __init__(self, frames):
        f = np.ascontiguousarray(frames, dtype=np.float32)
        assert f.ndim == 2 and np.isfinite(f).all()
        mant, exp = np.frexp(f.astype(np.float64))
        mi = np.round(mant * 16777216.0).astype(np.int64)            # 24-bit mantissas: exact
        assert np.array_equal(mi.astype(np.float64) * 2.0 ** -24, mant)
        e = exp.astype(np.int64) - 24
        # drop trailing zero bits so that small integers stay small
        nz = mi != 0
        tz = np.zeros_like(mi)
        low = np.where(nz, mi & -mi, 1)
        tz[nz] = np.round(np.log2(low[nz].astype(np.float64))).astype(np.int64)
        mi = np.where(nz, mi >> tz, 0)
        e = e + tz
        emin = int(e[nz].min()) if nz.any() else 0
        self.k = -emin
        sh = np.where(nz, e - emin, 0)
        self.shape = f.shape
        self.bits = int((np.where(nz, np.floor(np.log2(np.abs(mi).astype(np.float64) + (~nz))) + 1, 0) + sh).max())
        # signed limbs of _LIMB bits, least significant first, as int64 arrays
        x = [[int(a) << int(b) for a, b in zip(ra, rb)] for ra, rb in zip(mi.tolist(), sh.tolist())]
        self.x = x
        nl = max(1, -(-self.bits // _LIMB))
        mask = (1 << _LIMB) - 1
        self.limbs = []
        for l in range(nl):
            s = l * _LIMB
            self.limbs.append(np.array([[((v >> s) & mask) if v >= 0 else -(((-v) >> s) & mask) for v in row]
                                        for row in x], dtype=np.int64).reshape(f.shape))

    def frame(self, t):
        """Frame t as exact mpmath-ready integers (value = int / 2^k)."""
        return self.x[t]

    def moments(self, ranges):
        """Exact Moments of the union of the frame ranges [(begin, end)]."""
        d = self.shape[1]
        n = 0
        s = [0] * d
        m = [[0] * d for _ in range(d)]
        for (b, e) in ranges:
            for c in range(b, e, _ROWS):
                ce = min(e, c + _ROWS)
                n += ce - c
                parts = [l[c:ce] for l in self.limbs]
                for p, a in enumerate(parts):
                    col = a.sum(axis=0).tolist()
                    for i in range(d):
                        s[i] += col[i] << (p * _LIMB)
                    for q in range(p, len(parts)):
                        g = (a.T @ parts[q]).tolist()            # |entries| < 2^(40 + 12): exact in int64
                        sh = (p + q) * _LIMB
                        if p == q:
                            for i in range(d):
                                gi, mi = g[i], m[i]
                                for j in range(d):
                                    mi[j] += gi[j] << sh
                        else:                                    # the (q, p) product is the transpose
                            for i in range(d):
                                gi, mi = g[i], m[i]
                                for j in range(d):
                                    mi[j] += (gi[j] + g[j][i]) << sh
        return Moments(n, s, m, self.k)


# ---------------------------------------------------------------------- determinants
def bareiss_det(a, symmetric=False):
    """det of a square matrix of Python integers, fraction-free: every division is exact.
    symmetric=True: `a` is symmetric positive semi-definite; only the upper triangle is
    eliminated, no pivot search is needed (a zero pivot of a PSD matrix means det = 0)."""
    n = len(a)
    a = [list(r) for r in a]
    if n == 0:
        return 1
    sign, prev = 1, 1
    for k in range(n - 1):
        if a[k][k] == 0:
            if symmetric:
                return 0
            for r in range(k + 1, n):
                if a[r][k] != 0:
                    a[k], a[r] = a[r], a[k]
                    sign = -sign
                    break
            else:
                return 0
        pk, rk = a[k][k], a[k]
        if symmetric:
            for i in range(k + 1, n):
                aik, ri = rk[i], a[i]
                for j in range(i, n):
                    ri[j] = (pk * ri[j] - aik * rk[j]) // prev
        else:
            for i in range(k + 1, n):
                ri = a[i]
                aik = ri[k]
                for j in range(k + 1, n):
                    ri[j] = (pk * ri[j] - aik * rk[j]) // prev
        prev = pk
    return sign * a[n - 1][n - 1]


def _mp(bits=MP_BITS):
    return mpmath.workprec(bits)


def _log_int(v):
    return mpmath.log(mpmath.mpf(v)) if v > 0 else mpmath.mpf('-inf')


def logdet_cov(mom):
    """log det of the sample covariance (np.cov) of the frames behind `mom`, exact up to the
    final rounding of the MP_BITS-bit logarithm; -inf when the covariance is singular."""
    d = len(mom.s)
    with _mp():
        det = bareiss_det(mom.scatter(), symmetric=True)
        if det <= 0:
            return mpmath.mpf('-inf')
        return (_log_int(det) - d * _log_int(mom.n * (mom.n - 1))
                - 2 * d * mom.k * mpmath.log(mpmath.mpf(2)))


def logdet_pooled(m1, m2):
    """log det((n1/n) S1 + (n2/n) S2), the pooled term of GLR:
    (n1/n) S1 + (n2/n) S2 = ((n2 - 1) A1 + (n1 - 1) A2) / (n (n1 - 1) (n2 - 1)) / 4^k."""
    d = len(m1.s)
    a1, a2 = m1.scatter(), m2.scatter()
    w1, w2 = m2.n - 1, m1.n - 1
    b = [[w1 * a1[i][j] + w2 * a2[i][j] for j in range(d)] for i in range(d)]
    with _mp():
        det = bareiss_det(b, symmetric=True)
        if det <= 0:
            return mpmath.mpf('-inf')
        return (_log_int(det) - d * _log_int((m1.n + m2.n) * (m1.n - 1) * (m2.n - 1))
                - 2 * d * m1.k * mpmath.log(mpmath.mpf(2)))


def pair_logdets(m1, m2, want_glr=True):
    """(logdet1, logdet2, logdet_union, logdet_glr or None) as mpf."""
    return (logdet_cov(m1), logdet_cov(m2), logdet_cov(m1 + m2),
            logdet_pooled(m1, m2) if want_glr else None)


def bic(n1, n2, ld1, ld2, ldu, lambdac, dim=DIM):
    """change_detection.bic_from_terms on exact log-dets (mpf)."""
    with _mp():
        n = n1 + n2
        h = mpmath.mpf(1) / 2
        pen = mpmath.mpf(lambdac) * h * (dim + h * dim * (dim + 1)) * mpmath.log(mpmath.mpf(n))
        return h * n * ldu - h * n1 * ld1 - h * n2 * ld2 - pen


def glr(n1, n2, ld1, ld2, ldg):
    """change_detection.glr_from_terms on exact log-dets (mpf)."""
    with _mp():
        n = mpmath.mpf(n1 + n2)
        return -(n / 2) * ((n1 / n) * ld1 + (n2 / n) * ld2 - ldg)


def _cov_and_inv_diag(mom):
    """(diag of cov, diag of cov^-1, mean) as mpf lists at MP_BITS_INV bits."""
    d = len(mom.s)
    a = mom.scatter()
    scale = mpmath.mpf(mom.n * (mom.n - 1)) * mpmath.mpf(4) ** mom.k        # cov = A / scale
    # symmetric elimination A = L D L^T in mpf, then the diagonal of A^-1 from the rows of L^-1
    low = [[mpmath.mpf(0)] * d for _ in range(d)]
    ld = [[mpmath.mpf(0)] * d for _ in range(d)]          # L_ik D_k
    dg = [mpmath.mpf(0)] * d
    for j in range(d):
        dg[j] = mpmath.mpf(a[j][j]) - sum((low[j][k] * ld[j][k] for k in range(j)), mpmath.mpf(0))
        if not dg[j] > 0:
            raise ZeroDivisionError('covariance is singular')
        for i in range(j + 1, d):
            v = mpmath.mpf(a[i][j]) - sum((ld[i][k] * low[j][k] for k in range(j)), mpmath.mpf(0))
            ld[i][j] = v
            low[i][j] = v / dg[j]
    # X = L^-1 (unit lower), column by column; (A^-1)_ii = sum_k X_ki^2 / D_k
    inv_diag = [mpmath.mpf(0)] * d
    for i in range(d):
        col = [mpmath.mpf(0)] * d
        col[i] = mpmath.mpf(1)
        for r in range(i + 1, d):
            acc = mpmath.mpf(0)
            lr = low[r]
            for c in range(i, r):
                if col[c] != 0:
                    acc += lr[c] * col[c]
            col[r] = -acc
        inv_diag[i] = sum((col[r] * col[r] / dg[r] for r in range(i, d)), mpmath.mpf(0)) * scale
    cov_diag = [mpmath.mpf(a[i][i]) / scale for i in range(d)]
    mean = [mpmath.mpf(mom.s[i]) / mom.n / mpmath.mpf(2) ** mom.k for i in range(d)]
    return cov_diag, inv_diag, mean


def kl2(m1, m2):
    """numpy_engine.kl2_frames with exact covariances, inverses and means.  The reference's
    products are element-wise, so only the diagonals enter:
    1/2 sum_i (S1_ii - S2_ii)(P2_ii - P1_ii) + 1/2 sum_i (P1_ii + P2_ii) delta_i^2."""
    with _mp(MP_BITS_INV):
        c1, p1, mu1 = _cov_and_inv_diag(m1)
        c2, p2, mu2 = _cov_and_inv_diag(m2)
        t = mpmath.mpf(0)
        for i in range(len(c1)):
            dl = mu1[i] - mu2[i]
            t += (c1[i] - c2[i]) * (p2[i] - p1[i]) + (p1[i] + p2[i]) * dl * dl
        return t / 2


# ---------------------------------------------------------------------- doubles
def hi_lo(v):
    """v (mpf) as a pair of doubles hi + lo, hex strings; hi is v rounded to nearest."""
    with _mp():
        hi = float(v)
        if math.isinf(hi) or math.isnan(hi):
            return [hi.hex(), (0.0).hex()]
        lo = float(v - mpmath.mpf(hi))
        return [hi.hex(), lo.hex()]


def from_hi_lo(pair):
    return float.fromhex(pair[0])


def rel(a, b):
    """The project's measure of a difference between two scores."""
    return abs(a - b) / max(1.0, abs(a), abs(b))
