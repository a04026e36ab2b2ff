"""The exact weighted quantile function of a column, and the backward error of a returned quantile against it.

`utils.quantile(x, q, weights)` interpolates the points (cdf_k, x_(k)), k = 0 .. M-1, where x_(k) is the column in
stable ascending order, C_k the sum of the weights of the first k points in that order and cdf_k = C_k / C_{M-1}.  Its
quantile function Q is that piecewise-linear, non-decreasing curve (a vertical segment where a weight is zero), and
Q = x_(M-1) from cdf_{M-1} = 1 on.  Here C_k are exact: every float64 weight is an integer multiple of 2^-1126, and the
sums are Python integers.

Why a backward error.  Where the weights in a tail are tiny, Q has slopes of 10^11 and more: a forward bound
slope * eps says nothing, while the differences that occur are 10^-14.  So a returned y is judged by the q it
answers: `preimage` gives the set {q : Q(q) = y} (an interval where values are tied, one point on a slope, the
jump's q on a vertical segment), and `backward_error` the distance of the requested q from that set, for y or y moved
by up to 4 ulp: the final addition of the interpolation rounds y itself by up to half an ulp, a real displacement, so
the set is that of the whole interval [y - 4 ulp, y + 4 ulp] -- Q is monotone, so it runs from the lower end of the
lower bound's set to the upper end of the upper bound's.  (Trying only the nine doubles around y is not the same
thing: between two points 10^-5 apart, one of them holding 10^-3 of the weight, neighbouring doubles are 4 10^-14
apart in q, and a correctly rounded y is up to half of that from the q asked for.)

Budgets, in units of q (cdf <= 1 and t <= 1 throughout).

The device (csrc/merge_marginals.hip) replaces w_i by W_i 2^-62, W_i = llrint(w_i 2^62), |W_i 2^-62 - w_i| <= u = 2^-63, and
then works in exact integers.  With a = C_k + t w_(k) the exact cumulative weight at the returned point, r = Norm - a
the rest, and a', r' their integer versions, |a' - a| <= n_a u and |r' - r| <= n_r u with n_a + n_r <= M points, and

    a / (a + r) - a' / (a' + r') = (a r' - a' r) / (Norm Norm') = (a dr - r da) / (Norm Norm'),
    |a dr - r da| <= max(a, r) (n_a + n_r) u <= Norm M u,

so the quantisation moves q by at most M u / Norm', Norm' >= Norm - M u.  Then the float64 steps, each one rounding
of relative size 2^-53 of a quantity that is at most 1 in q units: fl(Norm) and the product q Norm (2); the integer
difference floor(T) - C_k to double, its sum with T's fraction, W_(k) to double, the division (4); the difference
x_(k+1) - x_(k) and its product with t, both relative changes of t (2).  The last addition is the 4-ulp allowance.

    eps_device = M 2^-63 / (Norm - M 2^-63) + 8 * 2^-53.

The reference's own float64 result carries its sequential cumsum: M - 1 additions of partial sums <= 1, M 2^-53 with
the normalisation and np.interp's few roundings inside the margin the M - 1 leaves:

    eps_reference = M 2^-53."""
from fractions import Fraction

import numpy as np

SCALE_BITS = 1126  # float64: 53 bits above 2^-1074 at the least


def _exact(w):
    num, den = float(w).as_integer_ratio()
    return num * ((1 << SCALE_BITS) // den)


class Column:
    """One column: `x` (M,) values, `w` (M,) float64 weights."""

    def __init__(self, x, w):
        x = np.asarray(x, dtype=np.float64)
        w = np.asarray(w, dtype=np.float64)
        self.order = np.argsort(x, kind="stable")
        self.xs = x[self.order]
        self.M = len(x)
        c = [0]
        for wi in w[self.order][:-1]:
            c.append(c[-1] + _exact(wi))
        self.C = c  # C[k] = sum of the first k weights, scaled by 2^SCALE_BITS
        self.norm = c[-1]
        self.norm_float = float(Fraction(self.norm, 1 << SCALE_BITS))

    def preimage(self, y):
        """(a, b): {q : Q(q) = y} = [a / norm, b / norm] as exact numbers scaled by norm; None outside the range."""
        lo = int(np.searchsorted(self.xs, y, side="left"))
        hi = int(np.searchsorted(self.xs, y, side="right"))
        if hi > lo:
            return Fraction(self.C[lo]), Fraction(self.C[hi - 1])
        if lo == 0 or lo == self.M:
            return None
        k = lo - 1
        t = (Fraction(float(y)) - Fraction(float(self.xs[k]))) / (Fraction(float(self.xs[k + 1])) - Fraction(float(self.xs[k])))
        a = self.C[k] + t * (self.C[k + 1] - self.C[k])
        return a, a

    def backward_error(self, q, y, ulps=4):
        """Distance from q to {q' : Q(q') in [y - ulps ulp(y), y + ulps ulp(y)]} (inf where that set is empty)."""
        y = float(y)
        r = ulps * float(np.spacing(abs(y)))
        lo, hi = y - r, y + r  # (exact: a few ulps of y)
        if hi < self.xs[0] or lo > self.xs[-1]:
            return np.inf
        a = Fraction(0) if lo <= self.xs[0] else self.preimage(lo)[0]
        b = Fraction(self.norm) if hi >= self.xs[-1] else self.preimage(hi)[1]
        target = Fraction(float(q)) * self.norm
        return float(max(a - target, target - b, 0) / self.norm)

    def eps_device(self):
        u = 2.0 ** -63
        return self.M * u / (self.norm_float - self.M * u) + 8 * 2.0 ** -53

    def eps_reference(self):
        return self.M * 2.0 ** -53


def worst(samples, w, cols, q, got, kind):
    """Worst backward error / budget over the columns `cols` and quantiles `q` of `got` (ncol, nq); kind: 'device' or
    'reference'.  Returns (worst ratio, worst error, budget of that column)."""
    out = (0.0, 0.0, 0.0)
    for i, c in enumerate(cols):
        col = Column(np.asarray(samples)[:, c], w)
        eps = col.eps_device() if kind == "device" else col.eps_reference()
        for qq, y in zip(q, got[i]):
            e = col.backward_error(qq, y)
            if e / eps >= out[0]:
                out = (e / eps, e, eps)
    return out
