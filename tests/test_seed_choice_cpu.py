"""The seeds of a dynamic batch as a pure function (dynesty_amd/seeds.py, the NumPy mirror of csrc/merge_seed.hip;
DESIGN.md section 3.8.6): the law -- the k largest of logvol + Gumbel noise against the exact probabilities of
successive sampling, with Generator.choice held to the same statistic --, the bookkeeping against dynamic.batch_seed on
a MergedRun, and the arguments run_dynamic refuses."""
import itertools

import numpy as np
import pytest

import fold_cases
import merge_cases
from dynesty_amd import dynamic, seeds

LOGVOL7 = np.array([0.0, -0.2, -0.45, -0.6, -0.9, -1.1, -1.35])
K7, STRANDS7 = 3, 8192


def ordered_outcomes(logvol, k):
    """Every ordered k-tuple of distinct points with its probability under successive sampling proportional to
    exp(logvol): (tuples, probabilities)."""
    w = np.exp(logvol - np.max(logvol))
    outs, probs = [], []
    for t in itertools.permutations(range(len(w)), k):
        p, rest = 1.0, w.sum()
        for i in t:
            p *= w[i] / rest
            rest -= w[i]
        outs.append(t)
        probs.append(p)
    return outs, np.array(probs)


def chi2_quantile(df, p):
    """The p quantile of chi^2(df): scipy where it is installed, else Wilson-Hilferty with the normal quantile by
    bisection on erf (good to a few parts in 10^4 at df = 209, far inside the gap to the statistics seen)."""
    try:
        from scipy import stats
        return float(stats.chi2.ppf(p, df))
    except ImportError:
        import math
        lo, hi = 0.0, 10.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if 0.5 * (1.0 + math.erf(mid / math.sqrt(2.0))) < p:
                lo = mid
            else:
                hi = mid
        z = 0.5 * (lo + hi)
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi2_of(draws, logvol, k):
    """Pearson's statistic of the ordered outcomes `draws` (n, k) against successive sampling; (chi2, smallest
    expected count, number of outcomes)."""
    outs, probs = ordered_outcomes(logvol, k)
    where = {t: j for j, t in enumerate(outs)}
    counts = np.zeros(len(outs))
    for row in np.asarray(draws):
        counts[where[tuple(int(x) for x in row)]] += 1
    expect = probs * len(draws)
    return float(((counts - expect) ** 2 / expect).sum()), float(expect.min()), len(outs)


def test_the_law_is_successive_sampling():
    """7 points, k = 3, 8192 strands, seed 1: the counts of the 210 ordered outcomes against the exact probabilities;
    pass iff chi^2 lies below the 1 - 1e-4 quantile of chi^2(209) (about 293).  Generator.choice(p, replace=False), the
    host route's call, is held to the same statistic."""
    bound = chi2_quantile(209, 1.0 - 1e-4)
    assert 285.0 < bound < 300.0
    key = seeds.seed_keys_host(LOGVOL7, 1, STRANDS7)
    assert key.shape == (STRANDS7, 7)
    order = np.argsort(-key, axis=1, kind="stable")
    top = np.take_along_axis(key, order, axis=1)[:, :K7 + 1]
    gap = float(np.min(top[:, :-1] - top[:, 1:]))
    chi2, emin, nout = chi2_of(order[:, :K7], LOGVOL7, K7)
    print(f"[seed law] mirror: chi2 = {chi2:.1f} (bound {bound:.1f}), smallest expected count {emin:.2f}, smallest gap "
          f"among the top four keys {gap:.3g}")
    assert nout == 210 and 5.5 < emin < 5.7
    assert gap > 1e-5
    assert chi2 < bound
    # the same through the whole mirror: 8 points, the first at the boundary, so the subset is the 7 points above it
    logl = np.arange(8, dtype=np.float64)
    got = seeds.batch_seeds_host(logl, np.concatenate([[0.5], LOGVOL7]), np.zeros(8), np.zeros(8), np.zeros(8), 0.0, K7,
                                 1, STRANDS7)
    assert got["lo"] == 1 and got["count"] == got["n_pos"] == 7 and got["idx"].min() >= 1
    chi2_b = chi2_of(got["idx"] - 1, LOGVOL7, K7)[0]
    print(f"[seed law] batch_seeds_host on the shifted points: chi2 = {chi2_b:.1f}")
    assert chi2_b < bound
    rng = np.random.default_rng(1)
    w = np.exp(LOGVOL7)
    draws = np.array([rng.choice(7, size=K7, p=w / w.sum(), replace=False) for _ in range(STRANDS7)])
    chi2_g = chi2_of(draws, LOGVOL7, K7)[0]
    print(f"[seed law] Generator.choice: chi2 = {chi2_g:.1f}")
    assert chi2_g < bound


def test_keys_are_a_function_of_seed_strand_and_point():
    a = seeds.seed_keys_host(LOGVOL7, 5, 5)
    np.testing.assert_array_equal(seeds.seed_keys_host(LOGVOL7, 5, 2, first=3), a[3:5])
    np.testing.assert_array_equal(seeds.seed_keys_host(LOGVOL7[:4], 5, 5), a[:, :4])  # a point's words are its index's
    assert not np.array_equal(seeds.seed_keys_host(LOGVOL7, 6, 5), a)
    from dynesty_amd import errors
    u = errors.uniforms(5, [seeds.SEED_SEQ + 2], 7)[0]
    np.testing.assert_array_equal(a[2], LOGVOL7 - np.log(-np.log(u)))
    assert seeds.SEED_SEQ == errors.BOOT_SEQ + (1 << 62)


def host_run(seed=2, base_niters=(300, 310, 290), base_nlive=20, D=3):
    rng = np.random.default_rng(seed)
    base = merge_cases.make(rng, list(base_niters), base_nlive, D)
    return dynamic.single_run(merge_cases.host_merge(base, prior_transform=lambda u: 20. * u - 10.))


@pytest.fixture(scope="module")
def fold_run():
    """The base of a fold case (tests/fold_cases.py) merged on the host: three base values equal to logl_min."""
    kw = fold_cases.CASES["one_strand_d1"]
    base, _, lmin, _ = fold_cases.make(**kw)
    return dynamic.single_run(merge_cases.host_merge(base, prior_transform=lambda u: 20. * u - 10.)), lmin


def same_bookkeeping(m, logl_min, k):
    got = m.batch_seeds(logl_min, k, 3, seed=9, want_keys=True)
    want = dynamic.batch_seed(m, (logl_min, 1e300), k, np.random.default_rng(4))
    assert got["prior"] == want["prior"] and got["logl_min"] == want["logl_min"] and got["vol_idx"] == want["vol_idx"]
    assert got["start"] == want["start"]
    return got, want


def test_bookkeeping_equals_batch_seed(fold_run):
    m, lmin = fold_run
    M = len(m.logl)
    # a boundary inside the run; on a plateau of equal ln L (the fold case's three base values at logl_min)
    got, want = same_bookkeeping(m, float(m.logl[M // 2]) + 1e-9, 16)
    assert not got["prior"] and got["idx"].shape == (3, 16) and got["count"] == M - got["lo"]
    assert got["lo"] == int(np.searchsorted(m.logl, float(m.logl[M // 2]) + 1e-9, side="right")) > M // 2
    assert (m.logl[got["idx"]] > got["logl_min"]).all() and (np.diff(got["keys"], axis=1) <= 0).all()
    assert all(len(set(row)) == 16 for row in got["idx"])
    assert (m.logl == lmin).sum() >= 3
    got, want = same_bookkeeping(m, lmin, 16)
    assert got["vol_idx"] == int(np.nonzero(m.logl == lmin)[0][0]) + 1 and got["lo"] == int((m.logl <= lmin).sum())
    # fewer than nlive_new points above it: the boundary moves down to the last nlive_new points
    got, want = same_bookkeeping(m, float(m.logl[-5]), 12)
    assert got["lo"] == M - 12 and got["count"] == 12 and got["logl_min"] == m.logl[M - 13] and got["n_pos"] == 12
    assert all(sorted(row) == list(range(M - 12, M)) for row in got["idx"])
    # ... and below the first point where the run is that short: a prior strand whose seeds stand
    short = host_run(base_niters=(3, 2, 4), base_nlive=4)
    got, want = same_bookkeeping(short, float(short.logl[-3]), len(short.logl))
    assert got["prior"] and got["logl_min"] == -np.inf and got["vol_idx"] == 0 and got["start"] is None
    assert all(sorted(row) == list(range(len(short.logl))) for row in got["idx"])
    # below the first point: from the prior, no choice
    got, want = same_bookkeeping(m, float(m.logl[0]) - 1.0, 16)
    assert got["prior"] and got["idx"] is None and want["idx"] is None and got["lo"] == 0 and got["n_pos"] == 0
    got, want = same_bookkeeping(m, -np.inf, 16)
    assert got["prior"] and got["vol_idx"] == 0
    # above the last point
    for call in (lambda: m.batch_seeds(float(m.logl[-1]), 16, 2, seed=1),
                 lambda: dynamic.batch_seed(m, (float(m.logl[-1]), 1e300), 16, np.random.default_rng(1))):
        with pytest.raises(RuntimeError, match="Could not find live points"):
            call()
    for bad in (dict(strands=0), dict(strands=65537), dict(nlive_new=0), dict(nlive_new=65536), dict(logl_min=np.nan),
                dict(seed=-1), dict(first=-1)):
        kw = dict(logl_min=lmin, nlive_new=16, strands=2, seed=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            m.batch_seeds(**kw)


def test_too_few_points_of_positive_weight():
    """2 runs x 2 live points x 1700 iterations, so that logvol spans more than 708 (1500 iterations, 3000 steps of
    ln(5/4), span 671: the cut-off would lie outside the run): both routes raise ValueError where nlive_new exceeds the
    points of positive weight."""
    m = host_run(seed=6, base_niters=(1700, 1700), base_nlive=2)
    assert m.logvol[0] - m.logvol[-1] > 708.0
    lmin = float(m.logl[10])
    sub = m.logvol[11:]
    n_pos = int((sub - sub.max() >= seeds.LOG_MIN).sum())
    w = np.exp(sub - sub.max())
    n_host = int((w / w.sum() > 0).sum())  # (the host's test lets the denormal tail of exp through: the departure)
    assert 0 < n_pos <= n_host < len(sub)
    got, want = same_bookkeeping(m, lmin, n_pos)
    assert got["n_pos"] == n_pos and got["idx"].max() < 11 + n_pos
    for call in (lambda: m.batch_seeds(lmin, n_pos + 1, 2, seed=1),
                 lambda: dynamic.batch_seed(m, (lmin, 1e300), n_host + 1, np.random.default_rng(1))):
        with pytest.raises(ValueError, match="positive weight"):
            call()


def test_run_dynamic_refuses_device_seeds_on_the_host_merge():
    with pytest.raises(ValueError, match="merge='device'"):
        dynamic.run_dynamic(None, 2, 16, 2, 16, 1, merge='host', seeds='device')
    with pytest.raises(ValueError, match="seeds="):
        dynamic.run_dynamic(None, 2, 16, 2, 16, 1, seeds='gpu')
