"""The strand bootstrap restated for its tests (tests/test_merge_bootstrap_cpu.py, tests/test_gpu_merge_bootstrap.py):
the strand draws from tests/philox_ref.py's words, the expansion and the live counts strand by strand as the reference
states them (utils.resample_run, utils.py:1601-1622), and the integrals of the expanded sequence in long double with
the bounds of tests/merge_errors_ref.py -- those are a function of the sequence (ln L, n) they are given, so the chain
length comes from M', the resampled run's length.  Nothing here is the package's code."""
import numpy as np

import merge_errors_ref as er
import philox_ref
from merge_errors_ref import U, bounds, check, device_chains, host_chains  # noqa: F401

KS_CRIT = 0.0617  # two samples of 2000 at level 0.001 (1.95 sqrt(2 / 2000))


def draws(seed, boot, S):
    """Strand of draw j < S of bootstrap `boot`: x = w_2j | w_2j+1 << 32 of subsequence 2^63 + boot, strand = x S >> 64
    (Python integers)."""
    w = philox_ref.words(int(seed), [(1 << 63) + int(boot)], 0, 2 * S)[0]
    return np.array([((int(w[2 * j]) | (int(w[2 * j + 1]) << 32)) * S) >> 64 for j in range(S)], dtype=np.int64)


def expand(logl, key, mult):
    """(idx, n') of the resampled run, strand by strand: the points of every drawn strand, sorted by ln L (stable, by
    merged index inside ties); a strand drawn m times adds m live points below its last point's ln L, and at that
    ln L, over the g positions of equal ln L, int(j / (g / m)) + 1 counted from the group's end."""
    logl, key = np.asarray(logl, dtype=np.float64), np.asarray(key)
    parts = [np.flatnonzero(key == u) for u, m in enumerate(mult) for _ in range(int(m))]
    idx = np.sort(np.concatenate(parts), kind="stable")
    l = logl[idx]
    n = np.zeros(len(idx), dtype=np.int64)
    for u, m in enumerate(mult):
        if m == 0:
            continue
        upper = logl[key == u].max()
        n[l < upper] += int(m)
        end = np.flatnonzero(l == upper)
        g = len(end)
        n[end] += (np.arange(g) / (g / int(m))).astype(np.int64)[::-1] + 1
    return idx, n


def hp(m, idx, n, seed, boot, jitter):
    """The long-double realization `boot` of the expanded sequence of the merged run `m`."""
    return er.realization_hp(np.asarray(m["logl"])[idx], n, seed, boot, jitter, None, np.asarray(m["samples"])[idx])


def reference_allowance(h):
    """The reference's own float64 arithmetic against the exact value: sequential sums (host chains) and its volume
    steps log(n / (n + 1)), whose quotient next to 1 is rounded at full size: u absolute per step, 2 M' u by the end
    (tests/test_merge_errors_cpu.py's reference_allowance, at M')."""
    b = bounds(h, host_chains(h["M"]))
    return {k: b[k] + h["M"] * 2 * U for k in b}


def sort_in_ties(idx, logl):
    """idx with every group of equal ln L in ascending order."""
    idx = np.asarray(idx, dtype=np.int64)
    return idx[np.lexsort((idx, np.asarray(logl)[idx]))]


def ks2(a, b):
    a, b = np.sort(a), np.sort(b)
    x = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, x, side="right") / len(a) - np.searchsorted(b, x, side="right") / len(b))))


def gates(lz, fix, label):
    """KS below the critical value, means within 3 combined standard errors, ratio of standard deviations in [0.9, 1.1]."""
    ks = ks2(lz, fix)
    se = np.sqrt(lz.var(ddof=1) / len(lz) + fix.var(ddof=1) / len(fix))
    dm = abs(lz.mean() - fix.mean()) / se
    ratio = lz.std(ddof=1) / fix.std(ddof=1)
    print(f"[merge bootstrap {label}] KS {ks:.4f} (< {KS_CRIT}), mean difference {dm:.2f} se (<= 3), sd ratio {ratio:.4f}")
    assert ks < KS_CRIT
    assert dm <= 3
    assert 0.9 <= ratio <= 1.1
