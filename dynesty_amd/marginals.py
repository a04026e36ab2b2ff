"""Credible intervals and the histograms of a corner plot, one surface for both merge routes.

`ensemble.MergedRun` (merge='host') computes them in NumPy, `_lib.DeviceMergedRun` (merge='device') where the run
lives (csrc/merge_marginals.hip).  This module holds what the two share: how `columns`, `bins` and
`range` are read, and `corner_data`.  A class supplies `ndim`, `_quantile(q, cols)`, `_hist1d(cols, edges, weighted, ranges)`
(ranges: the (lo, hi) the edges were spaced over, None for explicit edges) and `_hist2d(pairs, xedges, yedges, weighted)`,
which validate their own arguments."""
import numpy as np


def _is_count(b):
    return isinstance(b, (int, np.integer))


def _edges(bins, rng, n, minmax):
    """(n, nb + 1) edges and the (n, 2) ranges they span (None for explicit edges): `bins` an int with `rng` (None:
    minmax(), a (lo, hi) pair for all, or n pairs), or explicit edges (one set for all, or n sets).  Integer bins are
    np.linspace(lo, hi, bins + 1), np.histogram's own edges."""
    if not _is_count(bins):
        e = np.asarray(bins, dtype=np.float64)
        if e.ndim == 1:
            e = np.broadcast_to(e, (n, len(e)))
        if e.ndim != 2 or e.shape[0] != n or e.shape[1] < 2:
            raise ValueError(f"bins: explicit edges of shape {e.shape} for {n} histograms")
        return np.ascontiguousarray(e), None
    nb = int(bins)
    if nb < 1:
        raise ValueError("bins must be positive")
    r = minmax() if rng is None else np.asarray(rng, dtype=np.float64)
    if r.ndim == 1:
        r = np.broadcast_to(r, (n, 2))
    if r.shape != (n, 2) or not np.isfinite(r).all() or (r[:, 0] > r[:, 1]).any():
        raise ValueError(f"range: (lo, hi) pairs with lo <= hi for {n} histograms")
    out = np.empty((n, nb + 1))
    for i, (lo, hi) in enumerate(r):
        if lo == hi:  # np.histogram's rule for an empty range
            lo, hi = lo - 0.5, hi + 0.5
        out[i] = np.linspace(lo, hi, nb + 1)
    return out, np.ascontiguousarray(r)


class Marginals:
    def _columns(self, columns):
        if columns is None:
            return np.arange(self.ndim, dtype=np.int32)
        c = np.atleast_1d(np.asarray(columns))
        if c.ndim != 1 or not np.issubdtype(c.dtype, np.integer):
            raise ValueError("columns: a list of column indices")
        return np.ascontiguousarray(c, dtype=np.int32)

    def _minmax(self, cols):
        """[min, max] per column: quantile([0, 1]), which both routes return exactly and for any weights."""
        return self._quantile(np.array([0., 1.]), cols)

    def quantile(self, q, columns=None):
        """utils.quantile(samples[:, c], q, weights=importance_weights) for every column c of `columns` (None: all):
        an array of shape (ncol, nq).  The order of a column is np.argsort(kind="stable")'s."""
        q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
        if q.ndim != 1:
            raise ValueError("q: a list of quantiles")
        return self._quantile(q, self._columns(columns))

    def histogram(self, columns=None, bins=50, range=None, weighted=True):
        """np.histogram(samples[:, c], bins, range, weights=importance_weights) per column (weighted=False: counts).
        bins: an int, or explicit edges (one set, or one per column); range: None = the column's [min, max], a
        (lo, hi) pair, or one per column.  Returns (hist (ncol, nbins), edges (ncol, nbins + 1))."""
        cols = self._columns(columns)
        # `ranges` goes along for the host route alone: np.histogram sums each bin on its own for bins=int, range=
        # but differences a cumulative sum for explicit edges (absolute error 1e-16 in a bin of 1e-30), so MergedRun
        # has to call the first form to BE np.histogram there; the device works from the edges and ignores it
        edges, ranges = _edges(bins, range, len(cols), lambda: self._minmax(cols))
        return self._hist1d(cols, edges, bool(weighted), ranges), edges

    def histogram2d(self, pairs, bins=50, range=None, weighted=True):
        """np.histogram2d(samples[:, i], samples[:, j], bins, range, weights=importance_weights) per pair (i, j).
        bins: an int, (nbx, nby), or (xedges, yedges) (one set each, or one per pair); range: None = [min, max] per
        column, ((xlo, xhi), (ylo, yhi)), or one such per pair.  Returns (H (npair, nbx, nby), xedges, yedges)."""
        p = np.asarray(pairs)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
            raise ValueError("pairs: a list of (column, column)")
        p = np.ascontiguousarray(p, dtype=np.int32)
        bx, by = (bins, bins) if _is_count(bins) else bins
        if range is None:
            rx = ry = None
        else:
            r = np.asarray(range, dtype=np.float64)
            if r.ndim == 2:
                r = np.broadcast_to(r, (len(p), 2, 2))
            if r.shape != (len(p), 2, 2):
                raise ValueError("range: ((xlo, xhi), (ylo, yhi)), or one per pair")
            rx, ry = r[:, 0], r[:, 1]
        xe = _edges(bx, rx, len(p), lambda: self._minmax(p[:, 0]))[0]
        ye = _edges(by, ry, len(p), lambda: self._minmax(p[:, 1]))[0]
        return self._hist2d(p, xe, ye, bool(weighted)), xe, ye

    def corner_data(self, span=0.999999426697, bins=50, columns=None):
        """What a corner plot is drawn from: per column the span [quantile(0.5 - span / 2), quantile(0.5 + span / 2)]
        (plotting.check_span), its 1-D weighted histogram in that span, and for every pair i < j of the columns the
        2-D weighted histogram in the two spans.  Returns a dict: columns, span (ncol, 2), hist (ncol, bins),
        edges (ncol, bins + 1), pairs (npair, 2), hist2d (npair, bins, bins), xedges, yedges."""
        cols = self._columns(columns)
        sp = self.quantile([0.5 - 0.5 * span, 0.5 + 0.5 * span], cols)
        hist, edges = self.histogram(cols, bins=bins, range=sp)
        n = len(cols)
        ij = np.array([(i, j) for i in np.arange(n) for j in np.arange(i + 1, n)], dtype=np.int64).reshape(-1, 2)
        out = dict(columns=cols, span=sp, hist=hist, edges=edges, pairs=cols[ij])
        if len(ij):
            out["hist2d"], out["xedges"], out["yedges"] = self.histogram2d(
                cols[ij], bins=bins, range=np.stack([sp[ij[:, 0]], sp[ij[:, 1]]], axis=1))
        else:
            out["hist2d"], out["xedges"], out["yedges"] = np.empty((0, bins, bins)), np.empty((0, bins + 1)), np.empty((0, bins + 1))
        return out
