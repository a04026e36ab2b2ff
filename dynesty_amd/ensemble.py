"""Many independent runs sharded over the GPUs of one node (BASELINE config C5).

Runs share nothing: rank r -- one process per GPU,
launched by torchrun / torch.distributed.run -- owns a contiguous block of run
ids and executes them on its own device with no communication.  Seeds are
derived from the *global* run id (``SeedSequence(base).spawn(total)[run]``), so
results do not depend on the number of GPUs.  The only exchange step is at the
end: one fixed-size record per run, all-gathered with RCCL over xGMI (backend
"nccl" on ROCm; "gloo" in the CPU tests).  At 512 x 5 doubles = 20 KB the
collective is latency bound; posterior samples stay sharded (they can be merged
on the host with the reference's ``utils.merge_runs``) unless ``gather_ragged``
is asked for them.
"""
import numpy as np

from .errors import (Errors, bootstrap_host, bootstrap_run_host, kld_bootstrap_host, kld_bootstrap_run_host, kld_host,
                     kld_run_host, realization_host, realize_host, weight_bounds, weight_indices, weights_host)
from .marginals import Marginals

RECORD_FIELDS = ("run", "logz", "logzerr", "niter", "ncall", "h")


def shard_runs(total, world, rank):
    """Contiguous block of run ids owned by `rank` (sizes differ by <= 1)."""
    base, extra = divmod(int(total), int(world))
    start = rank * base + min(rank, extra)
    return range(start, start + base + (1 if rank < extra else 0))


def run_seeds(base_seed, total):
    """One SeedSequence child per global run id."""
    return np.random.SeedSequence(base_seed).spawn(int(total))


def gather_records(local, total, world, rank, dist=None, device=None, nfield=None):
    """All-gather the per-run records (n_local x len(RECORD_FIELDS), float64;
    column 0 is the global run id).  Returns the (total x nfield) table ordered
    by run id on every rank.  With dist=None (no process group) it is a sort;
    with a process group the collective runs for every world size, 1 included
    (a one-rank RCCL communicator is still RCCL: `bench.py` and the `-m gpu`
    tests go through it on a single MI355X)."""
    local = np.ascontiguousarray(local, dtype=np.float64).reshape(
        -1, nfield or len(RECORD_FIELDS))
    if dist is None:
        out = local
    else:
        import torch
        nmax = -(-int(total) // int(world))  # ceil: equal-sized buffers
        buf = np.full((nmax, local.shape[1]), np.nan)
        buf[:len(local)] = local
        t = torch.from_numpy(buf)
        if device is not None:
            t = t.to(device)
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        out = np.concatenate([p.cpu().numpy() for p in parts])
        out = out[~np.isnan(out[:, 0])]
    out = out[np.argsort(out[:, 0], kind="stable")]
    assert len(out) == total, (len(out), total)
    return out


def gather_ragged(arrays, world, rank, dist=None, device=None):
    """Optional second exchange: gather variable-length (n_i, d) float64 arrays
    (e.g. weighted posterior samples) as [counts all-gather, padded
    all-gather].  Returns the list of arrays of every rank, in rank order."""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    if dist is None:
        return arrays
    import torch
    d = arrays[0].shape[1] if arrays else 0
    flat = np.concatenate(arrays) if arrays else np.zeros((0, d))
    counts = torch.tensor([len(a) for a in arrays] or [0], dtype=torch.int64)
    meta = torch.tensor([len(arrays), len(flat), d], dtype=torch.int64)
    if device is not None:
        meta = meta.to(device)
    metas = [torch.empty_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta)
    metas = [m.cpu().numpy() for m in metas]
    max_runs = max(int(m[0]) for m in metas) or 1
    max_rows = max(int(m[1]) for m in metas) or 1
    d = max(int(m[2]) for m in metas)
    cbuf = torch.zeros(max_runs, dtype=torch.int64)
    cbuf[:len(arrays)] = counts[:len(arrays)]
    fbuf = torch.zeros((max_rows, d), dtype=torch.float64)
    if len(flat):
        fbuf[:len(flat)] = torch.from_numpy(flat)
    if device is not None:
        cbuf, fbuf = cbuf.to(device), fbuf.to(device)
    call = [torch.empty_like(cbuf) for _ in range(world)]
    fall = [torch.empty_like(fbuf) for _ in range(world)]
    dist.all_gather(call, cbuf)
    dist.all_gather(fall, fbuf)
    out = []
    for r in range(world):
        c = call[r].cpu().numpy()[:int(metas[r][0])]
        f = fall[r].cpu().numpy()
        off = 0
        for n in c:
            out.append(f[off:off + int(n)].copy())
            off += int(n)
    return out


def run_ensemble(prob, total_runs, base_seed=21, world=1, rank=0, dist=None,
                 device=None, **run_kw):
    """Run this rank's shard with ``nested.run_static`` and gather the records.
    Returns (table, local_results)."""
    from . import nested
    seeds = run_seeds(base_seed, total_runs)
    mine = shard_runs(total_runs, world, rank)
    local, results = [], []
    for rid in mine:
        rng = np.random.Generator(np.random.PCG64(seeds[rid]))
        r = nested.run_static(prob, rstate=rng, **run_kw)
        results.append(r)
        local.append([rid, r.logz, r.logzerr, r.niter, r.ncall, r.h])
    table = gather_records(np.array(local).reshape(-1, len(RECORD_FIELDS)),
                           total_runs, world, rank, dist=dist, device=device)
    return table, results


STATUS_RAISED = -99.0  # status of the runs of a rank whose ns_ensemble call raised (never a device status)


def run_ensemble_device(prob, total_runs, base_seed=21, world=1, rank=0,
                        dist=None, device=None, nlive=2000, queue_size=512,
                        walks=None, bound='multi', dlogz=0.01, on_failure='raise', **kw):
    """BASELINE config C5: this rank's shard of `total_runs` static runs executed
    by the device-resident loop (`dh_ns_ensemble`, one launch sequence for the
    whole shard), then the RCCL all-gather of the per-run records.  Seeds are
    keyed on the global run id, so the table does not depend on `world`.
    bound: 'multi' | 'single', or 'balls' / 'cubes' (RadFriends / SupFriends) with
    sample='unif' passed in **kw -- as Context.ns_ensemble takes them.
    on_failure: 'raise' (default) or 'nan' -- what to do with a run whose status is
    not 0; with 'nan' its ln Z / error / information are NaN in the table and
    `combine_logz` leaves it out."""
    if on_failure not in ('raise', 'nan'):
        raise ValueError("on_failure must be 'raise' or 'nan'")
    from .backend import get_backend
    mine = shard_runs(total_runs, world, rank)
    nf = len(RECORD_FIELDS)
    local = np.zeros((0, nf + 1))
    raised = None
    if len(mine):
        try:
            r = get_backend().ns_ensemble(prob, len(mine), nlive, queue_size,
                                          walks=walks, bound=bound, dlogz=dlogz,
                                          entropy=np.atleast_1d(base_seed),
                                          first_run=mine.start, **kw)
        except Exception as e:  # argument / memory / HIP errors raise before any status exists
            #  this rank must still enter the collective, else the others block in the all-gather
            # until the communicator times out: its runs travel as NaN rows with the sentinel status, and every
            # rank raises after the gather; this rank re-raises its own exception
            raised = e
            r = None
        if r is None:
            local = np.full((len(mine), nf + 1), np.nan)
            local[:, 0] = np.arange(mine.start, mine.stop)
            local[:, nf] = STATUS_RAISED
        else:
            status = np.asarray(r["status"]).astype(np.float64)
            bad = np.flatnonzero(status != 0)
            # a failed run (bound rebuild error, dead-point capacity) or one that hit max_fills
            # before dlogz must never enter the table as a valid ln Z estimate
            for key in ("logz", "logzerr", "h"):
                r[key] = np.array(r[key], dtype=np.float64)
                r[key][bad] = np.nan
            local = np.stack([np.arange(mine.start, mine.stop, dtype=np.float64),
                              r["logz"], r["logzerr"], r["niter"].astype(float),
                              r["ncall"].astype(float), r["h"], status], axis=1)
    # The collective comes FIRST: the status column travels with the records, so that every rank
    # learns of a failed run and all of them raise together -- raising on the owning rank alone
    # would leave the others blocked in the all-gather until the communicator times out.
    table = gather_records(local, total_runs, world, rank, dist=dist,
                           device=device, nfield=nf + 1)
    status = table[:, nf]
    table = np.ascontiguousarray(table[:, :nf])
    if raised is not None:
        raise raised
    if np.any(status == STATUS_RAISED):
        raise RuntimeError(
            f"ns_ensemble raised on the rank(s) owning runs "
            f"{[int(table[b, 0]) for b in np.flatnonzero(status == STATUS_RAISED)]}")
    bad = np.flatnonzero(status != 0)
    if len(bad) and on_failure == 'raise':
        raise RuntimeError(
            f"ns_ensemble: runs {[int(table[b, 0]) for b in bad]} ended with status "
            f"{[int(status[b]) for b in bad]} (1 = not converged within max_fills, "
            f"< 0 = failed)")
    return table


def combine_logz(table):
    """Ensemble estimate from the gathered record table: mean and standard error of the
    per-run ln Z over the runs that completed (failed runs carry NaN, see
    run_ensemble_device(on_failure='nan')).  Returns (mean, se, n_used)."""
    lz = np.asarray(table)[:, RECORD_FIELDS.index("logz")]
    ok = np.isfinite(lz)
    n = int(ok.sum())
    if n == 0:
        raise RuntimeError("combine_logz: no completed run in the table")
    se = float(lz[ok].std(ddof=1) / np.sqrt(n)) if n > 1 else float('nan')
    return float(lz[ok].mean()), se, n


class MergedRun(dict, Marginals, Errors):
    """Result of `merge_static_runs`: the fields of the reference's merged
    `Results` (utils.merge_runs) that are defined for an ensemble of static
    runs, with attribute access.  quantile / histogram / histogram2d /
    corner_data (marginals.Marginals) are NumPy here; the device's merged run
    (_lib.DeviceMergedRun) offers the same four computed where it lives.
    logz_realizations / logz_error / jitter_run / realization / reweight
    (errors.Errors) likewise: the same function of (seed, realization) here
    in NumPy as there on the device; so are the strand bootstrap's
    bootstrap_realizations / resample_run / simulate_run /
    logz_error_sampling / logz_error_total, which need samples_run and
    samples_id; and kld_realizations / kld_error / weight_function /
    stopping_function."""
    __getattr__ = dict.get

    def _err_logl(self):
        return np.asarray(self["logl"], dtype=np.float64)

    def _err_realize(self, seed, first, nreal, jitter, logrwt, means):
        return realize_host(self["logl"], self["samples_n"], self.get("samples"), seed, first, nreal, jitter,
                            logrwt, means)

    def _err_field(self, seed, real, jitter, logrwt, field, first, count):
        return realization_host(self["logl"], self["samples_n"], seed, real, jitter, logrwt, field, first, count)

    def _err_strands(self):
        """(strand key run * nlive + slot, final-live flag, number of strands) of every point."""
        if self.get("samples_run") is None or self.get("samples_id") is None:
            raise ValueError("the strand bootstrap needs the points' bookkeeping: merge with dead_id / dead_it / "
                             "dead_nc / live_it (samples_run and samples_id)")
        if self.get("samples_batch") is not None:
            # (strands are read off a live count that only falls: S = n[0], a final point wherever it drops; on a run
            # with batches n rises where a batch joins, and both would be wrong)
            raise ValueError("the strand bootstrap is not defined here for a run that carries dynamic batches "
                             "(dynamic.merge_batch): use the volume realizations (error='jitter')")
        n = np.asarray(self["samples_n"], dtype=np.int64)
        run = np.asarray(self["samples_run"], dtype=np.int64)
        S, R = int(n[0]), int(run.max()) + 1
        final = np.concatenate([n[:-1] - n[1:], [1]]).astype(bool)  # the live count drops after a final point
        return run * (S // R) + np.asarray(self["samples_id"], dtype=np.int64), final, S

    def _err_bootstrap(self, seed, first, nboot, jitter, mult, means):
        strand, final, S = self._err_strands()
        return bootstrap_host(self["logl"], strand, final, S, self.get("samples"), seed, first, nboot, jitter, mult,
                              means)

    def _err_bootstrap_run(self, seed, boot, jitter, mult):
        strand, final, S = self._err_strands()
        return bootstrap_run_host(self["logl"], strand, final, S, seed, boot, jitter, mult)

    def _err_kld(self, seed, first, n, mode, mult):
        if mode == 0:
            kld, lz = kld_host(self["logl"], self["samples_n"], self["logwt"], self["logz"][-1], seed, first, n)
            return kld, lz, np.full(len(kld), len(self["logl"]), dtype=np.int64)
        strand, final, S = self._err_strands()
        return kld_bootstrap_host(self["logl"], strand, final, S, self["logwt"], self["logz"][-1], seed, first, n,
                                  mode == 2, mult)

    def _err_kld_run(self, seed, index, mode, mult, first, count):
        if mode == 0:
            out = kld_run_host(self["logl"], self["samples_n"], self["logwt"], self["logz"][-1], seed, index)
        else:
            strand, final, S = self._err_strands()
            out = kld_bootstrap_run_host(self["logl"], strand, final, S, self["logwt"], self["logz"][-1], seed, index,
                                         mode == 2, mult)
        first = int(first)
        count = len(out) - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > len(out):
            raise ValueError(f"[{first}, {first + count}) of {len(out)} points")
        return np.ascontiguousarray(out[first:first + count])

    def _err_weights(self, pfrac):
        return weights_host(self["logl"], self["logvol"], self["logz"], self["samples_n"], self.importance_weights(),
                            pfrac)

    def _err_weight_function(self, pfrac, maxfrac, pad):
        i0, i1 = weight_indices(self._err_weights(pfrac)[2], maxfrac)
        logl = self["logl"]
        return weight_bounds(i0, i1, pad, len(logl), lambda k: logl[k]), (i0, i1)

    def _err_summary(self):
        """(logzerr, Kish's effective sample size) of the run (the reference's get_neff_from_logwt)."""
        w = np.exp(self["logwt"] - np.max(self["logwt"]))
        return float(self["logzerr"][-1]), float(w.sum() ** 2 / (w * w).sum())

    def batch_seeds(self, logl_min, nlive_new, strands, seed, first=0, want_rows=True, want_keys=False):
        """The start points of `strands` strands of one dynamic batch as a pure function of (seed, strand, point):
        seeds.batch_seeds_host on this run's columns, the mirror of _lib.DeviceMergedRun.batch_seeds.  dict(prior, idx,
        keys, logl_min, vol_idx, start, lo, count, n_pos) and, with want_rows, seed_u / seed_logl (samples_u and logl at
        idx)."""
        from .seeds import batch_seeds_host
        out = batch_seeds_host(self["logl"], self["logvol"], self["logz"], self["information"], self["logzerr"], logl_min,
                               nlive_new, seed, strands, first)
        if not want_keys:
            out["keys"] = None
        if want_rows:
            has = out["idx"] is not None and self.get("samples_u") is not None
            out["seed_u"] = np.asarray(self["samples_u"])[out["idx"]] if has else None
            out["seed_logl"] = np.asarray(self["logl"])[out["idx"]] if out["idx"] is not None else None
        return out

    def importance_weights(self):
        """Normalised posterior weights exp(logwt - logz[-1])."""
        w = np.exp(self["logwt"] - self["logz"][-1])
        return w / w.sum()

    @property
    def ndim(self):
        return self["samples"].shape[1]

    def _column(self, c):
        if not 0 <= c < self.ndim:
            raise ValueError(f"column {c} outside [0, {self.ndim})")
        return self["samples"][:, c]

    def _quantile(self, q, cols):
        """utils.quantile (utils.py:1190-1234) with a stable argsort; q = 0 and q = 1 are the column's minimum and
        maximum exactly (np.interp's ends wherever the first weight of the order is positive)."""
        if not len(q) or not ((q >= 0.0) & (q <= 1.0)).all():  # (NaN fails both)
            raise ValueError("Quantiles must be between 0. and 1.")
        w = self.importance_weights()
        out = np.empty((len(cols), len(q)))
        for i, c in enumerate(cols):
            x = self._column(c)
            idx = np.argsort(x, kind="stable")
            cdf = np.cumsum(w[idx])[:-1]
            cdf /= cdf[-1]
            out[i] = np.interp(q, np.append(0, cdf), x[idx])
            # the ends as the device gives them: np.interp returns the LAST point of cdf 0 at q = 0, which is not the
            # minimum where the first weights of the order are 0.0 (a run that spans thousands of nats)
            out[i, q == 0.0], out[i, q == 1.0] = x[idx[0]], x[idx[-1]]
        return out

    def _hist1d(self, cols, edges, weighted, ranges=None):
        w = self.importance_weights() if weighted else None
        if ranges is None:
            return np.array([np.histogram(self._column(c), bins=e, weights=w)[0] for c, e in zip(cols, edges)],
                            dtype=np.float64)
        # equal-width bins: NumPy sums each bin on its own there (its explicit-edge form differences a cumulative sum)
        return np.array([np.histogram(self._column(c), bins=edges.shape[1] - 1, range=tuple(r), weights=w)[0]
                         for c, r in zip(cols, ranges)], dtype=np.float64)

    def _hist2d(self, pairs, xedges, yedges, weighted):
        w = self.importance_weights() if weighted else None
        return np.array([np.histogram2d(self._column(i), self._column(j), bins=(xe, ye), weights=w)[0]
                         for (i, j), xe, ye in zip(pairs, xedges, yedges)], dtype=np.float64)


def merge_static_runs(dead_logl, niter, live_logl, dead_u=None, live_u=None,
                      prior_transform=None, ncall=None, dead_id=None, dead_it=None,
                      dead_nc=None, live_it=None, live_id=None):
    """Combine R static runs of equal, constant nlive into ONE run with R*nlive
    live points -- what the reference's utils.merge_runs / _merge_two
    (utils.py:1817-1900, 2000-2226) produce for such runs.

    Every point (a run's dead points in death order, then its final live points
    in ascending log-likelihood) carries the number of live points its own run
    had when it died (N for dead points; N, N-1, ..., 1 for the final ones);
    the merged sequence is ordered by log-likelihood (stable) and each point
    shrinks the prior volume by n/(n+1) with n the summed live count; weights,
    ln Z, information and var[ln Z] follow utils.compute_integrals
    (utils.py:1411-1467).

    dead_logl: (R, >=max niter), niter: (R,), live_logl: (R, N) in slot order;
    dead_u: (R, >=max niter, D) and live_u: (R, N, D) optional (posterior
    samples); prior_transform: optional callable mapping an (n, D) array of
    unit-cube points to parameters (gives `samples`).

    dead_id / dead_it / dead_nc: (R, >=max niter) and live_it: (R, N) optional
    (together): the per-point bookkeeping the reference's runs carry -- live
    slot, iteration at which the point was proposed, likelihood calls spent on
    its replacement (sampler.py:1165-1182; the final live points have id = their
    slot and nc = 1, sampler.py:870-890) -- which _merge_two copies point by
    point into samples_id / samples_it / ncall (utils.py:2154-2156, 2196-2207).
    live_id: (R, N) slots of the rows of live_logl when they are not in slot order.

    Returns a MergedRun with niter, logl, logvol, logwt, logz, logzerr,
    information (all per point, cumulative where the reference's are),
    samples_n, samples_run (run index of each point), samples_seq (index within
    its run's own sequence), with coordinates given samples_u / samples, and with
    the per-point bookkeeping given samples_id, samples_it and ncall (array; its
    sum replaces the `ncall` argument in eff = 100 niter / sum(ncall))."""
    from .nested import _integrate_full
    dead_logl = np.asarray(dead_logl)
    live_logl = np.asarray(live_logl)
    R, N = live_logl.shape
    ls, ns, rs, its, us = [], [], [], [], []
    point_info = dead_id is not None
    ids, bits, ncs = [], [], []
    for r in range(R):
        k = int(niter[r])
        d = dead_logl[r, :k]
        lo = np.argsort(live_logl[r], kind="stable")
        ls.append(np.concatenate([d, live_logl[r][lo]]))
        # change of this run's live count AFTER each of its points dies
        ns.append(np.concatenate([np.zeros(k), -np.ones(N)]))
        rs.append(np.full(k + N, r, dtype=np.int64))
        its.append(np.arange(k + N, dtype=np.int64))
        if dead_u is not None:
            us.append(np.concatenate([np.asarray(dead_u[r][:k]),
                                      np.asarray(live_u[r])[lo]]))
        if point_info:
            ids.append(np.concatenate([np.asarray(dead_id[r][:k], dtype=np.int64),
                                       lo if live_id is None else np.asarray(live_id[r], dtype=np.int64)[lo]]))
            bits.append(np.concatenate([np.asarray(dead_it[r][:k], dtype=np.int64),
                                        np.asarray(live_it[r], dtype=np.int64)[lo]]))
            ncs.append(np.concatenate([np.asarray(dead_nc[r][:k], dtype=np.int64),
                                       np.ones(N, dtype=np.int64)]))
    logl = np.concatenate(ls)
    dn = np.concatenate(ns)
    order = np.argsort(logl, kind="stable")
    logl, dn = logl[order], dn[order]
    nlive_at = R * N + np.concatenate([[0.], np.cumsum(dn)[:-1]])
    logvol = -np.cumsum(np.log((nlive_at + 1.) / nlive_at))
    logwt, logz, h, logzvar = _integrate_full(logl, logvol)
    out = MergedRun(niter=len(logl), logl=logl, logvol=logvol, logwt=logwt,
                    logz=logz, logzerr=np.sqrt(logzvar), information=h,
                    samples_n=nlive_at.astype(np.int64),
                    samples_run=np.concatenate(rs)[order],
                    samples_seq=np.concatenate(its)[order])
    if point_info:
        out["samples_id"] = np.concatenate(ids)[order]
        out["samples_it"] = np.concatenate(bits)[order]
        out["ncall"] = np.concatenate(ncs)[order]
        out["eff"] = 100. * len(logl) / float(out["ncall"].sum())
    elif ncall is not None:
        out["ncall"] = int(np.sum(ncall))
        out["eff"] = 100. * len(logl) / out["ncall"]
    if us:
        out["samples_u"] = np.concatenate(us)[order]
        if prior_transform is not None:
            out["samples"] = np.asarray(prior_transform(out["samples_u"]))
    return out


def merge_logz(dead_logl, niter, live_logl):
    """(logz, logzerr) of the merged run (see merge_static_runs)."""
    m = merge_static_runs(dead_logl, niter, live_logl)
    return float(m["logz"][-1]), float(m["logzerr"][-1])


def run_ensemble_merged(prob, runs, nlive=2000, queue_size=512, entropy=(21,),
                        max_iter=None, merge='host', release=True, **kw):
    """`runs` static runs on the device (dh_ns_ensemble) merged into one run
    with posterior samples: the single-process form of BASELINE C5's
    "gather of logZ / posterior samples".

    merge='host' (default): every run's points come to the host and
    `merge_static_runs` combines them; returns a MergedRun.
    merge='device': the ensemble stays on the device (ns_ensemble(keep=True))
    and the device combiner merges it there (Context.merge_kept); returns the
    DeviceMergedRun -- summary, field(), mean_and_cov(), resample_equal(),
    to_merged_run() -- with only what is asked for crossing to the host.
    The kept ensemble is released once merged; the merged run stays on the
    device until its release() or the context's next merge.
    release=False (merge='device' only) keeps the ensemble instead, so that it
    can be taken further (Context.ns_continue) and merged again
    (Context.merge_kept); runs that are not over (status 1) are then no error.
    Either way the per-run records are under ["runs"]."""
    if merge not in ('host', 'device'):
        raise ValueError(f"run_ensemble_merged: merge={merge!r} (one of 'host', 'device')")
    from .backend import get_backend
    be = get_backend()
    if max_iter is None:
        max_iter = 80 * nlive  # > nlive * (H + ln(1/dlogz)) for the benchmark problems
    if not release and merge != 'device':
        raise ValueError("run_ensemble_merged: release=False needs merge='device' (there is no kept ensemble otherwise)")
    if merge == 'device':
        r = be.ns_ensemble(prob, runs, nlive, queue_size, entropy=entropy,
                           max_iter=max_iter, want_samples=False, keep=True, **kw)
        if ((r["status"] != 0) if release else (r["status"] < 0)).any():
            if release:
                be.release_kept()
            raise RuntimeError(f"ns_ensemble: runs failed, status {r['status']}")
        try:
            m = be.merge_kept(prob)
        finally:
            if release:
                be.release_kept()  # the merged run stands alone: the ensemble's own allocation goes back at once
        m["runs"] = r
        return m
    r = be.ns_ensemble(prob, runs, nlive, queue_size, entropy=entropy,
                       max_iter=max_iter, want_samples=True, **kw)
    if (r["status"] != 0).any():
        raise RuntimeError(f"ns_ensemble: runs failed, status {r['status']}")

    def ptform(u):
        return be.problem_eval(prob, u)[0]
    m = merge_static_runs(r["dead_logl"], r["niter"], r["live_logl"],
                          r["dead_u"], r["live_u"], prior_transform=ptform,
                          dead_id=r["dead_id"], dead_it=r["dead_it"], dead_nc=r["dead_nc"],
                          live_it=r["live_it"])
    m["runs"] = r
    return m


def gather_and_merge(points_per_run, nlive, world=1, rank=0, dist=None,
                     device=None, prior_transform=None, ncall=None):
    """The sharded form of the combiner (north star: "gather of logZ / posterior
    samples"): every rank contributes, per local run, ONE array of rows
    [logl, is_final_live, id, it, nc, u_0 .. u_{D-1}] (`run_rows`: dead points in
    death order, then the final live points in any order; id = -1: no per-point
    bookkeeping); the rows travel in the ragged all-gather
    (`gather_ragged`: counts + padded rows, RCCL on GPUs, gloo on CPU) and every
    rank merges all runs with `merge_static_runs`.  Returns the MergedRun."""
    allruns = gather_ragged(points_per_run, world, rank, dist=dist, device=device)
    R = len(allruns)
    d = allruns[0].shape[1] - 5
    nit = np.array([int((a[:, 1] == 0).sum()) for a in allruns])
    dead_l = np.zeros((R, max(1, nit.max())))
    dead_u = np.zeros((R, max(1, nit.max()), d))
    dead_i = np.zeros((3, R, max(1, nit.max())), dtype=np.int64)
    live_l = np.zeros((R, nlive))
    live_u = np.zeros((R, nlive, d))
    live_i = np.zeros((2, R, nlive), dtype=np.int64)
    for i, a in enumerate(allruns):
        dmask = a[:, 1] == 0
        dead_l[i, :nit[i]] = a[dmask, 0]
        dead_u[i, :nit[i]] = a[dmask, 5:]
        dead_i[:, i, :nit[i]] = a[dmask, 2:5].T
        live_l[i] = a[~dmask, 0]
        live_u[i] = a[~dmask, 5:]
        live_i[:, i] = a[~dmask, 2:4].T
    info = {}
    if all((a[:, 2] >= 0).all() for a in allruns):
        info = dict(dead_id=dead_i[0], dead_it=dead_i[1], dead_nc=dead_i[2], live_id=live_i[0], live_it=live_i[1])
    if ncall is not None and dist is not None:
        import torch
        t = torch.tensor([float(np.sum(ncall))], dtype=torch.float64)
        if device is not None:
            t = t.to(device)
        dist.all_reduce(t)
        ncall = [float(t.item())]
    return merge_static_runs(dead_l, nit, live_l, dead_u, live_u,
                             prior_transform=prior_transform, ncall=ncall, **info)


def run_rows(dead_logl, dead_u, live_logl, live_u, dead_id=None, dead_it=None, dead_nc=None, live_it=None):
    """One run as the row block `gather_and_merge` expects (live points in slot order)."""
    k, n = len(dead_logl), len(live_logl)
    out = np.empty((k + n, 5 + np.shape(live_u)[1]))
    out[:k, 0], out[k:, 0] = dead_logl, live_logl
    out[:k, 1], out[k:, 1] = 0., 1.
    if dead_id is None:
        out[:, 2:5] = -1.
    else:
        out[:k, 2], out[k:, 2] = dead_id, np.arange(n)
        out[:k, 3], out[k:, 3] = dead_it, live_it
        out[:k, 4], out[k:, 4] = dead_nc, 1.
    out[:k, 5:], out[k:, 5:] = dead_u, live_u
    return out


def run_ensemble_merged_sharded(prob, total_runs, base_seed=21, world=1, rank=0,
                                dist=None, device=None, nlive=2000,
                                queue_size=512, max_iter=None, **kw):
    """BASELINE C5 end to end: this rank's shard of `total_runs` device-resident
    runs (dh_ns_ensemble with coordinates), the ragged gather of every run's
    points, and the merged posterior / evidence on every rank."""
    from .backend import get_backend
    be = get_backend()
    mine = shard_runs(total_runs, world, rank)
    if max_iter is None:
        max_iter = 80 * nlive
    rows, ncall, nbad = [], 0, 0
    r, raised = None, None
    if len(mine):
        try:
            r = be.ns_ensemble(prob, len(mine), nlive, queue_size,
                               entropy=np.atleast_1d(base_seed), first_run=mine.start,
                               max_iter=max_iter, want_samples=True, **kw)
            nbad = int((r["status"] != 0).sum())
        except Exception as e:  # this rank still joins the all-reduce below, then re-raises
            raised = e
            nbad = len(mine)
    # every rank learns of a failure before anyone leaves the collective sequence (see
    # run_ensemble_device): one all-reduce of the failure count, then raise everywhere
    if dist is not None:
        import torch
        t = torch.tensor([float(nbad)], dtype=torch.float64)
        if device is not None:
            t = t.to(device)
        dist.all_reduce(t)
        nbad_all = int(t.item())
    else:
        nbad_all = nbad
    if raised is not None:
        raise raised
    if nbad_all:
        raise RuntimeError(f"ns_ensemble: {nbad_all} run(s) of the ensemble failed"
                           + (f", local status {r['status']}" if nbad else ""))
    if len(mine):
        ncall = int(r["ncall"].sum())
        for i in range(len(mine)):
            k = int(r["niter"][i])
            rows.append(run_rows(r["dead_logl"][i, :k], r["dead_u"][i, :k],
                                 r["live_logl"][i], r["live_u"][i], r["dead_id"][i, :k],
                                 r["dead_it"][i, :k], r["dead_nc"][i, :k], r["live_it"][i]))

    def ptform(u):
        return be.problem_eval(prob, u)[0]
    return gather_and_merge(rows, nlive, world, rank, dist=dist, device=device,
                            prior_transform=ptform, ncall=[ncall])


def run_ensemble_checkpointed(prob, runs, nlive=2000, queue_size=512, checkpoint_file=None, checkpoint_fills=256,
                              resume=False, max_legs=None, dlogz=0.01, maxiter=None, maxcall=None, logl_max=None,
                              add_live=True, want_dead_logl=False, want_samples=False, **kw):
    """Context.ns_ensemble in legs of `checkpoint_fills` fills with the ensemble saved to `checkpoint_file` after every
    leg (Context.ns_save: written beside the file and renamed, so an interrupted save leaves the previous one) -- the
    resident loop's form of run_nested(checkpoint_file=..., resume=True).  A leg ends by max_fills (its runs have
    status 1 in between), the last one by the stop rules; with PCG64 streams, and with Philox streams too (the legs
    end at fill boundaries), the result is bit for bit that of ONE ns_ensemble call with the same arguments.
    resume=True starts from the file if it exists (the problem must be the one the file was written for; the other
    arguments of the first leg then come from the file).  max_legs stops after that many legs (None: until every run
    is over) -- what an interruption leaves behind, for tests and time-sliced jobs.  Returns what ns_ensemble returns;
    the ensemble is released at the end unless max_legs cut the run short."""
    import os
    from .backend import get_backend
    if checkpoint_file is None:
        raise ValueError("run_ensemble_checkpointed: checkpoint_file is required")
    if checkpoint_fills < 1:
        raise ValueError("run_ensemble_checkpointed: checkpoint_fills must be at least 1")
    be = get_backend()
    crit = dict(dlogz=dlogz, maxiter=maxiter, maxcall=maxcall, logl_max=logl_max, add_live=add_live)
    want = dict(want_dead_logl=want_dead_logl, want_samples=want_samples)
    legs = 0
    if resume and os.path.exists(checkpoint_file):
        be.ns_load(prob, checkpoint_file)
        r = None
    else:
        r = be.ns_ensemble(prob, runs, nlive, queue_size, max_fills=checkpoint_fills, keep=True, **crit, **want, **kw)
        be.ns_save(checkpoint_file)
        legs = 1
    while (r is None or (r["status"] == 1).any()) and (max_legs is None or legs < max_legs):
        r = be.ns_continue(max_fills=checkpoint_fills, **crit, **want)
        be.ns_save(checkpoint_file)
        legs += 1
    if r is not None and not (r["status"] == 1).any():
        be.release_kept()
    return r
