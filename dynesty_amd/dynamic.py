"""Dynamic nested sampling on the device-resident loop: batches of strands started inside a finished run.

The reference's DynamicSampler adds a batch in three steps (dynamicsampler.py): _configure_batch_sampler (:300-622)
chooses nlive_new points of the saved run above the batch's lower ln L bound and samples a fresh live set from them,
sample_batch (:1228-1465) runs that live set up to the upper bound, and combine_runs (:1467-1609) folds the new points
into the saved run.  Here

  batch_seed   restates the choice of the start points (NumPy, host; the same calls on the same bits give the
               reference's indices),
  Context.ns_batch (dh_ns_batch, csrc/ns.hip) samples the live set and runs the strands on the device,
  merge_batch  restates combine_runs (NumPy, host), one strand at a time,
  merge_strands  folds all strands of a batch in one pass (NumPy, host): the same result as merge_batch strand after
               strand, with one integration of the whole run; the host mirror of the device's fold (dh_merged_fold,
               csrc/merge_fold.hip),
  fold_batch   folds an ns_batch / ns_ensemble result into a MergedRun (merge_strands) or a DeviceMergedRun (the
               device's fold),
  run_dynamic  is the loop around them: weight_function -> batch_seed x strands -> ns_batch -> merge_batch (merge='host')
               or fold_batch on the device (merge='device') -> stopping_function.  With seeds='device' the seeds of all
               strands are chosen where the merged run lives (DeviceMergedRun.batch_seeds, csrc/merge_seed.hip; the
               NumPy mirror is seeds.py); the chosen rows come back with the indices and go into ns_batch.

Where this departs from the reference: a batch needs nlive_new seeds of positive weight (the reference goes on with
fewer live points; batch_seed raises ValueError); the device's departures (a)-(d) are listed in include/dynhip.h.
"""
import math
import time

import numpy as np

from .ensemble import MergedRun, run_ensemble_merged

__all__ = ["batch_seed", "merge_batch", "merge_strands", "fold_batch", "single_run", "strand_of", "run_dynamic"]


def _base_columns(base):
    """(logl, logvol) of the saved run; from a DeviceMergedRun these two columns are all that crosses PCIe here."""
    if hasattr(base, "field") and not isinstance(base, MergedRun):
        return base.field("logl"), base.field("logvol")
    return np.asarray(base["logl"], dtype=np.float64), np.asarray(base["logvol"], dtype=np.float64)


def _base_row(base, i):
    """(logvol, logz, h, logzvar, logl) of point i of the saved run."""
    if hasattr(base, "field") and not isinstance(base, MergedRun):
        one = {k: float(base.field(k, i, 1)[0]) for k in ("logvol", "logz", "information", "logzerr", "logl")}
    else:
        one = {k: float(np.asarray(base[k])[i]) for k in ("logvol", "logz", "information", "logzerr", "logl")}
    return one["logvol"], one["logz"], one["information"], one["logzerr"] ** 2, one["logl"]


def batch_seed(base, logl_bounds, nlive_new, rstate, columns=None):
    """The start points of one strand of a batch (dynamicsampler.py:394-416, 457-533, 606-610).

    columns: (logl, logvol) of the saved run where the caller holds them already -- the strands of one batch share one
    download of a DeviceMergedRun's two columns; default: read from `base`.

    base: a MergedRun or a DeviceMergedRun (the saved run); logl_bounds: (logl_min, logl_max) or None for the
    reference's default, (-inf, ln L at the last index with logvol < logvol[-1] + ln nlive_new); rstate: a
    numpy Generator -- the one call made on it is rstate.choice(subset0, size=nlive_new, p=..., replace=False), the
    reference's.  For R strands call this R times on one rstate, in strand order.

    Returns a dict: prior (True: every saved ln L lies above logl_min -- or the boundary moved below the first saved
    point -- and the batch starts from the prior), idx (the nlive_new chosen indices into the saved run; None where no
    choice was made), logl_min / logl_max (logl_min moved down where fewer than nlive_new points lay above it), vol_idx
    (the strand joins the saved run after its first vol_idx points) and start = (logvol, logz, h, logzvar, logl) of
    the saved run at vol_idx - 1 (None for a batch from the prior).

    Raises RuntimeError when no saved point lies above logl_min (the reference's type), ValueError when fewer than
    nlive_new points of positive weight are available (the reference goes on with fewer live points; this does not)."""
    nlive_new = int(nlive_new)
    saved_logl, saved_logvol = _base_columns(base) if columns is None else columns
    if logl_bounds is None:
        pos = np.nonzero(saved_logvol < (saved_logvol[-1] + np.log(nlive_new)))[0]
        pos = pos[-1] if len(pos) > 0 else len(saved_logl) - 1
        logl_min, logl_max = -np.inf, saved_logl[pos]
    else:
        logl_min, logl_max = logl_bounds
    if np.all(saved_logl > logl_min):
        # (the bounds stay as given and vol_idx is the reference's own, :606-610; a batch from the prior uses neither)
        vol_idx = 0 if logl_min == -np.inf else int(np.argmin(np.abs(saved_logl - logl_min))) + 1
        return dict(prior=True, idx=None, logl_min=float(logl_min), logl_max=float(logl_max), vol_idx=vol_idx,
                    start=None)
    subset0 = np.nonzero(saved_logl > logl_min)[0]
    if len(subset0) == 0:
        raise RuntimeError("Could not find live points in the required logl interval: "
                           f"logl_min {logl_min}, logl_bounds {logl_bounds}, saved ln L max {saved_logl.max()}")
    if len(subset0) < nlive_new:
        if len(saved_logl) < nlive_new:
            subset0 = np.arange(len(saved_logl))
        else:
            # the boundary moves down to collect nlive_new points
            subset0 = np.arange(subset0[-1] - nlive_new + 1, subset0[-1] + 1)
        logl_min = saved_logl[subset0[0] - 1] if subset0[0] > 0 else -np.inf
    cur_log_uniwt = saved_logvol[subset0]
    cur_uniwt = np.exp(cur_log_uniwt - cur_log_uniwt.max())
    cur_uniwt = cur_uniwt / cur_uniwt.sum()  # (linear domain: the sum must be 1 for Generator.choice)
    n_pos_weight = int((cur_uniwt > 0).sum())
    if n_pos_weight < nlive_new:
        raise ValueError(f"batch_seed: {n_pos_weight} saved points of positive weight above ln L = {logl_min}, "
                         f"nlive_new = {nlive_new} are needed (a batch on fewer live points is not supported)")
    subset = rstate.choice(subset0, size=nlive_new, p=cur_uniwt, replace=False)
    if logl_min == -np.inf:
        # (the boundary moved below the first saved point: the seeds stand, the strand's volume starts at the prior's)
        return dict(prior=True, idx=np.asarray(subset, dtype=np.int64), logl_min=-np.inf, logl_max=float(logl_max),
                    vol_idx=0, start=None)
    vol_idx = int(np.argmin(np.abs(saved_logl - logl_min))) + 1
    return dict(prior=False, idx=np.asarray(subset, dtype=np.int64), logl_min=float(logl_min),
                logl_max=float(logl_max), vol_idx=vol_idx, start=_base_row(base, vol_idx - 1))


def strand_of(out, r, nlive_new, prior_transform=None):
    """Strand r of a Context.ns_batch / ns_ensemble result (want_samples=True) as merge_batch takes it: its dead points
    in death order, then its final live points lowest first; n = nlive_new for the dead points and nlive_new, ..., 1
    for the final ones; id = live slot, it, nc (1 for the final points) as the loop records them."""
    k, N = int(out["niter"][r]), int(nlive_new)
    lo = np.argsort(out["live_logl"][r], kind="stable")
    s = dict(logl=np.concatenate([out["dead_logl"][r, :k], out["live_logl"][r][lo]]),
             n=np.concatenate([np.full(k, N, dtype=np.int64), np.arange(N, 0, -1, dtype=np.int64)]),
             id=np.concatenate([out["dead_id"][r, :k].astype(np.int64), lo.astype(np.int64)]),
             it=np.concatenate([out["dead_it"][r, :k].astype(np.int64), out["live_it"][r][lo].astype(np.int64)]),
             nc=np.concatenate([out["dead_nc"][r, :k].astype(np.int64), np.ones(N, dtype=np.int64)]),
             u=np.concatenate([out["dead_u"][r, :k], out["live_u"][r][lo]]))
    if prior_transform is not None:
        s["v"] = np.asarray(prior_transform(s["u"]))
    return s


def _batch_logvol(logl, n, logvol_init=0.0):
    """combine_runs' volume pass (dynamicsampler.py:1554-1583): ln((n + 1) / n) per point, except that a run of equal
    ln L shrinks the volume in equal LINEAR steps of X / (n + 1), with X and n taken where the run starts."""
    logl = np.asarray(logl, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    steps = np.log((n + 1.) / n)
    if not (logl[1:] == logl[:-1]).any():
        return logvol_init - np.cumsum(steps)
    out = np.empty(len(logl))
    tie_next = np.concatenate([logl[1:] == logl[:-1], [False]])
    plateau_mode, counter, plogdvol, logvol = False, 0, 0.0, float(logvol_init)
    for i in range(len(logl)):
        if not plateau_mode and tie_next[i]:
            nplateau = int((logl[i:] == logl[i]).sum())
            if nplateau > 1:
                counter = nplateau
                plogdvol = logvol + math.log(1. / (n[i] + 1))
                plateau_mode = True
        if not plateau_mode:
            logvol -= steps[i]
        else:
            logvol = logvol + math.log1p(-math.exp(plogdvol - logvol))
        out[i] = logvol
        if plateau_mode:
            counter -= 1
            if counter == 0:
                plateau_mode = False
    return out


def merge_batch(base, strand, logl_min, logl_max):
    """combine_runs (dynamicsampler.py:1467-1609): one strand folded into the saved run.

    base: a MergedRun (merge_static_runs' fields; samples_id must identify a strand of the whole run -- run_dynamic
    renumbers a merged ensemble's per-run slots); strand: dict(logl, n, id, it, nc[, u, v]) in the strand's own order
    (strand_of).  The walk over both sequences takes the saved point on ties; a point's n is n_saved + n_new of the two
    current heads while the saved head's ln L is above logl_min, else n_saved (an exhausted side counts 0, its head
    +inf); the strand's ids are shifted by max(base id) + 1; volumes by the plateau rule; the integrals are recomputed
    over the whole run.  Several strands fold one after the other, in strand order, as repeated add_batch calls would.

    Returns a MergedRun with merge_static_runs' fields plus samples_batch (0 = the base run), batch_nlive and
    batch_bounds (entry 0: the base run, then one entry per folded strand).  On such a run the strand bootstrap
    (bootstrap_realizations, resample_run, simulate_run, error='resample' | 'simulate') raises ValueError: it reads
    strands off a live count that only falls.  The volume realizations (error='jitter') work."""
    from .nested import _integrate_full
    sl = np.asarray(base["logl"], dtype=np.float64)
    nl = np.asarray(strand["logl"], dtype=np.float64)
    sn = np.asarray(base["samples_n"], dtype=np.int64)
    nn = np.asarray(strand["n"], dtype=np.int64)
    ns_, nw = len(sl), len(nl)
    if nw == 0:
        raise ValueError("No new samples are currently saved.")
    # the two-pointer walk on sorted sequences is the stable merge with the saved point first on ties
    src_new = np.concatenate([np.zeros(ns_, dtype=bool), np.ones(nw, dtype=bool)])
    order = np.argsort(np.concatenate([sl, nl]), kind="stable")
    from_new = src_new[order]
    idx_new = np.cumsum(from_new) - from_new          # strand points consumed before each output position
    idx_saved = np.arange(ns_ + nw) - idx_new         # saved points consumed before it
    head_l = np.concatenate([sl, [np.inf]])[idx_saved]
    head_ns = np.concatenate([sn, [0]])[idx_saved]
    head_nn = np.concatenate([nn, [0]])[idx_new]
    n = np.where(head_l > logl_min, head_ns + head_nn, head_ns)
    logl = np.concatenate([sl, nl])[order]
    logvol = _batch_logvol(logl, n)
    logwt, logz, h, logzvar = _integrate_full(logl, logvol)
    # (a run that holds no batch yet counts as the reference's base entry: its own live count, unbounded)
    # (either may come back as a NumPy array from a run rebuilt out of saved arrays: no truth test on them)
    b_nlive, b_bounds = base.get("batch_nlive"), base.get("batch_bounds")
    b_nlive = [int(sn.max())] if b_nlive is None or len(b_nlive) == 0 else [int(x) for x in b_nlive]
    b_bounds = ([(-np.inf, np.inf)] if b_bounds is None or len(b_bounds) == 0
                else [(float(lo), float(hi)) for lo, hi in b_bounds])
    nbatch = len(b_nlive) - 1
    sbatch = base.get("samples_batch")
    sbatch = np.zeros(ns_, dtype=np.int64) if sbatch is None else np.asarray(sbatch, dtype=np.int64)
    sid = np.asarray(base["samples_id"], dtype=np.int64)
    out = MergedRun(niter=len(logl), logl=logl, logvol=logvol, logwt=logwt, logz=logz, logzerr=np.sqrt(logzvar),
                    information=h, samples_n=n.astype(np.int64),
                    samples_id=np.concatenate([sid, np.asarray(strand["id"], dtype=np.int64) + sid.max() + 1])[order],
                    samples_batch=np.concatenate([sbatch, np.full(nw, nbatch + 1, dtype=np.int64)])[order],
                    batch_nlive=b_nlive + [int(nn.max())],
                    batch_bounds=b_bounds + [(float(logl_min), float(logl_max))])

    def both(key, skey, dtype=np.int64):
        b = base.get(key)
        if b is None or skey not in strand:
            return
        out[key] = np.concatenate([np.asarray(b, dtype=dtype), np.asarray(strand[skey], dtype=dtype)])[order]
    both("samples_it", "it")
    both("ncall", "nc")
    both("samples_u", "u", np.float64)
    both("samples", "v", np.float64)
    if base.get("samples_run") is not None:
        out["samples_run"] = np.concatenate([np.asarray(base["samples_run"], dtype=np.int64),
                                             np.zeros(nw, dtype=np.int64)])[order]
    # index within the point's own sequence: the strand's counts on from its own first point
    out["samples_seq"] = np.concatenate([np.asarray(base["samples_seq"], dtype=np.int64) if base.get("samples_seq")
                                         is not None else np.arange(ns_), np.arange(nw)])[order]
    if isinstance(out.get("ncall"), np.ndarray):
        out["eff"] = 100. * len(logl) / float(out["ncall"].sum())
    return out


def single_run(m):
    """A merge of static runs as ONE run, in place: a point's id names its strand in the whole run (run * nlive + slot),
    its run is 0.  nlive is read off the run itself: the first point's live count is runs * nlive.  A run that is one
    already (a single static run, a run that holds batches) comes back as it is."""
    if m.get("samples_batch") is not None or m.get("samples_run") is None:
        return m
    run = np.asarray(m["samples_run"], dtype=np.int64)
    nruns = int(run.max()) + 1 if len(run) else 1
    if m.get("samples_id") is not None:
        nlive = int(np.asarray(m["samples_n"])[0]) // nruns
        m["samples_id"] = run * nlive + np.asarray(m["samples_id"], dtype=np.int64)
    m["samples_run"] = np.zeros(len(run), dtype=np.int64)
    return m


def merge_strands(base, strands, logl_min, logl_max):
    """All strands of one batch folded into the saved run in one pass: the result of merge_batch applied strand after
    strand, in strand order, with the same bounds -- one sort and one integration of the whole run instead of one per
    strand.  base: a MergedRun as merge_batch takes it; strands: a list of strand_of dicts (n = nlive_new for the dead
    points and nlive_new, ..., 1 for the final ones).

      order  the stable order of (base, strand 0, .., strand R-1): on equal ln L the base point first, then the strands
             by index, then a strand's own order
      n      n_base at the base's next point (0 past its end) + where ln L > logl_min (strictly) the strands' heads:
             the sum of the strands' first n less one for each of their FINAL points before the position
      id     strand s shifted by the largest id so far + 1; batch = batches before + 1 + s
      ln X   _batch_logvol's plateau rule over the whole run; the integrals by _integrate_full

    Raises ValueError where merge_batch does (an empty strand; a plateau longer than the live count where it starts),
    and for a strand point at or below logl_min, which merge_batch would count without its own strand."""
    from .nested import _integrate_full
    if len(strands) < 1:
        raise ValueError("No new samples are currently saved.")
    sl = np.asarray(base["logl"], dtype=np.float64)
    sn = np.asarray(base["samples_n"], dtype=np.int64)
    ns_ = len(sl)
    nls = [np.asarray(s["logl"], dtype=np.float64) for s in strands]
    nns = [np.asarray(s["n"], dtype=np.int64) for s in strands]
    if any(len(x) == 0 for x in nls):
        raise ValueError("No new samples are currently saved.")
    nl = np.concatenate(nls)
    if not (nl > logl_min).all():
        raise ValueError(f"merge_strands: a strand point lies at or below logl_min = {logl_min}")
    nw = len(nl)
    # a strand's final points: where its live count falls (the last nn[0] points, as strand_of writes them)
    fin_new = np.concatenate([np.concatenate([x[:-1] > x[1:], [True]]) for x in nns])
    heads = int(sum(int(x[0]) for x in nns))
    order = np.argsort(np.concatenate([sl, nl]), kind="stable")
    from_new = order >= ns_
    idx_saved = np.arange(ns_ + nw) - (np.cumsum(from_new) - from_new)   # base points before each position
    fin_sorted = np.concatenate([np.zeros(ns_, dtype=bool), fin_new])[order]
    cfin = np.cumsum(fin_sorted) - fin_sorted                            # new final points before it
    logl = np.concatenate([sl, nl])[order]
    n = np.concatenate([sn, [0]])[idx_saved] + np.where(logl > logl_min, heads - cfin, 0)
    logvol = _batch_logvol(logl, n)
    logwt, logz, h, logzvar = _integrate_full(logl, logvol)
    b_nlive, b_bounds = base.get("batch_nlive"), base.get("batch_bounds")
    b_nlive = [int(sn.max())] if b_nlive is None or len(b_nlive) == 0 else [int(x) for x in b_nlive]
    b_bounds = ([(-np.inf, np.inf)] if b_bounds is None or len(b_bounds) == 0
                else [(float(lo), float(hi)) for lo, hi in b_bounds])
    nbatch = len(b_nlive) - 1
    sbatch = base.get("samples_batch")
    sbatch = np.zeros(ns_, dtype=np.int64) if sbatch is None else np.asarray(sbatch, dtype=np.int64)
    sid = np.asarray(base["samples_id"], dtype=np.int64)
    ids, top = [sid], int(sid.max())
    for s in strands:  # (the running maximum: the largest id so far, as one merge_batch after the other sees it)
        ids.append(np.asarray(s["id"], dtype=np.int64) + top + 1)
        top = int(ids[-1].max())
    out = MergedRun(niter=len(logl), logl=logl, logvol=logvol, logwt=logwt, logz=logz, logzerr=np.sqrt(logzvar),
                    information=h, samples_n=n.astype(np.int64), samples_id=np.concatenate(ids)[order],
                    samples_batch=np.concatenate([sbatch] + [np.full(len(x), nbatch + 1 + i, dtype=np.int64)
                                                             for i, x in enumerate(nls)])[order],
                    batch_nlive=b_nlive + [int(x.max()) for x in nns],
                    batch_bounds=b_bounds + [(float(logl_min), float(logl_max))] * len(strands))

    def both(key, skey, dtype=np.int64):
        b = base.get(key)
        if b is None or any(skey not in s for s in strands):
            return
        out[key] = np.concatenate([np.asarray(b, dtype=dtype)] + [np.asarray(s[skey], dtype=dtype) for s in strands])[order]
    both("samples_it", "it")
    both("ncall", "nc")
    both("samples_u", "u", np.float64)
    both("samples", "v", np.float64)
    if base.get("samples_run") is not None:
        out["samples_run"] = np.concatenate([np.asarray(base["samples_run"], dtype=np.int64),
                                             np.zeros(nw, dtype=np.int64)])[order]
    out["samples_seq"] = np.concatenate([np.asarray(base["samples_seq"], dtype=np.int64) if base.get("samples_seq")
                                         is not None else np.arange(ns_)] + [np.arange(len(x)) for x in nls])[order]
    if isinstance(out.get("ncall"), np.ndarray):
        out["eff"] = 100. * len(logl) / float(out["ncall"].sum())
    return out


def fold_batch(base, out, nlive_new, logl_min, logl_max, prior_transform=None):
    """One batch folded into the saved run: `out` is a Context.ns_batch / ns_ensemble result (want_samples=True), all of
    whose strands join.  A DeviceMergedRun is folded where it lives (Context.merged_fold, dh_merged_fold; the strands'
    arrays are uploaded, the run stays on the device; the old handle goes stale; the new points' parameters are the
    problem's the run was merged with); a MergedRun by merge_strands, with prior_transform for the new points'
    parameters.  Returns the new run, of the base's type."""
    if hasattr(base, "field") and not isinstance(base, MergedRun):
        if int(np.shape(out["live_logl"])[1]) != int(nlive_new):
            raise ValueError(f"fold_batch: strands of {np.shape(out['live_logl'])[1]} live points, nlive_new {nlive_new}")
        pt = dict(dead_id=out["dead_id"], dead_it=out["dead_it"], dead_nc=out["dead_nc"],
                  live_it=out["live_it"]) if base.have_pt else {}
        return base._live().merged_fold(base, base.prob, out["niter"], out["dead_logl"], out["live_logl"], out["dead_u"],
                                         out["live_u"], logl_min=logl_min, logl_max=logl_max, **pt)
    strands = [strand_of(out, r, nlive_new, prior_transform=prior_transform) for r in range(len(out["niter"]))]
    return merge_strands(base, strands, logl_min, logl_max)


def run_dynamic(prob, runs, nlive_init, strands, nlive_batch, maxbatch, pfrac=0.8, entropy=(21,), queue_size=None,
                maxfrac=0.8, pad=1, dlogz_init=0.01, dlogz_batch=0.01, max_iter=None, rstate=None, stop_kwargs=None,
                merge='host', seeds='host', **kw):
    """Dynamic nested sampling on one device: a base ensemble of `runs` static runs of nlive_init live points, merged;
    then up to maxbatch batches of `strands` strands of nlive_batch live points each, placed by the merged run's
    weight_function(pfrac, maxfrac, pad) and folded in by merge_batch.  After every batch
    stopping_function(**stop_kwargs) is asked; the loop ends when it says so or at maxbatch.

    entropy seeds the base ensemble; batch b (1-based) runs on entropy + (b,).  rstate: the generator of the seeds'
    weighted choice (default: np.random.default_rng(entropy words)).  **kw goes to Context.ns_ensemble and
    Context.ns_batch alike (sample, walks, slices, bound, enlarge, bootstrap, ...; PCG64 streams, 'multi' / 'single').

    merge='host' (default): the base ensemble is merged on the host and every strand folded in by merge_batch; the run
    is a MergedRun.  merge='device': the base is merged on the device (run_ensemble_merged(merge='device')) and stays
    there; per batch the saved run's logl and logvol columns cross once, the seeds' unit-cube rows by a gather, and all
    strands fold in one dh_merged_fold (fold_batch); the run is a DeviceMergedRun.  Both routes run the same strands:
    the seeds' choice and the PCG64 streams are the same functions of the same bits.

    seeds='host' (default): dynamic.batch_seed per strand, the Generator's weighted choice.  seeds='device' (with
    merge='device' only): per batch ONE DeviceMergedRun.batch_seeds chooses the seeds of all strands where the run
    lives (the same law as a pure function of a per-batch seed, SeedSequence(entropy + (b,)); rstate is not used) and
    returns their rows and ln L, gathered on the device, for ns_batch; fold_batch folds.  The logl / logvol columns do
    not cross PCIe and no gather call is made; the chosen rows come down and go back up.  A batch from the prior runs
    through ns_ensemble(logl_max=) on either route.

    Returns (the run, log): log[0] describes the base run (and holds it, merged, under "run"), log[b] batch b --
    bounds, whether it started from the prior, ncall, seed_ncall, niter (points added), seconds, and the stopping
    function's verdict after it, and which route chose the seeds."""
    from .backend import get_backend
    if merge not in ('host', 'device'):
        raise ValueError(f"run_dynamic: merge={merge!r} (one of 'host', 'device')")
    if seeds not in ('host', 'device'):
        raise ValueError(f"run_dynamic: seeds={seeds!r} (one of 'host', 'device')")
    if seeds == 'device' and merge != 'device':
        raise ValueError("run_dynamic: seeds='device' chooses the seeds where the merged run lives: it needs merge='device'")
    be = get_backend()
    entropy = tuple(int(x) for x in np.atleast_1d(entropy))
    if queue_size is None:
        queue_size = max(1, min(512, nlive_batch // 4, nlive_init // 4))
    if rstate is None:
        rstate = np.random.default_rng(list(entropy))
    stop_kwargs = dict(stop_kwargs or {})
    on_device = merge == 'device'

    def ptform(u):
        return be.problem_eval(prob, u)[0]
    t0 = time.perf_counter()
    m = run_ensemble_merged(prob, runs, nlive_init, queue_size, entropy=entropy, max_iter=max_iter, merge=merge,
                            dlogz=dlogz_init, **kw)
    base_runs = m.pop("runs")
    if not on_device:
        # one run from here on: a point's id names its strand in the WHOLE run (run * nlive + slot for the base's)
        m = single_run(m)  # (the device's first fold renumbers its base the same way)
    log = [dict(bounds=(-np.inf, np.inf), prior=True, ncall=int(base_runs["ncall"].sum()), niter=int(m.niter),
                seconds=time.perf_counter() - t0, stop=bool(m.stopping_function(**stop_kwargs)), run=m)]
    cap = max_iter if max_iter is not None else 80 * nlive_batch
    for b in range(1, int(maxbatch) + 1):
        if log[-1]["stop"]:
            break
        t0 = time.perf_counter()
        bounds = m.weight_function(pfrac=pfrac, maxfrac=maxfrac, pad=pad)
        ent = entropy + (b,)
        if seeds == 'device':
            # one call for all strands, their rows gathered on the device; the batch's seed is a function of ent
            bseed = int(np.random.SeedSequence(list(ent)).generate_state(1, np.uint64)[0])
            s0 = m.batch_seeds(bounds[0], nlive_batch, int(strands), bseed, want_rows=True)
            s0["logl_max"] = float(bounds[1])
            picked = None
        else:
            # (the device's run: its two columns cross once per batch, the seeds' rows by a gather)
            cols = _base_columns(m) if on_device else None
            picked = [batch_seed(m, bounds, nlive_batch, rstate, columns=cols) for _ in range(int(strands))]
            s0 = picked[0]
        if s0["prior"]:
            # logl_min = -inf: an ordinary ensemble of nlive_batch live points up to logl_max
            out = be.ns_ensemble(prob, int(strands), nlive_batch, queue_size, entropy=ent, max_iter=cap,
                                 want_samples=True, dlogz=dlogz_batch, logl_max=s0["logl_max"], **kw)
            seed_calls = 0
        elif seeds == 'device':
            start = np.array(list(s0["start"]) + [1.0])
            out = be.ns_batch(prob, s0["seed_u"], s0["seed_logl"], s0["logl_min"], start, queue_size,
                              logl_max=s0["logl_max"], entropy=ent, max_iter=cap, dlogz=dlogz_batch, **kw)
            seed_calls = int(out["seed_ncall"].sum())
        else:
            start = np.array(list(s0["start"]) + [1.0])  # (the merged run keeps no per-point scale: departure (d))
            if on_device:
                pick = np.concatenate([s["idx"] for s in picked])
                seed_u = m.gather(pick, "samples_u").reshape(len(picked), -1, m.ndim)
                seed_l = cols[0][pick].reshape(len(picked), -1)
            else:
                seed_u = np.stack([m["samples_u"][s["idx"]] for s in picked])
                seed_l = np.stack([m["logl"][s["idx"]] for s in picked])
            out = be.ns_batch(prob, seed_u, seed_l, s0["logl_min"], start, queue_size,
                              logl_max=s0["logl_max"], entropy=ent, max_iter=cap, dlogz=dlogz_batch, **kw)
            seed_calls = int(out["seed_ncall"].sum())
        if (out["status"] != 0).any():
            raise RuntimeError(f"run_dynamic: strands of batch {b} failed, status {out['status']}")
        if on_device:
            m = fold_batch(m, out, nlive_batch, s0["logl_min"], s0["logl_max"])
            added = int(np.sum(out["niter"])) + int(strands) * int(nlive_batch)
        else:
            added = 0
            for r in range(int(strands)):
                s = strand_of(out, r, nlive_batch, prior_transform=ptform)
                m = merge_batch(m, s, s0["logl_min"], s0["logl_max"])
                added += len(s["logl"])
        log.append(dict(bounds=(s0["logl_min"], s0["logl_max"]), prior=bool(s0["prior"]),
                        ncall=int(out["ncall"].sum()), seed_ncall=seed_calls, niter=added, seeds=seeds,
                        seconds=time.perf_counter() - t0, stop=bool(m.stopping_function(**stop_kwargs))))
    return m, log
