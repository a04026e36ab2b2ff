"""The seeds of a dynamic batch chosen on the device (csrc/merge_seed.hip, dh_merged_batch_seed;
DESIGN.md section 3.8.6) against the NumPy mirror (dynesty_amd/seeds.py): the answer's bookkeeping exactly,
the keys to 1e-12, the indices exactly wherever the mirror's keys are more than 1e-9 apart; shapes chosen to break a
tile, a block pair or a bin; reproducibility; the law on the device; the rows that come back with the choice against a
gather of the same indices, bit for bit, and a batch run from them; the refusals; and run_dynamic(seeds='device').

Two cases differ from what one would write for the host alone, because a merged run's logvol column is the device's own
and cannot be set: the law is tested on the last seven points of a merged run (weights 7 : 6 : .. : 1, smallest expected
count 2.6) against the probabilities computed from the downloaded column, and "all logvol equal" is replaced by a
boundary on a plateau of equal ln L (equal ln L does not make equal volumes)."""
import numpy as np
import pytest

import merge_cases
from test_seed_choice_cpu import chi2_of, chi2_quantile

pytestmark = pytest.mark.gpu

COLS = ("logl", "logvol", "logz", "information", "logzerr")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def prob3():
    from dynesty_amd import problems
    return problems.Problem(3, problems.LIKE_GAUSS_IID, [0.0], problems.PRIOR_AFFINE, [10.0, 0.0], name="gauss3_unnormalised")


def merged(ctx, niters, nlive, seed):
    """A synthetic merged run on the device and its columns on the host."""
    d = ctx.merge_runs(prob3(), **merge_cases.make(np.random.default_rng(seed), niters, nlive, 3))
    return d, {k: d.field(k) for k in COLS}


def compare(d, cols, logl_min, k, strands, seed, first=0, label=""):
    """One call against the mirror; returns (device answer, mirror answer)."""
    from dynesty_amd import seeds
    want = seeds.batch_seeds_host(*(cols[c] for c in COLS), logl_min, k, seed, strands, first)
    got = d.batch_seeds(logl_min, k, strands, seed, first=first, want_rows=False, want_keys=True)
    for key in ("prior", "lo", "count", "n_pos", "logl_min", "vol_idx", "start"):
        assert got[key] == want[key], (label, key, got[key], want[key])
    idx, keys = got["idx"], got["keys"]
    assert idx.shape == keys.shape == (strands, k)
    allk = seeds.seed_keys_host(cols["logvol"], seed, strands, first)
    mine = np.take_along_axis(allk, idx, axis=1)
    err = np.abs(keys - mine)
    fin = np.isfinite(mine)
    assert (keys[~fin] == mine[~fin]).all()
    worst = float(np.max(err[fin] / (1e-12 + 1e-12 * np.abs(mine[fin])))) if fin.any() else 0.0
    assert worst <= 1.0, (label, worst)
    assert (np.diff(keys, axis=1) <= 0).all(), label
    lo = got["lo"]
    sub = cols["logvol"][lo:]
    can = np.zeros(len(cols["logvol"]), dtype=bool)
    can[lo:] = sub - sub.max() >= seeds.LOG_MIN
    assert all(can[row].all() and len(set(row)) == k for row in idx), label
    # no unselected point of positive weight above the last selected key
    rest = np.where(can[None, :], allk, -np.inf)
    np.put_along_axis(rest, idx, -np.inf, axis=1)
    assert (rest.max(axis=1) <= keys[:, -1] + 1e-12).all(), label
    # the indices: the mirror's, for every strand whose mirror keys at ranks 1 .. k + 1 are more than 1e-9 apart -- here
    # all of them (checked: the cases are chosen so that the mirror exempts none)
    ranked = -np.sort(-np.where(can[None, :], allk, -np.inf), axis=1)[:, :k + 1]
    gaps = ranked[:, :-1] - ranked[:, 1:]
    with np.errstate(invalid="ignore"):  # (rank k + 1 is -inf where k = n_pos: a gap of +inf)
        clear = (gaps > 1e-9).all(axis=1)
    exempt = int((~clear).sum())
    print(f"[batch seed {label}] lo {lo} count {got['count']} n_pos {got['n_pos']} k {k} strands {strands} passes "
          f"{got['passes']}: worst key error / tolerance {worst:.3g}, exempt strands {exempt}")
    assert exempt == 0 and exempt <= 0.02 * strands
    np.testing.assert_array_equal(idx[clear], want["idx"][clear], err_msg=label)
    return got, want


@pytest.fixture(scope="module")
def small():
    """230 points on a context of their own (a context holds one merged run: the other tests' merges replace theirs)."""
    from dynesty_amd import _lib
    return merged(_lib.Context(0), [100, 90], 20, 11)


def test_small_subsets_against_the_mirror(small):
    d, cols = small
    logl, M = cols["logl"], len(cols["logl"])
    # a subset smaller than one wavefront; lo odd (the first Philox block half used) and even; k = 1; one strand and 65
    compare(d, cols, float(logl[M - 41]), 8, 5, seed=3, label="40 points")
    for lo in (181, 182):
        got, _ = compare(d, cols, float(logl[lo - 1]), 8, 65, seed=4, label=f"lo = {lo}")
        assert got["lo"] == lo
    compare(d, cols, float(logl[150]), 1, 65, seed=5, label="k = 1")
    compare(d, cols, float(logl[150]), 16, 1, seed=6, label="one strand")
    # k = count = n_pos: pure ordering; one more and the boundary moves
    got, _ = compare(d, cols, float(logl[M - 33]), 32, 3, seed=7, label="k = count")
    assert got["count"] == got["n_pos"] == 32 and all(sorted(r) == list(range(M - 32, M)) for r in got["idx"])
    got, _ = compare(d, cols, float(logl[M - 33]), 33, 3, seed=7, label="moved boundary")
    assert got["lo"] == M - 33 and got["logl_min"] == logl[M - 34]
    # the whole run: the boundary moves below the first point, a prior strand whose seeds stand
    got, _ = compare(d, cols, float(logl[M - 3]), M, 2, seed=8, label="k = M")
    assert got["prior"] and got["logl_min"] == -np.inf and got["start"] is None and got["idx"].shape == (2, M)
    # from the prior: no choice
    from dynesty_amd import seeds
    got = d.batch_seeds(float(logl[0]) - 1.0, 8, 2, 1, want_rows=False)
    want = seeds.batch_seeds_host(*(cols[c] for c in COLS), float(logl[0]) - 1.0, 8, 1, 2)
    assert got["prior"] and got["idx"] is None and {k: got[k] for k in want} == want
    with pytest.raises(RuntimeError, match="live points"):
        d.batch_seeds(float(logl[-1]), 8, 2, 1, want_rows=False)


def test_two_chunks_plus_three_and_a_plateau(ctx):
    d, cols = merged(ctx, [2400, 2300], 100, 12)  # 4900 points
    M = len(cols["logl"])
    got, _ = compare(d, cols, float(cols["logl"][M - 4099 - 1]), 64, 65, seed=9, label="2 x 2048 + 3 points")
    assert got["count"] == 4099
    # a boundary on a plateau of equal ln L: vol_idx is the plateau's first point
    b = merge_cases.cases()["b_plateau"]
    d = ctx.merge_runs(prob3(), **b)
    cols = {k: d.field(k) for k in COLS}
    x = float(b["dead_logl"][1][50])
    first, n = int(np.nonzero(cols["logl"] == x)[0][0]), int((cols["logl"] == x).sum())
    assert n >= 7
    got, _ = compare(d, cols, x, 24, 9, seed=10, label="plateau")
    assert got["vol_idx"] == first + 1 and got["lo"] == first + n


def test_cutoff_inside_the_subset_and_a_sort_beyond_lds(ctx):
    # 2 runs x 2 live points x 1700 iterations: logvol spans more than 708 (tests/test_seed_choice_cpu.py), k = n_pos
    d, cols = merged(ctx, [1700, 1700], 2, 6)
    sub = cols["logvol"][11:]
    n_pos = int((sub - sub.max() >= -708.0).sum())
    assert 0 < n_pos < len(sub)
    got, _ = compare(d, cols, float(cols["logl"][10]), n_pos, 3, seed=13, label="k = n_pos < count")
    assert got["n_pos"] == n_pos and all(sorted(r) == list(range(11, 11 + n_pos)) for r in got["idx"])
    with pytest.raises(ValueError, match="positive weight"):
        d.batch_seeds(float(cols["logl"][10]), n_pos + 1, 3, 13, want_rows=False)
    # k = 5000 of about 20 000 points: the final sort works through global memory tiles
    d, cols = merged(ctx, [4900, 5100, 5000, 4800], 50, 14)
    compare(d, cols, float(cols["logl"][99]), 5000, 2, seed=15, label="k = 5000")


def test_reproducible_and_a_function_of_the_global_strand(small):
    d, cols = small
    lmin = float(cols["logl"][120])
    a = d.batch_seeds(lmin, 24, 5, 77, want_rows=False, want_keys=True)
    b = d.batch_seeds(lmin, 24, 5, 77, want_rows=False, want_keys=True)
    np.testing.assert_array_equal(a["idx"], b["idx"])
    np.testing.assert_array_equal(a["keys"], b["keys"])
    c = d.batch_seeds(lmin, 24, 2, 77, first=3, want_rows=False, want_keys=True)
    np.testing.assert_array_equal(c["idx"], a["idx"][3:5])
    np.testing.assert_array_equal(c["keys"], a["keys"][3:5])


def test_the_law_on_the_device(small):
    """The last seven points of the run, k = 3, 8192 strands in one call, seed 1: the 210 ordered outcomes against
    successive sampling on the downloaded logvol, the CPU test's bound."""
    d, cols = small
    M = len(cols["logl"])
    got = d.batch_seeds(float(cols["logl"][M - 8]), 3, 8192, 1, want_rows=False)
    assert got["lo"] == M - 7 and got["count"] == got["n_pos"] == 7
    chi2, emin, nout = chi2_of(got["idx"] - got["lo"], cols["logvol"][M - 7:], 3)
    bound = chi2_quantile(209, 1.0 - 1e-4)
    print(f"[batch seed law] device: chi2 = {chi2:.1f} (bound {bound:.1f}), smallest expected count {emin:.2f}")
    assert nout == 210 and chi2 < bound


@pytest.fixture(scope="module")
def real_base(ctx):
    """A finished 3-D run on the device: 4 static runs of 64 live points, merged where they ran."""
    from dynesty_amd import backend
    from dynesty_amd.ensemble import run_ensemble_merged
    prob = prob3()
    backend.set_backend(ctx)
    try:
        m = run_ensemble_merged(prob, 4, 64, 16, entropy=(21, 3), merge='device', dlogz=0.1, max_iter=20000)
    finally:
        backend.set_backend(None)
    m.pop("runs")
    return prob, m, m.weight_function()


def test_the_rows_that_come_back_are_the_chosen_points(ctx, real_base):
    """seed_u / seed_logl, gathered on the device, are samples_u and logl at idx bit for bit, so Context.ns_batch on them
    is ns_batch on the rows a gather would have brought (tests/test_gpu_ns_batch.py holds that call to its mirror); one
    batch runs from them."""
    prob, m, bounds = real_base
    logl = m.field("logl")
    lmin = bounds[0] if bounds[0] > logl[0] else float(logl[len(logl) // 4])  # (a boundary inside the run either way)
    s = m.batch_seeds(lmin, 32, 4, 5)
    assert not s["prior"] and s["idx"].shape == (4, 32) and s["seed_u"].shape == (4, 32, 3)
    np.testing.assert_array_equal(s["seed_u"], m.gather(s["idx"].ravel(), "samples_u").reshape(4, 32, 3))
    np.testing.assert_array_equal(s["seed_logl"], logl[s["idx"]])
    assert (s["seed_logl"] > s["logl_min"]).all()
    plain = m.batch_seeds(lmin, 32, 4, 5, want_rows=False)
    np.testing.assert_array_equal(plain["idx"], s["idx"])
    assert "seed_u" not in plain
    for sample, kw in (("rwalk", dict(walks=10)), ("unif", {})):
        out = ctx.ns_batch(prob, s["seed_u"], s["seed_logl"], s["logl_min"], np.array(list(s["start"]) + [1.0]), 8,
                           logl_max=bounds[1], entropy=(21, 3, 1), max_iter=4000, dlogz=0.1, sample=sample, **kw)
        assert (out["status"] == 0).all() and (out["niter"] > 0).all()
        assert all((out["dead_logl"][r, :n] > s["logl_min"]).all() for r, n in enumerate(out["niter"]))


def test_refusals_leave_the_context_usable():
    from dynesty_amd import _lib
    c = _lib.Context(0)
    prob = prob3()
    d = c.merge_runs(prob, **merge_cases.make(np.random.default_rng(11), [100, 90], 20, 3))
    logl = d.field("logl")
    lmin = float(logl[100])
    s = d.batch_seeds(lmin, 16, 2, 1)
    for bad in (dict(strands=0), dict(nlive_new=65536), dict(strands=65537), dict(nlive_new=0), dict(logl_min=np.nan),
                dict(first=-1)):
        args = dict(logl_min=lmin, nlive_new=16, strands=2, seed=1)
        args.update(bad)
        with pytest.raises(ValueError):
            d.batch_seeds(**args)
    with pytest.raises(RuntimeError):
        d.batch_seeds(float(logl[-1]), 16, 2, 1)
    P = _lib._ptr
    assert c.lib.dh_merged_batch_seed(c.handle, 1, 0, 2, 16, lmin, None, None, None, None, None) == _lib.ERR_ARG
    info = np.zeros(12)
    idx = np.empty((2, 16), dtype=np.int64)
    assert c.lib.dh_merged_batch_seed(c.handle, 1, 0, 2, 16, lmin, P(idx), None, None, None, P(info)) == 0
    np.testing.assert_array_equal(idx, s["idx"])  # (the context goes on answering, and the merged run is as it was)
    np.testing.assert_array_equal(d.field("logl"), logl)
    # after a fold the choice is made on the new run; a released run is refused; so is a context without one
    new = merge_cases.make(np.random.default_rng(3), [30, 25], 10, 3)
    top = float(logl[-1])
    new["dead_logl"] = [x + top + 40.0 for x in new["dead_logl"]]
    new["live_logl"] = new["live_logl"] + top + 40.0
    d2 = c.merged_fold(d, prob, logl_min=lmin, logl_max=np.inf, **new)
    with pytest.raises(ValueError, match="no longer on the device"):
        d.batch_seeds(lmin, 16, 2, 1)
    got = d2.batch_seeds(lmin, 16, 2, 1)
    assert got["idx"].shape == (2, 16) and got["count"] == d2.niter - got["lo"]
    d2.release()
    with pytest.raises(ValueError):
        c.merged_batch_seed(d2, lmin, 16, 2, 1)
    assert c.lib.dh_merged_batch_seed(c.handle, 1, 0, 2, 16, lmin, P(idx), None, None, None, P(info)) == _lib.ERR_ARG


def test_run_dynamic_with_device_seeds(ctx, monkeypatch):
    """4 runs x 64 live points, 2 batches of 4 strands x 32: the loop finishes, every batch's log says seeds='device',
    ln Z lies within 5 combined logzerr of the seeds='host' run on the same entropy, and inside the batch loop no whole
    logl / logvol column comes to the host and no gather of samples_u is made (the rows come back with the choice)."""
    from dynesty_amd import _lib, backend, dynamic
    prob = prob3()
    calls = []
    field, gather = _lib.DeviceMergedRun.field, _lib.DeviceMergedRun.gather

    def field_rec(self, name, first=0, count=None):
        calls.append(("field", name, first, count, self.niter))
        return field(self, name, first, count)

    def gather_rec(self, idx, field="samples"):
        calls.append(("gather", field, len(idx)))
        return gather(self, idx, field)
    backend.set_backend(ctx)
    try:
        kw = dict(pfrac=0.8, entropy=(21, 3), queue_size=8, walks=10, stop_kwargs=dict(target_n_effective=10 ** 9))
        mh, log_h = dynamic.run_dynamic(prob, 4, 64, 4, 32, 2, merge='device', seeds='host', **kw)
        zh, eh = mh.summary["logz"], mh.summary["logzerr"]
        monkeypatch.setattr(_lib.DeviceMergedRun, "field", field_rec)
        monkeypatch.setattr(_lib.DeviceMergedRun, "gather", gather_rec)
        md, log_d = dynamic.run_dynamic(prob, 4, 64, 4, 32, 2, merge='device', seeds='device', **kw)
    finally:
        backend.set_backend(None)
    assert len(log_d) == 3 and all(e["seeds"] == "device" for e in log_d[1:]) and all(e["seeds"] == "host" for e in log_h[1:])
    assert all(e["niter"] > 4 * 32 for e in log_d[1:])
    assert not all(e["prior"] for e in log_d[1:])  # (a batch inside the run: the device chose its seeds)
    zd, ed = md.summary["logz"], md.summary["logzerr"]
    print(f"[run_dynamic seeds] prior batches {[e['prior'] for e in log_d[1:]]}; ln Z host seeds {zh:.4f} +- {eh:.4f}, device seeds {zd:.4f} +- {ed:.4f}; calls {calls}")
    assert abs(zd - zh) <= 5.0 * np.hypot(eh, ed)
    for c in calls:
        if c[0] == "field":
            assert not (c[1] in ("logl", "logvol") and (c[3] is None or c[3] >= c[4])), c
        else:
            assert c[1] != "samples_u", c
