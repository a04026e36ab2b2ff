#!/usr/bin/env python
"""Generate tests/golden/*.npz by running the REAL reference (dynesty 3.0.0
from /root/reference/py, numpy/scipy of this image) on the seeded inputs of
tests/inputs.py.  Run in the build container only:

    python tools/make_golden.py

The reference cannot travel to the GPU box, the fixtures can.  Nothing here is
imported by the product.  Import shim per SURVEY.md appendix B.
"""
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def import_reference():
    shim = tempfile.mkdtemp(prefix="dynesty_shim_")
    di = os.path.join(shim, "dynesty-3.0.0.dist-info")
    os.makedirs(di)
    with open(os.path.join(di, "METADATA"), "w") as f:
        f.write("Metadata-Version: 2.1\nName: dynesty\nVersion: 3.0.0\n")
    sys.path.insert(0, shim)
    sys.path.insert(0, "/root/reference/py")
    import dynesty  # noqa
    return dynesty


def ell_fields(e):
    return dict(ctr=e.ctr, cov=e.cov, am=e.am, axes=e.axes, axlens=e.axlens,
                logvol=np.float64(e.logvol))


def gen_bounding(out):
    from dynesty import bounding as db
    import inputs
    g = {}
    for name in inputs.CLOUDS_SMALL:
        pts = inputs.cloud(name)
        n, d = pts.shape
        e = db.bounding_ellipsoid(pts)
        for k, v in ell_fields(e).items():
            g[f"{name}/be/{k}"] = v
        m = db.MultiEllipsoid(d)
        m.update(pts, rstate=np.random.default_rng(5))
        g[f"{name}/mu/nells"] = np.int64(m.nells)
        g[f"{name}/mu/ctrs"] = m.ctrs
        g[f"{name}/mu/covs"] = m.covs
        g[f"{name}/mu/ams"] = m.ams
        g[f"{name}/mu/logvol_ells"] = m.logvol_ells
        g[f"{name}/mu/logvol"] = np.float64(m.logvol)
        g[f"{name}/mu/axes"] = np.array([el.axes for el in m.ells])
        g[f"{name}/mu/axlens"] = np.array([el.axlens for el in m.ells])
        # which ellipsoid(s) each input point falls in: exact integer KAT
        # (reference: tests/test_ellipsoid.py:106-133 test_overlap)
        probe_rng = np.random.default_rng(11)
        probes = pts[probe_rng.integers(n, size=64)] + \
            0.3 * pts.std(axis=0) * probe_rng.standard_normal((64, d))
        wl = [m.within(p) for p in probes]
        g[f"{name}/kat/probes"] = probes
        g[f"{name}/kat/within_flat"] = np.concatenate(wl).astype(np.int64) \
            if len(wl) else np.zeros(0, np.int64)
        g[f"{name}/kat/within_count"] = np.array([len(w) for w in wl],
                                                 dtype=np.int64)
        g[f"{name}/kat/contains"] = np.array([m.contains(p) for p in probes])
        g[f"{name}/kat/overlap_skip0"] = np.array(
            [m.overlap(p, j=0) for p in probes], dtype=np.int64)
        # union samples, same seed (reference: bounding.py:592-606)
        g[f"{name}/mu/samples"] = m.samples(40, rstate=np.random.default_rng(7))
        # enlargement as applied by Sampler.update_bound (sampler.py:506-508)
        m.scale_to_logvol(m.logvol + np.log(1.25))
        g[f"{name}/sc/ctrs"] = m.ctrs
        g[f"{name}/sc/covs"] = m.covs
        g[f"{name}/sc/ams"] = m.ams
        g[f"{name}/sc/logvol_ells"] = m.logvol_ells
        g[f"{name}/sc/logvol"] = np.float64(m.logvol)
        g[f"{name}/sc/axes"] = np.array([el.axes for el in m.ells])
        g[f"{name}/sc/axlens"] = np.array([el.axlens for el in m.ells])
        # single-ellipsoid bound
        s = db.Ellipsoid(d)
        s.update(pts, rstate=np.random.default_rng(5))
        g[f"{name}/single/samples"] = s.samples(
            40, rstate=np.random.default_rng(8))
        g[f"{name}/single/contains"] = np.array(
            [s.contains(p) for p in probes])
        # anisotropic branch of scale_to_logvol (bounding.py:257-275):
        # ask for a volume that forces axes against the sqrt(D)/2 cap
        big = db.bounding_ellipsoid(pts)
        target = big.logvol + d * np.log(
            (np.sqrt(d) / 2) / big.axlens.max()) + 0.3 * d
        maxlv = d * np.log(np.sqrt(d) / 2) + db.logvol_prefactor(d)
        target = min(target, maxlv - 1e-3)
        big.scale_to_logvol(target)
        for k, v in ell_fields(big).items():
            g[f"{name}/aniso/{k}"] = v
        g[f"{name}/aniso/target"] = np.float64(target)
        # bootstrap expansion factors (bounding.py:1619-1648)
        seeds = np.random.SeedSequence(77).spawn(3)
        g[f"{name}/boot/single"] = np.array([
            db._ellipsoid_bootstrap_expand((False, pts, sd)) for sd in seeds])
        seeds = np.random.SeedSequence(77).spawn(3)
        g[f"{name}/boot/multi"] = np.array([
            db._ellipsoid_bootstrap_expand((True, pts, sd)) for sd in seeds])
    # improve_covar_mat on the reference's own edge cases
    # (tests/test_ellipsoid.py:242-255 test_bounds)
    for tag, mat in [("zero", np.zeros((4, 4))),
                     ("rank1", np.outer(np.arange(1., 5.), np.arange(1., 5.))),
                     ("neg", -np.eye(3))]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            good, cov, am, axes = db.improve_covar_mat(mat)
        g[f"icm/{tag}/in"] = mat
        g[f"icm/{tag}/good"] = np.bool_(good)
        g[f"icm/{tag}/cov"] = cov
        g[f"icm/{tag}/am"] = am
        g[f"icm/{tag}/axes"] = axes
    for nd in (1, 2, 3, 25, 200):
        g[f"prefactor/{nd}"] = np.float64(db.logvol_prefactor(nd))
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


def gen_proposals(out):
    from dynesty import internal_samplers as dis
    from dynesty import bounding as db
    from dynesty.utils import get_nonbounded
    import inputs
    g = {}

    def run(tag, cls, kwargs, case, nwalk, seedbase, scale=None, extra=None):
        prob = case["problem"]
        seeds = np.random.SeedSequence(seedbase).spawn(nwalk)
        smp = cls(**kwargs)
        kw = dict(smp.sampler_kwargs)
        if extra:
            kw.update(extra)
        res = []
        for i in range(nwalk):
            arg = dis.SamplerArgument(
                u=case["u0"][i].copy(), loglstar=case["loglstar"],
                axes=case["axes"], scale=scale or case["scale"],
                prior_transform=prob.prior_transform,
                loglikelihood=prob.loglikelihood, rseed=seeds[i], kwargs=kw)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res.append(cls.sample(arg))
        g[f"{tag}/u"] = np.array([r.u for r in res])
        g[f"{tag}/v"] = np.array([r.v for r in res])
        g[f"{tag}/logl"] = np.array([float(r.logl) for r in res])
        g[f"{tag}/ncalls"] = np.array([r.ncalls for r in res], dtype=np.int64)
        ti = [r.tuning_info for r in res]
        if ti[0] is not None:
            for key in ti[0]:
                g[f"{tag}/ti_{key}"] = np.array([t[key] for t in ti])
        g[f"{tag}/seedbase"] = np.int64(seedbase)
        g[f"{tag}/nwalk"] = np.int64(nwalk)

    # ---- rwalk (internal_samplers.py:866-986) ----
    for pname, nw, walks in (("C2", 8, 45), ("G5", 16, 25), ("C1", 8, 23),
                             ("C3", 8, 22), ("N6", 8, 26)):
        case = inputs.walker_case(pname, 64, 900 + walks)
        d = case["problem"].ndim
        run(f"rwalk/{pname}", dis.RWalkSampler,
            dict(ndim=d, ncdim=d, walks=walks, nonbounded=None, periodic=None,
                 reflective=None), case, nw, 4000 + walks)
    # periodic + reflective dims
    case = inputs.walker_case("G5", 64, 931, shrink=3.0)
    per, ref = np.array([0, 3]), np.array([1])
    run("rwalk/G5_pr", dis.RWalkSampler,
        dict(ndim=5, ncdim=5, walks=30,
             nonbounded=get_nonbounded(5, per, ref), periodic=per,
             reflective=ref), case, 16, 4100, scale=2.5)
    # ncdim < ndim: last two dims are redrawn U(0,1) at every step
    case = inputs.walker_case("G5", 64, 932, shrink=2.0)
    case3 = dict(case)
    case3["axes"] = case["axes"][:3, :3].copy()
    run("rwalk/G5_nc3", dis.RWalkSampler,
        dict(ndim=5, ncdim=3, walks=20, nonbounded=None, periodic=None,
             reflective=None), case3, 16, 4200)

    # ---- rslice / slice (internal_samplers.py:745-855, 593-709, 1075-1206) --
    for pname, nw, slices in (("C3", 12, 5), ("G5", 12, 4), ("N6", 8, 3),
                              ("C2", 4, 3)):
        case = inputs.walker_case(pname, 64, 950 + slices)
        d = case["problem"].ndim
        run(f"rslice/{pname}", dis.RSliceSampler,
            dict(ndim=d, ncdim=d, slices=slices, nonbounded=None,
                 periodic=None, reflective=None), case, nw, 5000 + slices)
    case = inputs.walker_case("G5", 64, 961)
    run("rslice/G5_dbl", dis.RSliceSampler,
        dict(ndim=5, ncdim=5, slices=4, nonbounded=None, periodic=None,
             reflective=None), case, 12, 5100,
        extra=dict(slice_doubling=True))
    # tiny scale forces many expansions
    run("rslice/G5_tiny", dis.RSliceSampler,
        dict(ndim=5, ncdim=5, slices=2, nonbounded=None, periodic=None,
             reflective=None), case, 8, 5200, scale=0.02)
    for pname, nw, slices in (("G5", 8, 2), ("E3", 8, 2)):
        case = inputs.walker_case(pname, 64, 970 + slices)
        d = case["problem"].ndim
        run(f"slice/{pname}", dis.SliceSampler,
            dict(ndim=d, ncdim=d, slices=slices, nonbounded=None,
                 periodic=None, reflective=None), case, nw, 6000 + slices)
    case = inputs.walker_case("G5", 64, 981)
    run("slice/G5_dbl", dis.SliceSampler,
        dict(ndim=5, ncdim=5, slices=2, nonbounded=None, periodic=None,
             reflective=None), case, 8, 6100, extra=dict(slice_doubling=True))

    # ---- unif inside a bound (internal_samplers.py:243-340) ----
    def run_unif(tag, prob, bound, nwalk, seedbase, loglstar, ndim, ncdim):
        seeds = np.random.SeedSequence(seedbase).spawn(nwalk)
        kw = dict(bound=bound, ndim=ndim, n_cluster=ncdim, nonbounded=None)
        res = []
        for i in range(nwalk):
            arg = dis.SamplerArgument(
                u=np.zeros(ndim), loglstar=loglstar, axes=None, scale=1.,
                prior_transform=prob.prior_transform,
                loglikelihood=prob.loglikelihood, rseed=seeds[i], kwargs=kw)
            res.append(dis.UniformBoundSampler.sample(arg))
        g[f"{tag}/u"] = np.array([r.u for r in res])
        g[f"{tag}/v"] = np.array([r.v for r in res])
        g[f"{tag}/logl"] = np.array([float(r.logl) for r in res])
        g[f"{tag}/ncalls"] = np.array([r.ncalls for r in res], dtype=np.int64)
        g[f"{tag}/loglstar"] = np.float64(loglstar)
        g[f"{tag}/seedbase"] = np.int64(seedbase)

    prob = inputs.problem("C1")
    pts = inputs.cloud("g3")
    single = db.Ellipsoid(3)
    single.update(pts, rstate=np.random.default_rng(5))
    lstar = float(np.quantile(
        prob.loglikelihood_many(prob.prior_transform_many(pts)), 0.3))
    run_unif("unif/C1_single", prob, single, 16, 7000, lstar, 3, 3)
    prob = inputs.problem("G5")
    pts = inputs.cloud("two5")
    multi = db.MultiEllipsoid(5)
    multi.update(pts, rstate=np.random.default_rng(5))
    multi.scale_to_logvol(multi.logvol + 5 * np.log(3.0))  # make them overlap
    lstar = float(np.quantile(
        prob.loglikelihood_many(prob.prior_transform_many(pts)), 0.3))
    run_unif("unif/G5_multi", prob, multi, 16, 7100, lstar, 5, 5)
    g["unif/G5_multi/nells"] = np.int64(multi.nells)
    # ncdim < ndim with a 3-D bound on a 5-D problem
    b3 = db.Ellipsoid(3)
    b3.update(pts[:, :3].copy(), rstate=np.random.default_rng(5))
    run_unif("unif/G5_nc3", prob, b3, 8, 7200, lstar - 30.0, 5, 3)

    # ---- unit cube (internal_samplers.py:364-441) ----
    prob = inputs.problem("C1")
    seeds = np.random.SeedSequence(7300).spawn(8)
    res = []
    for i in range(8):
        arg = dis.SamplerArgument(
            u=np.zeros(3), loglstar=-60.0, axes=None, scale=1.,
            prior_transform=prob.prior_transform,
            loglikelihood=prob.loglikelihood, rseed=seeds[i],
            kwargs=dict(ndim=3))
        res.append(dis.UnitCubeSampler.sample(arg))
    g["unitcube/C1/u"] = np.array([r.u for r in res])
    g["unitcube/C1/logl"] = np.array([float(r.logl) for r in res])
    g["unitcube/C1/ncalls"] = np.array([r.ncalls for r in res], dtype=np.int64)

    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


def gen_rng(out):
    """PCG64 / SeedSequence / ziggurat known answers from NumPy itself (the
    reference's RNG: utils.py:993-1009)."""
    g = {}
    ss = np.random.SeedSequence([11, 22, 33, 44])
    kids = ss.spawn(5)
    g["ss/entropy"] = np.array([11, 22, 33, 44], dtype=np.uint64)
    g["ss/child_state4"] = np.array(
        [k.generate_state(4, np.uint64) for k in kids])
    st = []
    for k in kids:
        s = np.random.PCG64(k).state["state"]
        st.append([s["state"] >> 64, s["state"] & (2**64 - 1),
                   s["inc"] >> 64, s["inc"] & (2**64 - 1)])
    g["ss/pcg_state"] = np.array(st, dtype=np.uint64)
    rng = np.random.Generator(np.random.PCG64(kids[2]))
    g["stream/normals"] = rng.standard_normal(5000)
    g["stream/uniforms"] = rng.random(100)
    g["stream/normals2"] = rng.standard_normal(7)
    s = rng.bit_generator.state["state"]
    g["stream/final_state"] = np.array(
        [s["state"] >> 64, s["state"] & (2**64 - 1), s["inc"] >> 64,
         s["inc"] & (2**64 - 1)], dtype=np.uint64)
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


def gen_friends(out):
    """RadFriends ('balls') / SupFriends ('cubes'): two successive updates (the
    second clusters in the metric of the first), a bootstrap update, membership
    index lists, scale_to_logvol and same-seed draws."""
    from dynesty import bounding as db
    from dynesty.utils import get_seed_sequence
    import inputs
    g = {}
    for kind, cls in (("balls", db.RadFriends), ("cubes", db.SupFriends)):
        for name in inputs.CLOUDS_FRIENDS:
            if kind == "cubes" and name == "c2s":
                # 25-D: the max-norm radius is far below the 2-norm linkage length, the second
                # update finds 600 singleton clusters and the reference divides by hsmax = 0
                continue
            pts = inputs.cloud(name)
            n, d = pts.shape
            b = cls(d)
            key = f"{kind}/{name}"
            for step in (1, 2):
                b.update(pts, rstate=np.random.default_rng(7), bootstrap=0)
                for k in ("cov", "am", "axes", "axes_inv"):
                    g[f"{key}/u{step}/{k}"] = np.array(getattr(b, k)).real
                g[f"{key}/u{step}/logvol"] = np.float64(b.logvol)
            b.ctrs = pts  # what Sampler.propose_live does (sampler.py:483-484); SupFriends.update leaves it unset
            # membership of probe points: exact integer KAT
            rng = np.random.default_rng(11)
            probes = np.concatenate([pts[rng.integers(n, size=6)] + 0.3 * rng.standard_normal((6, d)) @ b.axes,
                                     rng.uniform(size=(4, d))])
            g[f"{key}/probes"] = probes
            w = [b.within(x) for x in probes]
            g[f"{key}/within_counts"] = np.array([len(x) for x in w], dtype=np.int64)
            g[f"{key}/within_idx"] = np.concatenate(w).astype(np.int64) if sum(map(len, w)) else np.zeros(0, np.int64)
            # draws from ONE generator
            rs = np.random.default_rng(13)
            g[f"{key}/samples"] = b.samples(12, rstate=rs)
            g[f"{key}/samples_state_after"] = np.array(
                [rs.bit_generator.state["state"]["state"] >> 64, rs.bit_generator.state["state"]["state"] & (2**64 - 1),
                 rs.bit_generator.state["has_uint32"], rs.bit_generator.state["uinteger"]], dtype=np.uint64)
            rs = np.random.default_rng(14)
            xq = [b.sample(rstate=rs, return_q=True) for _ in range(8)]
            g[f"{key}/sample_q_x"] = np.array([x for x, q in xq])
            g[f"{key}/sample_q_q"] = np.array([q for x, q in xq], dtype=np.int64)
            # enlarge
            lv = b.logvol + np.log(1.25)
            b.scale_to_logvol(lv)
            for k in ("cov", "am", "axes", "axes_inv"):
                g[f"{key}/scaled/{k}"] = np.array(getattr(b, k)).real
            # bootstrap radius (3 replicas) from a fresh bound of the same kind
            b2 = cls(d)
            b2.update(pts, rstate=np.random.default_rng(7), bootstrap=0)
            b2.update(pts, rstate=np.random.default_rng(9), bootstrap=3)
            for k in ("cov", "am", "axes", "axes_inv"):
                g[f"{key}/boot/{k}"] = np.array(getattr(b2, k)).real
            g[f"{key}/boot/logvol"] = np.float64(b2.logvol)
            # no-clustering variant
            b3 = cls(d)
            b3.update(pts, rstate=np.random.default_rng(7), bootstrap=0, use_clustering=False)
            g[f"{key}/noclust/cov"] = np.array(b3.cov).real
            g[f"{key}/noclust/logvol"] = np.float64(b3.logvol)
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


def gen_runs(out):
    """Short end-to-end reference runs (static NestedSampler) for the logZ
    gate.  C1 full run; C2/C3 are too slow to regenerate casually, their
    same-seed values are recorded in SURVEY.md section 8c."""
    import dynesty
    import inputs
    g = {}
    prob = inputs.problem("C1")
    s = dynesty.NestedSampler(prob.loglikelihood, prob.prior_transform, 3,
                              nlive=500, bound='single', sample='unif',
                              rstate=np.random.default_rng(21))
    s.run_nested(dlogz=0.01, print_progress=False, add_live=False)
    r = s.results
    g["C1/logz"] = np.float64(r.logz[-1])
    g["C1/logzerr"] = np.float64(r.logzerr[-1])
    g["C1/niter"] = np.int64(r.niter)
    g["C1/ncall"] = np.int64(np.sum(r.ncall))
    np.savez_compressed(out, **g)
    print("wrote", out, dict((k, float(v)) for k, v in g.items()))


def gen_wide(out):
    """Wide-D shapes (D > 44) from the real reference: MultiEllipsoid on two / three clusters in
    48 / 64-D, Ellipsoid on the 4000 x 200 cloud (compact: centre, axis lengths, logvol, two rows of
    the covariance), RSliceSampler in 64-D and RWalkSampler in 50-D on child streams."""
    from dynesty import bounding as db
    from dynesty import internal_samplers as dis
    import inputs
    g = {}
    for d, sizes in ((48, (2000, 2000)), (64, (2000, 1800, 2200))):
        pts = inputs.blobs(d, sizes, 0.3, d)
        m = db.bounding_ellipsoids(pts)
        g[f"multi{d}/nells"] = np.int64(m.nells)
        g[f"multi{d}/ctrs"] = np.array(m.ctrs)
        g[f"multi{d}/logvol_ells"] = np.array(m.logvol_ells)
        g[f"multi{d}/covs"] = np.array(m.covs)
    pts = inputs.cloud("g200")
    e = db.bounding_ellipsoid(pts)
    g["single200/ctr"] = e.ctr
    g["single200/logvol"] = np.float64(e.logvol)
    g["single200/axlens_sorted"] = np.sort(e.axlens)
    g["single200/cov_rows"] = e.cov[[0, 17]]
    g["single200/cov_trace"] = np.float64(np.trace(e.cov))
    for tag, cls, d, kw, seedbase in (("rslice64", dis.RSliceSampler, 64, dict(slices=3), 6400),
                                       ("rwalk50", dis.RWalkSampler, 50, dict(walks=30), 5000)):
        case = inputs.wide_walker_case(d, 6, d)
        prob = case["problem"]
        smp = cls(ndim=d, ncdim=d, nonbounded=None, periodic=None, reflective=None, **kw)
        seeds = np.random.SeedSequence(seedbase).spawn(6)
        res = []
        for i in range(6):
            arg = dis.SamplerArgument(u=case["u0"][i].copy(), loglstar=case["loglstar"], axes=case["axes"],
                                      scale=0.8, prior_transform=prob.prior_transform,
                                      loglikelihood=prob.loglikelihood, rseed=seeds[i],
                                      kwargs=dict(smp.sampler_kwargs))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res.append(cls.sample(arg))
        g[f"{tag}/u"] = np.array([r.u for r in res])
        g[f"{tag}/logl"] = np.array([float(r.logl) for r in res])
        g[f"{tag}/ncalls"] = np.array([r.ncalls for r in res], dtype=np.int64)
        for key in res[0].tuning_info:
            g[f"{tag}/ti_{key}"] = np.array([r.tuning_info[key] for r in res])
        g[f"{tag}/seedbase"] = np.int64(seedbase)
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


class _Enough(Exception):
    pass


def gen_livesets(out):
    """Live sets captured from REAL reference runs ("live sets captured from
    the oracle at fixed iterations, so shapes and distributions are real"), together with what the
    reference's own MultiEllipsoid.update made of them.  C2 (25-D, nlive 2000, multi/rwalk): bound
    updates number 1, 8 and 24 of the seed-21 run; C3 (eggbox, nlive 5000, multi/rslice): updates
    1, 6 and 16.  Uniform-in-contour shells, not Gaussian clouds: different fmax / k-means behaviour."""
    import dynesty
    from dynesty import bounding as db
    import inputs
    g = {}
    for tag, pname, nlive, sample, picks in (("C2", "C2", 2000, "rwalk", (1, 8, 24)),
                                             ("C3", "C3", 5000, "rslice", (1, 6, 16))):
        prob = inputs.problem(pname)
        taken = []
        orig = db.MultiEllipsoid.update

        def spy(self, points, *a, **kw):
            spy.n += 1
            pts = np.array(points)
            r = orig(self, points, *a, **kw)
            if spy.n in picks:
                taken.append((spy.n, pts, np.array(self.ctrs), np.array(self.covs),
                              np.array(self.logvol_ells), float(self.logvol)))
            if spy.n >= max(picks):
                raise _Enough
            return r
        spy.n = 0
        db.MultiEllipsoid.update = spy
        try:
            s = dynesty.NestedSampler(prob.loglikelihood, prob.prior_transform, prob.ndim,
                                      nlive=nlive, bound='multi', sample=sample,
                                      rstate=np.random.default_rng(21))
            try:
                s.run_nested(dlogz=0.01, print_progress=False)
            except _Enough:
                pass
        finally:
            db.MultiEllipsoid.update = orig
        for i, (n, pts, ctrs, covs, lve, lv) in enumerate(taken):
            g[f"{tag}/{i}/update_no"] = np.int64(n)
            g[f"{tag}/{i}/live_u"] = pts
            g[f"{tag}/{i}/nells"] = np.int64(len(ctrs))
            g[f"{tag}/{i}/ctrs"] = ctrs
            g[f"{tag}/{i}/covs"] = covs
            g[f"{tag}/{i}/logvol_ells"] = lve
            g[f"{tag}/{i}/logvol"] = np.float64(lv)
            print(tag, i, "update", n, "nells", len(ctrs), "logvol", lv, flush=True)
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


def gen_nsloop(out):
    """The run loop's bookkeeping from a REAL NestedSampler run (G5, nlive 200, multi/rwalk, queue of
    64 through a serial pool): for three queue fills the live log-likelihoods at the moment of the
    fill, the queue's (logl, ncalls) in order, and the dead points / evidence history the run
    recorded until the next fill; plus the whole run's dead and final live log-likelihoods with its
    final ln Z, error and information.  Pins oracle/nested_ref.py (sampler.py:741-776, 1070-1185,
    780-930; utils.py:1470-1492)."""
    import dynesty
    from dynesty import sampler as dsamp
    import inputs
    prob = inputs.problem("G5")
    nlive, K = 200, 64

    class SerialPool:
        size = K

        def map(self, f, x):
            return list(map(f, x))
    fills = []
    orig = dsamp.Sampler._fill_queue

    def spy(self, loglstar):
        snap = dict(it=len(self.saved_run['logl']), live_logl=np.array(self.live_logl),
                    loglstar_arg=float(loglstar), plateau_mode=bool(self.plateau_mode),
                    plateau_counter=int(getattr(self, "plateau_counter", 0) or 0),
                    plateau_logdvol=float(getattr(self, "plateau_logdvol", 0.) or 0.),
                    ncall=int(self.ncall))
        orig(self, loglstar)
        snap["q_logl"] = np.array([float(r.logl) for r in self.queue])
        snap["q_ncalls"] = np.array([int(r.ncalls) for r in self.queue], dtype=np.int64)
        fills.append(snap)
    dsamp.Sampler._fill_queue = spy
    # run_nested replaces the evidence history by compute_integrals' at the very end
    # (sampler.py:1342-1348): keep what the recurrence (progress_integration) had recorded
    rec = {}
    orig_ci = dsamp.compute_integrals

    def spy_ci(**kw):
        for key in ("logz", "logzvar", "h"):
            rec[key] = np.array(s.saved_run[key], dtype=np.float64)
        return orig_ci(**kw)
    dsamp.compute_integrals = spy_ci
    try:
        s = dynesty.NestedSampler(prob.loglikelihood, prob.prior_transform, prob.ndim, nlive=nlive,
                                  bound='multi', sample='rwalk', walks=20, pool=SerialPool(),
                                  queue_size=K, rstate=np.random.default_rng(77))
        s.run_nested(dlogz=0.05, print_progress=False)
    finally:
        dsamp.Sampler._fill_queue = orig
        dsamp.compute_integrals = orig_ci
    sr = dict(s.saved_run.items()) if hasattr(s.saved_run, "items") else s.saved_run
    final = {key: np.array(s.saved_run[key], dtype=np.float64) for key in ("logz", "logzvar", "h")}
    sr = {key: s.saved_run[key] for key in ("logl", "id", "logvol")}
    sr.update(rec)  # the per-iteration history below is the recurrence's
    niter = len(sr['logl']) - nlive  # add_live appended the final live points
    g = {"nlive": np.int64(nlive), "K": np.int64(K), "dlogz": np.float64(0.05),
         "nfills": np.int64(len(fills)), "niter": np.int64(niter),
         "run/logl": np.array(sr['logl'], dtype=np.float64),
         "run/logvol": np.array(sr['logvol'], dtype=np.float64),
         # the per-point bookkeeping of saved_run (sampler.py:1165-1182, 870-890)
         "run/id": np.array(s.saved_run['id'], dtype=np.int64),
         "run/it": np.array(s.saved_run['it'], dtype=np.int64),
         "run/nc": np.array(s.saved_run['nc'], dtype=np.int64),
         # every fill of the run, so that the whole loop can be replayed
         "fills/live_logl0": fills[0]["live_logl"],
         "fills/q_logl": np.array([f["q_logl"] for f in fills]),
         "fills/q_ncalls": np.array([f["q_ncalls"] for f in fills]),
         "run/ncall_init": np.int64(fills[0]["ncall"]),
         # final values of the recurrence (what the stopping rule saw) ...
         "rec/logz_final": np.float64(rec["logz"][-1]), "rec/logzvar_final": np.float64(rec["logzvar"][-1]),
         "rec/h_final": np.float64(rec["h"][-1]),
         # ... and compute_integrals' per-point history (what Results reports)
         "run/logz": final["logz"], "run/logzvar": final["logzvar"], "run/h": final["h"],
         "run/logz_final": np.float64(s.results.logz[-1]),
         "run/logzerr_final": np.float64(s.results.logzerr[-1]),
         "run/h_final": np.float64(s.results.information[-1]),
         "run/ncall": np.int64(s.ncall)}
    picks = (2, len(fills) // 2, len(fills) - 1)
    for tag, f in zip("abc", picks):
        a = fills[f]
        b = fills[f + 1]["it"] if f + 1 < len(fills) else niter
        i0 = a["it"]
        g[f"fill_{tag}/index"] = np.int64(f)
        g[f"fill_{tag}/it0"] = np.int64(i0)
        g[f"fill_{tag}/live_logl"] = a["live_logl"]
        g[f"fill_{tag}/q_logl"] = a["q_logl"]
        g[f"fill_{tag}/q_ncalls"] = a["q_ncalls"]
        # state after iteration i0 - 1 (the fill is asked for inside iteration i0)
        for key in ("logz", "logzvar", "h", "logvol", "logl"):
            g[f"fill_{tag}/state_{key}"] = np.float64(sr[key][i0 - 1] if i0 > 0 else
                                                      dict(logz=-1.e300, logzvar=0., h=0., logvol=0.,
                                                           logl=-1.e300)[key])
        g[f"fill_{tag}/dead_logl"] = np.array(sr['logl'][i0:b], dtype=np.float64)
        g[f"fill_{tag}/dead_slot"] = np.array(sr['id'][i0:b], dtype=np.int64)
        g[f"fill_{tag}/logz"] = np.array(sr['logz'][i0:b], dtype=np.float64)
        g[f"fill_{tag}/logzvar"] = np.array(sr['logzvar'][i0:b], dtype=np.float64)
        g[f"fill_{tag}/h"] = np.array(sr['h'][i0:b], dtype=np.float64)
        g[f"fill_{tag}/is_last"] = np.bool_(f + 1 == len(fills))
        g[f"fill_{tag}/state_plateau_mode"] = np.bool_(a["plateau_mode"])
        g[f"fill_{tag}/state_plateau_counter"] = np.int64(a["plateau_counter"])
        g[f"fill_{tag}/state_plateau_logdvol"] = np.float64(a["plateau_logdvol"])
        print("fill", tag, f, "it0", i0, "deaths", b - i0)
    lv = np.array(sr['logvol'][:niter], dtype=np.float64)
    ladder = np.abs(np.diff(lv, prepend=0.) + np.log((nlive + 1.) / nlive)) > 1e-12
    g["run/first_plateau_it"] = np.int64(np.argmax(ladder) if ladder.any() else niter)
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays; niter", niter, "fills", len(fills), "logz", g["run/logz_final"])


def gen_merge(out):
    """dynesty.utils.merge_runs on short static C1 runs (tests/test_merge_cpu.py): the per-run arrays the device
    hands to ensemble.merge_logz / merge_static_runs and the reference's merged results."""
    import dynesty
    from dynesty import utils as dyu
    import inputs
    prob = inputs.problem("C1")
    g = {}
    # 1) ln Z and its error: four runs of nlive 100
    res = []
    for s in range(4):
        sm = dynesty.NestedSampler(prob.loglikelihood, prob.prior_transform, 3, nlive=100, bound='single',
                                   sample='unif', rstate=np.random.default_rng(s))
        sm.run_nested(dlogz=0.1, print_progress=False)
        res.append(sm.results)
    merged = dyu.merge_runs(res, print_progress=False)
    nit = [r.niter for r in res]
    dead = np.zeros((4, max(nit)))
    for i, r in enumerate(res):
        dead[i, :nit[i]] = r.logl[:nit[i]]
    g["logz/dead"], g["logz/nit"] = dead, np.array(nit, dtype=np.int64)
    g["logz/live"] = np.array([np.asarray(r.logl[r.niter:]) for r in res])
    g["logz/logz"], g["logz/logzerr"] = np.float64(merged.logz[-1]), np.float64(merged.logzerr[-1])
    # 2) every per-point field: three runs of nlive 60
    R, N = 3, 60
    res = []
    for s in range(R):
        sm = dynesty.NestedSampler(prob.loglikelihood, prob.prior_transform, 3, nlive=N, bound='single',
                                   sample='unif', rstate=np.random.default_rng(100 + s))
        sm.run_nested(dlogz=0.3, print_progress=False)
        res.append(sm.results)
    ref = dyu.merge_runs(res, print_progress=False)
    nit = [r.niter for r in res]
    dead_l, dead_u = np.zeros((R, max(nit))), np.zeros((R, max(nit), 3))
    live_l, live_u = np.zeros((R, N)), np.zeros((R, N, 3))
    dead_i = np.zeros((3, R, max(nit)), dtype=np.int64)
    live_it = np.zeros((R, N), dtype=np.int64)
    for i, r in enumerate(res):
        dead_l[i, :nit[i]] = r.logl[:nit[i]]
        dead_u[i, :nit[i]] = r.samples_u[:nit[i]]
        dead_i[0, i, :nit[i]] = r.samples_id[:nit[i]]
        dead_i[1, i, :nit[i]] = r.samples_it[:nit[i]]
        dead_i[2, i, :nit[i]] = r.ncall[:nit[i]]
        # the device hands the final live points over in SLOT order (slot = the reference's 'id'), not sorted
        sl = np.argsort(r.samples_id[nit[i]:])
        assert (np.asarray(r.samples_id[nit[i]:])[sl] == np.arange(N)).all()
        live_l[i] = np.asarray(r.logl[nit[i]:])[sl]
        live_u[i] = np.asarray(r.samples_u[nit[i]:])[sl]
        live_it[i] = np.asarray(r.samples_it[nit[i]:])[sl]
    g.update({"static/nit": np.array(nit, dtype=np.int64), "static/dead_l": dead_l, "static/dead_u": dead_u,
              "static/live_l": live_l, "static/live_u": live_u, "static/dead_i": dead_i, "static/live_it": live_it})
    for k in ("samples_id", "samples_it", "ncall", "logl", "samples_n", "samples_u", "samples", "logvol", "logwt",
              "logz", "information", "logzerr"):
        g["ref/" + k] = np.asarray(getattr(ref, k))
    g["ref/niter"] = np.int64(ref.niter)
    g["ref/importance_weights"] = np.asarray(ref.importance_weights())
    g["ref/eff"] = np.float64(ref.eff)
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


def gen_merge_device(out, merge_npz):
    """Moments and equal-weight samples of the merged run merge.npz already holds (tests/test_merge_hp_cpu.py,
    tests/test_gpu_merge.py): utils.mean_and_cov and utils.resample_equal of (ref/samples, ref/importance_weights)
    for the generators default_rng(0..3), and the u0 each of them draws first."""
    from dynesty import utils as dyu
    m = np.load(merge_npz)
    samples, w = m["ref/samples"], m["ref/importance_weights"]
    g = {}
    g["mean"], g["cov"] = dyu.mean_and_cov(samples, w)
    for s in range(4):
        g[f"resample/{s}"] = dyu.resample_equal(samples, w, rstate=np.random.default_rng(s))
        g[f"u0/{s}"] = np.float64(np.random.default_rng(s).random())
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


MARGINAL_Q = [0, 0.001, 0.025, 0.16, 0.5, 0.84, 0.975, 0.999, 1]


def gen_merge_marginals(out, merge_npz):
    """Credible intervals of the merged run merge.npz already holds (tests/test_merge_marginals_cpu.py,
    tests/test_gpu_merge_marginals.py): utils.quantile(ref/samples[:, c], q, weights=ref/importance_weights) for
    c = 0..2 at MARGINAL_Q."""
    from dynesty import utils as dyu
    m = np.load(merge_npz)
    samples, w = m["ref/samples"], m["ref/importance_weights"]
    q = np.array(MARGINAL_Q, dtype=np.float64)
    g = dict(q=q, quantile=np.array([dyu.quantile(samples[:, c], q, weights=w) for c in range(3)], dtype=np.float64))
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


def gen_merge_errors(out, merge_npz):
    """Statistical errors of the merged run merge.npz already holds (tests/test_merge_errors_cpu.py,
    tests/test_gpu_merge_errors.py): a Results of its ref/* arrays; the last logz of utils.jitter_run(res,
    default_rng(i)) for i < 2000 (exact form) and of jitter_run(res, default_rng(10000 + i), approx=True), the last
    information of the first 200 of each, and utils.reweight_run(res, logp_new) for
    logp_new = logl + 0.3 default_rng(3).standard_normal(M): its logwt, logz and information arrays.

    The information: both functions compute it (compute_integrals' fourth result) and hand it to results_substitute
    under the key 'h', which a Results does not have, so their results still carry the INPUT run's information.  What is
    recorded here is the value they computed: utils.compute_integrals on the result's own logvol (and reweight)."""
    from dynesty import utils as dyu
    m = np.load(merge_npz)
    res = dyu.Results({k: m["ref/" + k] for k in ("samples_u", "samples_id", "samples_it", "logl", "samples", "samples_n",
                                                  "logvol", "logwt", "logz", "logzerr", "information", "ncall")})
    nreal, ninfo = 2000, 200
    g = {}
    for name, first, approx in (("exact", 0, False), ("approx", 10000, True)):
        lz, h = np.empty(nreal), np.empty(ninfo)
        for i in range(nreal):
            r = dyu.jitter_run(res, rstate=np.random.default_rng(first + i), approx=approx)
            lz[i] = r.logz[-1]
            if i < ninfo:
                assert np.array_equal(r.information, res.information)  # (the dropped 'h', see above)
                h[i] = dyu.compute_integrals(logl=np.asarray(res.logl), logvol=np.asarray(r.logvol))[3][-1]
        g[f"jitter/{name}/logz"], g[f"jitter/{name}/information"] = lz, h
    logl = np.asarray(res.logl)
    g["reweight/logp_new"] = logl + 0.3 * np.random.default_rng(3).standard_normal(len(logl))
    rw = dyu.reweight_run(res, g["reweight/logp_new"])
    for k in ("logwt", "logz"):
        g["reweight/" + k] = np.asarray(getattr(rw, k))
    g["reweight/information"] = dyu.compute_integrals(logl=logl, logvol=np.asarray(res.logvol),
                                                      reweight=g["reweight/logp_new"] - logl)[3]
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays")


class _RecordingGenerator:
    """A numpy Generator whose integers() draws are kept (utils.resample_run's strand draws)."""

    def __init__(self, rng):
        self._rng, self.draws = rng, []

    def integers(self, *a, **kw):
        d = self._rng.integers(*a, **kw)
        self.draws.append(np.array(d))
        return d

    def __getattr__(self, k):
        return getattr(self._rng, k)


def gen_merge_bootstrap(out, merge_npz):
    """The strand bootstrap (tests/test_merge_bootstrap_cpu.py, tests/test_gpu_merge_bootstrap.py).  For the golden
    merged run and the cases of tests/bootstrap_cases.py, as a Results whose samples_id is the strand key
    run * nlive + slot, with samples_batch = 0 and batch_logl_bounds = [(-inf, inf)] (every strand a base strand):
    utils.resample_run(res, default_rng(i), return_idx=True) for i < 4 -- the strand indices it drew, samples_n,
    samp_idx, logvol, logwt, logz and the information of utils.compute_integrals on the result's own logvol (the
    dropped 'h', see gen_merge_errors).  For the golden run the last logz of 2000 such calls with
    default_rng(20000 + i), and of 2000 calls of the documentation's simulate_run with default_rng(30000 + i): the
    reference no longer ships that function; it is jitter_run(resample_run(res, rstate), rstate, approx=True), as its
    documentation describes it."""
    from dynesty import utils as dyu
    import bootstrap_cases as bc
    gm = np.load(merge_npz)
    g = {}
    for name in bc.NAMES:
        m = bc.host_run(name, gm)
        key, S = bc.strands(m)
        M = len(key)
        assert np.array_equal(np.unique(key), np.arange(S))
        if name == "golden":
            for k in ("logvol", "logwt", "logz", "samples_n"):
                np.testing.assert_allclose(m[k], gm["ref/" + k], rtol=0, atol=1e-9)
        res = dyu.Results(dict(samples_u=m.samples_u, samples_id=key, samples_it=m.samples_it, logl=m.logl,
                               samples=m.samples, samples_n=m.samples_n, logvol=m.logvol, logwt=m.logwt, logz=m.logz,
                               logzerr=m.logzerr, information=m.information, ncall=m.ncall, blob=np.zeros(M),
                               samples_batch=np.zeros(M, dtype=int), batch_logl_bounds=np.array([(-np.inf, np.inf)])))
        for i in range(bc.NCALLS):
            rs = _RecordingGenerator(np.random.default_rng(i))
            r, idx = dyu.resample_run(res, rstate=rs, return_idx=True)
            assert len(rs.draws) == 1 and rs.draws[0].shape == (S,)
            p = f"{name}/{i}/"
            g[p + "draws"] = rs.draws[0].astype(np.int32)
            g[p + "samples_n"], g[p + "samp_idx"] = np.asarray(r.samples_n, dtype=np.int32), idx.astype(np.int32)
            g[p + "logvol"], g[p + "logwt"], g[p + "logz"] = (np.asarray(getattr(r, k)) for k in ("logvol", "logwt", "logz"))
            g[p + "information"] = np.float64(dyu.compute_integrals(logl=np.asarray(r.logl), logvol=np.asarray(r.logvol))[3][-1])
        if name == "golden":
            n = 2000
            g["golden/resample/logz"] = np.array([dyu.resample_run(res, rstate=np.random.default_rng(20000 + i)).logz[-1]
                                                  for i in range(n)])
            lz = np.empty(n)
            for i in range(n):
                rs = np.random.default_rng(30000 + i)
                lz[i] = dyu.jitter_run(dyu.resample_run(res, rstate=rs), rstate=rs, approx=True).logz[-1]
            g["golden/simulate/logz"] = lz
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays,", os.path.getsize(out), "bytes")


DYN_PFRAC, DYN_MAXFRAC = (0.0, 0.5, 0.8, 1.0), (0.8, 0.3, 0.05)
DYN_STOP = ({}, dict(pfrac=0.5, evid_thresh=0.05, target_n_effective=2000), dict(pfrac=0.0, evid_thresh=0.2))


def gen_merge_dynamic(out, merge_npz):
    """Run-level analysis of a dynamic sampler (tests/test_merge_dynamic_cpu.py, tests/test_gpu_merge_dynamic.py), on
    the Results gen_merge_bootstrap builds for the golden merged run and the cases of tests/bootstrap_cases.py.
    dynamicsampler.weight_function(res, args, return_weights=True) over pfrac in DYN_PFRAC, maxfrac in DYN_MAXFRAC and
    pad in (0, 1, 5, 2 M): the bounds, the first and last index above the threshold (from the weights it returned), and
    the three weight arrays at pfrac 0.8.  utils.kld_error(res, 'resample', rstate) with default_rng(i), i < NCALLS: the
    strand draws and the cumulative divergence.  For the golden run the last divergence of 2000 calls each of
    kld_error(res, 'jitter', default_rng(40000 + i), approx=True), of the exact form with default_rng(60000 + i) and of
    'resample' with default_rng(50000 + i), and stopping_function(res, args, return_vals=True) with n_mc = 0 for
    DYN_STOP."""
    from dynesty import dynamicsampler as dys
    from dynesty import utils as dyu
    import bootstrap_cases as bc
    gm = np.load(merge_npz)
    g = dict(pfrac=np.array(DYN_PFRAC), maxfrac=np.array(DYN_MAXFRAC))
    for name in bc.NAMES:
        m = bc.host_run(name, gm)
        key, S = bc.strands(m)
        M = len(key)
        res = dyu.Results(dict(samples_u=m.samples_u, samples_id=key, samples_it=m.samples_it, logl=m.logl,
                               samples=m.samples, samples_n=m.samples_n, logvol=m.logvol, logwt=m.logwt, logz=m.logz,
                               logzerr=m.logzerr, information=m.information, ncall=m.ncall, blob=np.zeros(M),
                               samples_batch=np.zeros(M, dtype=int), batch_logl_bounds=np.array([(-np.inf, np.inf)])))
        pads = (0, 1, 5, 2 * M)
        g[f"{name}/pad"] = np.array(pads, dtype=np.int64)
        bounds = np.empty((len(DYN_PFRAC), len(DYN_MAXFRAC), len(pads), 2))
        idx = np.empty((len(DYN_PFRAC), len(DYN_MAXFRAC), 2), dtype=np.int64)
        margin = np.inf
        for i, pf in enumerate(DYN_PFRAC):
            for j, mf in enumerate(DYN_MAXFRAC):
                for k, pad in enumerate(pads):
                    bounds[i, j, k], (pw, zw, w) = dys.weight_function(res, dict(pfrac=pf, maxfrac=mf, pad=pad), return_weights=True)
                on = np.flatnonzero(w > mf * w.max())
                idx[i, j] = on[0], on[-1]
                margin = min(margin, float(np.min(np.abs(w - mf * w.max())) / w.max()))
                if pf == 0.8:
                    g[f"{name}/pweight"], g[f"{name}/zweight"], g[f"{name}/weight"] = pw, zw, w
        g[f"{name}/bounds"], g[f"{name}/idx"] = bounds, idx
        print(name, "M", M, "smallest |weight - maxfrac max| / max", margin)
        for i in range(bc.NCALLS):
            rs = _RecordingGenerator(np.random.default_rng(i))
            kld = dyu.kld_error(res, "resample", rstate=rs)
            assert len(rs.draws) == 1 and rs.draws[0].shape == (S,)
            g[f"{name}/{i}/draws"], g[f"{name}/{i}/kld"] = rs.draws[0].astype(np.int32), np.asarray(kld)
        if name == "golden":
            n = 2000
            rng = np.random.default_rng
            g["golden/jitter_approx/kld"] = np.array([dyu.kld_error(res, "jitter", rstate=rng(40000 + i), approx=True)[-1] for i in range(n)])
            g["golden/jitter_exact/kld"] = np.array([dyu.kld_error(res, "jitter", rstate=rng(60000 + i), approx=False)[-1] for i in range(n)])
            g["golden/resample/kld"] = np.array([dyu.kld_error(res, "resample", rstate=rng(50000 + i))[-1] for i in range(n)])
            for i, args in enumerate(DYN_STOP):
                flag, vals = dys.stopping_function(res, dict(args, n_mc=0), return_vals=True)
                g[f"golden/stop/{i}"] = np.array(vals + (float(flag),))
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays,", os.path.getsize(out), "bytes")


class _ChoiceRecorder(np.random.Generator):
    """A numpy Generator (a real one: the reference tests isinstance) whose choice() results, and the bit generator's
    state before each, are kept in `calls`."""

    def choice(self, *a, **kw):
        if not hasattr(self, "calls"):
            self.calls = []
        before = _pcg_state(self)
        d = super().choice(*a, **kw)
        self.calls.append((before, np.array(d)))
        return d


def _pcg_state(rng):
    """[state hi, state lo, inc hi, inc lo, has_uint32, uinteger] of a PCG64 generator."""
    st = rng.bit_generator.state
    s, i = int(st["state"]["state"]), int(st["state"]["inc"])
    m = (1 << 64) - 1
    return np.array([s >> 64, s & m, i >> 64, i & m, int(st["has_uint32"]), int(st["uinteger"])], dtype=np.uint64)


def gen_batch(out):
    """Dynamic batches (tests/test_dynamic_cpu.py): a 3-D unit Gaussian exp(-|x|^2 / 2) under a uniform prior on
    [-10, 10]^3, DynamicNestedSampler.run_nested(nlive_init=50, nlive_batch=50, maxbatch=3), seed 20.  For every batch b:
    the saved run before it (b/base/*), the generator's state before _configure_batch_sampler's weighted choice and the
    chosen subset, the bounds it was given and the adjusted ones it returned, vol_idx (the rows it left in the batch
    sampler's saved run), the new run (b/new/*) and the saved run after combine_runs (b/after/*).  Then three calls of
    _configure_batch_sampler on the first saved run (sel/0..2): a bound with fewer than nlive_new points above it, a
    bound below every point, and logl_bounds=None."""
    import dynesty
    from dynesty import dynamicsampler as dys

    def loglike(x):
        return -0.5 * float(np.dot(x, x))

    def ptform(u):
        return 20.0 * u - 10.0
    NL = 50
    rec = _ChoiceRecorder(np.random.PCG64(20))
    rec.calls = []
    ds = dynesty.DynamicNestedSampler(loglike, ptform, 3, nlive=NL, rstate=rec, sample="rwalk", bound="multi")
    g = dict(nlive=np.array(NL))
    keys = ("logl", "logvol", "n", "id", "it", "nc", "u", "logz", "logzvar", "h", "batch")

    def saved(prefix, run, which=keys):
        for k in which:
            g[f"{prefix}/{k}"] = np.array(run[k])
    state = dict(b=0, first=None)
    conf0, comb0 = dys._configure_batch_sampler, dys.DynamicSampler.combine_runs

    def conf(main_sampler, nlive_new, update_interval, logl_bounds=None, save_bounds=None):
        b = state["b"]
        saved(f"{b}/base", main_sampler.saved_run)
        if state["first"] is None:
            state["first"] = main_sampler
        ncalls = len(rec.calls)
        res = conf0(main_sampler, nlive_new, update_interval, logl_bounds=logl_bounds, save_bounds=save_bounds)
        g[f"{b}/bounds_in"] = np.array(logl_bounds, dtype=np.float64)
        g[f"{b}/bounds_out"] = np.array([res[3], res[4]], dtype=np.float64)
        g[f"{b}/vol_idx"] = np.array(len(res[0].saved_run["logl"]))
        if len(rec.calls) > ncalls:
            g[f"{b}/rstate"], g[f"{b}/subset"] = rec.calls[ncalls]
        return res

    def comb(self):
        b = state["b"]
        saved(f"{b}/new", self.new_run, ("logl", "n", "id", "it", "nc", "u"))
        g[f"{b}/new_bounds"] = np.array([self.new_logl_min, self.new_logl_max], dtype=np.float64)
        comb0(self)
        saved(f"{b}/after", self.saved_run, keys + ("logwt",))
        g[f"{b}/after/batch_nlive"] = np.array(self.saved_run["batch_nlive"])
        g[f"{b}/after/batch_bounds"] = np.array(self.saved_run["batch_logl_bounds"], dtype=np.float64)
        state["b"] = b + 1
    dys._configure_batch_sampler, dys.DynamicSampler.combine_runs = conf, comb
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ds.run_nested(nlive_init=NL, nlive_batch=NL, maxbatch=3, print_progress=False)
        g["nbatch"] = np.array(state["b"])
        # three constructed selections on the FIRST saved run: the sampler is wound back to it
        first = {k: g[f"0/base/{k}"] for k in keys}
        for k in keys:
            ds.saved_run[k] = list(first[k])
        ll = first["logl"]
        cases = [(float(ll[-NL // 2]), float(ll[-1])),  # fewer than nlive_new points above the bound
                 (float(ll[0]) - 1.0, float(ll[-1])),   # below every point: the batch starts from the prior
                 None]
        for i, lb in enumerate(cases):
            ncalls = len(rec.calls)
            before = _pcg_state(rec)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = conf0(ds, NL, NL, logl_bounds=lb, save_bounds=False)
            g[f"sel/{i}/bounds_in"] = np.array([np.nan, np.nan] if lb is None else lb, dtype=np.float64)
            g[f"sel/{i}/bounds_out"] = np.array([res[3], res[4]], dtype=np.float64)
            g[f"sel/{i}/vol_idx"] = np.array(len(res[0].saved_run["logl"]))
            g[f"sel/{i}/rstate"] = rec.calls[ncalls][0] if len(rec.calls) > ncalls else before
            g[f"sel/{i}/subset"] = rec.calls[ncalls][1] if len(rec.calls) > ncalls else np.zeros(0, dtype=np.int64)
    finally:
        dys._configure_batch_sampler, dys.DynamicSampler.combine_runs = conf0, comb0
    np.savez_compressed(out, **g)
    print("wrote", out, len(g), "arrays,", os.path.getsize(out), "bytes; batches", state["b"])


def _ell_hp_one(key):
    import ell_hp_ref
    return key, ell_hp_ref.case_record(key)


def gen_ell_hp(out):
    """High-precision results (mpmath, 50 digits) of the ellipsoid linear algebra on the seeded cases of
    tests/ell_cases.py (tests/test_ell_hp_cpu.py, tests/test_gpu_ell_hp.py).  Nothing of the reference project is
    involved: the reference here is tests/ell_hp_ref.py.  Outputs only -- the inputs are regenerated from their seeds.
    A quarter of an hour of mpmath, spread over the processors."""
    import multiprocessing
    import ell_hp_ref
    keys = ell_hp_ref.all_case_keys()
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        records = dict(pool.imap_unordered(_ell_hp_one, keys, chunksize=1))
    g = ell_hp_ref.pack_fixture(records)
    np.savez_compressed(out, **g)
    print("wrote", out, len(keys), "cases,", len(g), "arrays")


def _friends_hp_one(job):
    import friends_hp_ref
    if isinstance(job, tuple):
        return job, friends_hp_ref.within_record(*job)
    return job, friends_hp_ref.update_record(job)


def gen_friends_hp(out):
    """High-precision results (mpmath, 50 digits) of the RadFriends / SupFriends checks on the seeded cases of
    tests/friends_cases.py (tests/test_friends_hp_cpu.py, tests/test_gpu_friends_hp.py): partitions and their margins,
    spectra and square roots of the exact covariances, the membership distances next to the threshold.  Nothing of the
    reference project is involved: the reference here is tests/friends_hp_ref.py.  Outputs only -- the inputs are
    regenerated from their seeds.  A few minutes of mpmath, spread over the processors."""
    import multiprocessing
    import friends_hp_ref
    ukeys, wkeys = friends_hp_ref.all_keys()
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        records = dict(pool.imap_unordered(_friends_hp_one, ukeys + wkeys, chunksize=1))
    g = friends_hp_ref.pack_fixture({k: records[k] for k in ukeys}, {k: records[k] for k in wkeys})
    np.savez_compressed(out, **g)
    print("wrote", out, len(ukeys), "update cases,", len(wkeys), "membership cases,", len(g), "arrays")


def _proposal_hp_one(key):
    import proposal_hp_ref
    if key.startswith("chain/"):
        return key, proposal_hp_ref.chain_record(key)
    if key.startswith("slice/"):
        return key, proposal_hp_ref.slice_record(key)
    return key, proposal_hp_ref.step_record(key)


def gen_proposal_hp(out):
    """High-precision results (mpmath, 50 digits; np.longdouble) of the proposal geometry on the seeded cases of
    tests/proposal_cases.py (tests/test_proposal_hp_cpu.py, tests/test_gpu_proposal_hp.py): ur^(1/n) / |z| of every
    one-step walker and of every draw inside an ellipsoid, the constructed generator states, and the end points,
    accumulated bounds and counts of the rwalk chains and of the rslice / slice cases.  Nothing of the reference
    project is involved: the reference here is tests/proposal_hp_ref.py.  Refuses to write a one-step case with an
    undecidable walker or a chain or slice case above the 2 % cap.  Half a minute on 16 processors."""
    import multiprocessing
    import proposal_hp_ref
    skeys, ekeys, ckeys = proposal_hp_ref.all_keys()
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        records = dict(pool.imap_unordered(_proposal_hp_one, ckeys + skeys + ekeys, chunksize=1))
    for k in skeys + ekeys:
        assert records[k]["undecidable"] == 0, f"{k}: {records[k]['undecidable']} undecidable walkers: choose other inputs"
    for k in ekeys:
        print(k, "constructed in at most", records[k]["tries"], "tries")
    for k in ckeys:
        if k.startswith("slice/"):
            proposal_hp_ref.check_slice_caps(records[k], k)
            print(k, "undecidable", int(records[k]["undecidable"].sum()), "smallest margin %.3g" % records[k]["margin"],
                  "calls", int(records[k]["ncalls"].sum()), "expansions", int(records[k]["n_expand"].sum()),
                  "contractions", int(records[k]["n_contract"].sum()))
            continue
        proposal_hp_ref.check_caps(records[k], k)
        print(k, "undecidable", int(records[k]["undecidable"].sum()), "smallest margin %.3g" % records[k]["margin"],
              "accepts", int(records[k]["accept"].sum()), "rejects", int(records[k]["reject"].sum()))
    g = proposal_hp_ref.pack_fixture(records)
    np.savez_compressed(out, **g)
    print("wrote", out, len(skeys), "one-step sets,", len(ekeys), "constructed sets,", len(ckeys), "chains,", len(g), "arrays")


def _ns_hp_one(key):
    import ns_hp_ref
    return ns_hp_ref.golden_record(key)


def gen_ns_hp(out):
    """High-precision results (mpmath, 50 digits) of the run loop's evidence integration on the seeded fill chains of
    tests/ns_cases.py (tests/test_ns_hp_cpu.py, tests/test_gpu_ns_hp.py): ln X, ln Z, H and var ln Z after every fill,
    and where the `stop` cases stop.  Nothing of the reference project is involved: the reference here is
    tests/ns_hp_ref.py.  Outputs only -- the inputs are regenerated from their seeds.  A few seconds on 16 processors."""
    import multiprocessing
    import ns_cases
    keys = ns_cases.all_keys()
    g = {}
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        for rec in pool.imap_unordered(_ns_hp_one, keys, chunksize=1):
            g.update(rec)
    np.savez_compressed(out, **g)
    print("wrote", out, len(keys), "cases,", len(g), "arrays,", os.path.getsize(out), "bytes")


def _split_hp_one(key):
    import split_hp_ref
    return key, (split_hp_ref.boot_record(key) if key.startswith("boot/") else split_hp_ref.case_record(key))


def gen_split_hp(out):
    """High-precision results (mpmath, 50 digits; np.longdouble) of MultiEllipsoid.update's split tree on the seeded
    clouds of tests/split_cases.py (tests/test_split_hp_cpu.py, tests/test_gpu_split_hp.py): the leaf of every point in
    list order, nnodes, every leaf's ellipsoid record, every k-means node's decisions with margin / bound, and the
    bootstrap expansion of the replicas.  Nothing of the reference project is involved: the reference here is
    tests/split_hp_ref.py.  Outputs only -- the inputs are regenerated from their seeds.  Refuses to write a case with
    an undecidable decision.  A minute on 8 processors."""
    import multiprocessing
    import split_cases
    import split_hp_ref
    bkeys = [c[0] for c in split_cases.BOOT_CASES]
    # the long cases first
    def cost(k):
        p = k.split("/")[1:] if k.startswith("boot/") else k.split("/")
        return -int(p[1])**3 * int(p[2])
    order = sorted(split_cases.KEYS + bkeys, key=cost)
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        records = dict(pool.imap_unordered(_split_hp_one, order, chunksize=1))
    for k in split_cases.KEYS:
        r = split_hp_ref.decidability(records[k])
        print(k, "nells", int(records[k]["head"][0]), "nnodes", int(records[k]["head"][1]), "smallest margin / bound %.3g" % r)
        assert r > 1, f"{k}: a decision is within its bound of a tie (margin / bound = {r:.3g}): choose another cloud"
    for k in bkeys:
        print(k, "n_in", records[k]["nin"], "expand^2", records[k]["q2"], "bound", records[k]["q2b"])
        assert np.all(records[k]["decid"] > 1), f"{k}: a replica's tree has an undecidable decision"
    g = {"split/" + n: v for n, v in split_hp_ref.pack_fixture(records, split_cases.KEYS).items()}
    g.update({"boot/" + n: v for n, v in split_hp_ref.pack_fixture(records, bkeys).items()})
    np.savez_compressed(out, **g)
    print("wrote", out, len(split_cases.KEYS), "trees,", len(bkeys), "bootstrap cases,", len(g), "arrays,",
          os.path.getsize(out), "bytes")


if __name__ == "__main__":
    gdir = os.path.join(ROOT, "tests", "golden")
    os.makedirs(gdir, exist_ok=True)
    which = sys.argv[1:] or ["bounding", "proposals", "rng", "runs", "friends", "wide", "nsloop"]
    if "split_hp" in which:  # not in the default list; needs no reference project (tests/split_hp_ref.py)
        gen_split_hp(os.path.join(gdir, "split_hp.npz"))
        which = [w for w in which if w != "split_hp"]
        if not which:
            sys.exit(0)
    if "ns_hp" in which:  # not in the default list; needs no reference project (tests/ns_hp_ref.py is the reference)
        gen_ns_hp(os.path.join(gdir, "ns_hp.npz"))
        which = [w for w in which if w != "ns_hp"]
        if not which:
            sys.exit(0)
    if "proposal_hp" in which:  # not in the default list; needs no reference project (tests/proposal_hp_ref.py)
        gen_proposal_hp(os.path.join(gdir, "proposal_hp.npz"))
        which = [w for w in which if w != "proposal_hp"]
        if not which:
            sys.exit(0)
    if "friends_hp" in which:  # not in the default list; needs no reference project (tests/friends_hp_ref.py)
        gen_friends_hp(os.path.join(gdir, "friends_hp.npz"))
        which = [w for w in which if w != "friends_hp"]
        if not which:
            sys.exit(0)
    if "ell_hp" in which:  # not in the default list; needs no reference project (tests/ell_hp_ref.py is the reference)
        gen_ell_hp(os.path.join(gdir, "ell_hp.npz"))
        which = [w for w in which if w != "ell_hp"]
        if not which:
            sys.exit(0)
    import_reference()
    if "bounding" in which:
        gen_bounding(os.path.join(gdir, "bounding.npz"))
    if "proposals" in which:
        gen_proposals(os.path.join(gdir, "proposals.npz"))
    if "rng" in which:
        gen_rng(os.path.join(gdir, "rng.npz"))
    if "runs" in which:
        gen_runs(os.path.join(gdir, "runs.npz"))
    if "friends" in which:
        gen_friends(os.path.join(gdir, "friends.npz"))
    if "wide" in which:
        gen_wide(os.path.join(gdir, "wide.npz"))
    if "nsloop" in which:
        gen_nsloop(os.path.join(gdir, "nsloop.npz"))
    if "merge" in which:  # not in the default list: tests/test_merge_cpu.py
        gen_merge(os.path.join(gdir, "merge.npz"))
    if "merge_device" in which:  # not in the default list; reads merge.npz, which stays as it is
        gen_merge_device(os.path.join(gdir, "merge_device.npz"), os.path.join(gdir, "merge.npz"))
    if "merge_marginals" in which:  # not in the default list; reads merge.npz, which stays as it is
        gen_merge_marginals(os.path.join(gdir, "merge_marginals.npz"), os.path.join(gdir, "merge.npz"))
    if "merge_errors" in which:  # not in the default list; reads merge.npz, which stays as it is
        gen_merge_errors(os.path.join(gdir, "merge_errors.npz"), os.path.join(gdir, "merge.npz"))
    if "merge_bootstrap" in which:  # not in the default list; reads merge.npz, which stays as it is
        gen_merge_bootstrap(os.path.join(gdir, "merge_bootstrap.npz"), os.path.join(gdir, "merge.npz"))
    if "merge_dynamic" in which:  # not in the default list; reads merge.npz, which stays as it is
        gen_merge_dynamic(os.path.join(gdir, "merge_dynamic.npz"), os.path.join(gdir, "merge.npz"))
    if "batch" in which:  # not in the default list: tests/test_dynamic_cpu.py
        gen_batch(os.path.join(gdir, "batch_combine.npz"))
    if "livesets" in which:  # not in the default list: two partial reference runs (minutes)
        gen_livesets(os.path.join(gdir, "livesets.npz"))
