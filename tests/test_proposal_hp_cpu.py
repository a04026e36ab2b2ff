"""tests/proposal_hp_ref.py without a device: the bounds are neither wrong nor vacuous.

  * the fixture tests/golden/proposal_hp.npz is what the generator produces now (a sample of records recomputed from
    scratch: mpmath radius and norm, the chain replay);
  * the float64 oracle (oracle.proposals_ref.propose_ball / rwalk / rslice / pslice) is within every bound on every
    case -- the worst error / bound per family is printed; a failure here means the derivation is wrong, not a constant too small;
  * no one-step case has an undecidable walker, every chain and slice case is within the 2 % cap, every chain keeps
    both outcomes;
  * the constructed generator states reproduce their target uniforms (0, 2^-53, 2^-30, 1 - 2^-53);
  * a radius wrong by 1e-13 relative (what a dropped Newton step of csrc/walkq.hip's root_n leaves) and a reflection of
    the wrong parity are rejected, while the first passes the 1e-12 the existing device tests apply;
  * how much tighter the bounds are than that 1e-12, per family.
"""
import numpy as np
import pytest

import proposal_cases as PC
import proposal_hp_ref as H
from oracle import proposals_ref as P


@pytest.fixture(scope="module")
def fix():
    return H.load_fixture()


def _bc_kw(bc):
    if bc is None:
        return {}
    # (the oracle's unitcheck takes min() of the hard coordinates: with none of them -- D = 1, 2 -- it is given no
    # mask, and asks 0 < u < 1 of coordinates that the wrap has put into [0, 1) already)
    return dict(periodic=np.where(bc == 1)[0], reflective=np.where(bc == 2)[0],
                nonbounded=bc == 0 if (bc == 0).any() else None)


def oracle_step(inp):
    k = inp["k"]
    u, ins, end = np.empty((k, inp["d"])), np.empty(k, dtype=bool), np.empty((k, 4), dtype=np.uint64)
    for i in range(k):
        g = PC.generator_of(inp["states"][i])
        up, fail = P.propose_ball(inp["u0"][i].copy(), inp["scale"], inp["axes"][inp["idx"][i]], inp["nc"], g,
                                  **_bc_kw(inp["bc"]))
        ins[i] = not fail
        u[i] = inp["u0"][i] if fail else up
        end[i] = PC.state_words(g.bit_generator)
    return dict(u=u, inside=ins, reject=(~ins).astype(np.int32), end=end)


def oracle_chain(inp):
    k, d, prob = inp["k"], inp["d"], inp["problem"]
    out = dict(u=np.empty((k, d)), v=np.empty((k, d)), logl=np.empty(k), accept=np.empty(k, dtype=np.int32),
               reject=np.empty(k, dtype=np.int32), end=np.empty((k, 4), dtype=np.uint64))
    for i in range(k):
        g = PC.generator_of(inp["states"][i])
        r = P.rwalk(inp["u0"][i].copy(), inp["loglstar"], inp["axes"][inp["idx"][i]], inp["scale"],
                    prob.prior_transform, prob.loglikelihood, g, inp["walks"], **_bc_kw(inp["bc"]))
        for name in ("u", "v", "logl", "accept", "reject"):
            out[name][i] = r[name]
        out["end"][i] = PC.state_words(g.bit_generator)
    return out


def oracle_slice(inp):
    k, d, prob = inp["k"], inp["d"], inp["problem"]
    out = dict(u=np.empty((k, d)), v=np.empty((k, d)), logl=np.empty(k), ncalls=np.empty(k, dtype=np.int32),
               n_expand=np.empty(k, dtype=np.int32), n_contract=np.empty(k, dtype=np.int32),
               expansion_warning_set=np.zeros(k, dtype=bool), end=np.empty((k, 4), dtype=np.uint64))
    fn = P.pslice if inp["principal"] else P.rslice
    for i in range(k):
        g = PC.generator_of(inp["states"][i])
        r = fn(inp["u0"][i].copy(), inp["loglstar"], inp["axes"][inp["idx"][i]], inp["scale"], prob.prior_transform,
               prob.loglikelihood, g, inp["slices"], doubling=inp["doubling"])
        for name in ("u", "v", "logl", "ncalls", "n_expand", "n_contract", "expansion_warning_set"):
            out[name][i] = r[name]
        out["end"][i] = PC.state_words(g.bit_generator)
    return out


def fp64_step(inp, radius_factor=1.0, flip_reflection=False):
    """A float64 step of this file's own (internal_samplers.py:989-1035), with two faults to switch on."""
    z, ur, extra, end = H.draws(inp)
    k, nc, bc = inp["k"], inp["nc"], inp["bc"]
    u, ins = np.empty((k, inp["d"])), np.empty(k, dtype=bool)
    for i in range(k):
        r = ur[i, 0]**(1.0 / nc) * radius_factor
        du = inp["axes"][inp["idx"][i]] @ (z[i, 0] * (r / np.linalg.norm(z[i, 0])))
        up = np.concatenate([inp["u0"][i, :nc] + inp["scale"] * du, extra[i, 0]])
        hard = np.ones(len(up), dtype=bool)
        if bc is not None:
            hard = bc == PC.BC_HARD
            per, ref = bc == PC.BC_PERIODIC, bc == PC.BC_REFLECT
            up[per] = np.mod(up[per], 1)
            even = (np.mod(up[ref], 2) < 1) != flip_reflection
            up[ref] = np.where(even, np.mod(up[ref], 1), 1 - np.mod(up[ref], 1))
        ins[i] = np.all((up[hard] > 0) & (up[hard] < 1))
        u[i] = up if ins[i] else inp["u0"][i]
    return dict(u=u, inside=ins, reject=(~ins).astype(np.int32), end=end)


def test_case_list_is_complete(fix):
    skeys, ekeys, ckeys = H.all_keys()
    keys = skeys + ekeys + ckeys
    assert len(keys) == len(set(keys)) and sorted(fix) == sorted(keys)
    entries = PC.step_entries() + PC.edge_entries() + PC.chain_entries()
    # every input set is run by some form, every form's set exists
    assert {k for _, k in entries} | set(PC.slice_keys()) | set(PC.draw_keys()) == set(keys)

    def dims(entry, group):
        return sorted({int(k.split("/")[1]) for e, k in PC.step_entries() if e == entry and k.endswith("/" + group)
                       and k.split("/")[1] == k.split("/")[2]})
    for g in PC.GROUPS:
        assert dims("quad", g) == list(range(2, 33))
        assert dims("lane", g) == [1, 2, 3, 4, 5, 8, 9, 16, 17, 25, 31, 32]
        assert dims("propose", g) == [5, 25]
        assert dims("wide", g) == [33, 40, 64, 65, 128, 200, 257, 512]
        assert ("lane", PC.step_key(5, 3, 83, g)) in entries and ("lane", PC.step_key(25, 7, 83, g)) in entries
        assert any(e == "quadf" for e, k in entries if k.endswith("/" + g))
    assert {(e, k) for e, k in entries if k.startswith("step/") and k.split("/")[3] == "5"} == \
        {("wide", PC.step_key(d, d, 5, "A")) for d in PC.WIDE_DIMS}
    assert sorted(int(k.split("/")[1]) for k in ekeys) == [2, 5, 25, 32, 40]
    assert {k.split("/")[2] for k in PC.chain_keys()} == {"prec", "iid", "normal", "egg"}
    assert "chain/25/prec/45/T" in ckeys and "chain/40/normal/10/E" in ckeys and "chain/8/prec/20/BC" in ckeys
    sl = {tuple(k.split("/")[1:3]) + (k.split("/")[5], k.split("/")[6]) for k in PC.slice_keys()}
    for form, d in (("r", "5"), ("r", "9"), ("p", "5"), ("p", "7")):
        assert (form, d, "0", "T") in sl and (form, d, "1", "T") in sl
    assert ("r", "40", "0", "T") in sl and ("r", "5", "0", "E") in sl and ("p", "5", "0", "E") in sl
    assert set(PC.feed_keys()) <= set(PC.slice_keys())


SAMPLE = ["draw/unif/3", "draw/bound/25", "draw/multi/5", "draw/unifmulti/5", "step/1/1/83/C", "step/2/2/83/A", "step/5/3/83/C",
          "step/13/13/83/B", "step/25/25/83/A", "step/40/40/9/C",
          "step/512/512/5/A"]


@pytest.mark.parametrize("key", SAMPLE + PC.edge_keys() + ["chain/2/egg/18/E", "chain/7/iid/18/T", "slice/r/5/prec/3/1/T",
                                                            "slice/r/5/iid/3/0/E"])
def test_fixture_is_what_the_generator_produces(fix, key):
    rec = H.chain_record(key) if key.startswith("chain/") else H.slice_record(key) if key.startswith("slice/") \
        else H.step_record(key)
    for name, have in fix[key].items():
        np.testing.assert_array_equal(np.asarray(rec[name]), np.asarray(have), err_msg=f"{key} {name}")


def test_constructed_states_reproduce_their_targets(fix):
    for key in PC.edge_keys():
        inp = H.inputs_of(key, fix)
        _, ur, _, _ = H.draws(inp)
        np.testing.assert_array_equal(ur[:, 0], PC.edge_targets().astype(np.float64) * 2.0**-53, err_msg=key)
        assert ur[0, 0] == 0.0 and np.float32(ur[3, 0]) == 1.0 and ur[1, 0] == 2.0**-53 and ur[2, 0] == 2.0**-30


def test_no_one_step_case_is_undecidable_and_chains_are_within_the_cap(fix):
    skeys, ekeys, ckeys = H.all_keys()
    for key in skeys + ekeys:
        assert fix[key]["undecidable"] == 0 and fix[key]["margin"] > 1.0, key
    some_rejects = 0
    for key in skeys:
        if key.endswith("/A"):
            some_rejects += int((fix[key]["inside"] == 0).sum())
        else:
            assert np.all(fix[key]["inside"] != 0), key
    assert some_rejects > 30  # the long family leaves the cube now and then: u0 must come back, with reject = 1
    for key in ckeys:
        if key.startswith("slice/"):
            H.check_slice_caps(fix[key], key)
            assert fix[key]["n_expand"].sum() > 0 and np.all(fix[key]["n_contract"] >= 1)
        else:
            H.check_caps(fix[key], key)
        print(f"proposal_hp {key}: undecidable {int(fix[key]['undecidable'].sum())} of {len(fix[key]['undecidable'])}, "
              f"smallest margin {fix[key]['margin']:.3g}")


def test_oracle_is_within_the_bounds_one_step(fix):
    skeys, ekeys, _ = H.all_keys()
    worst = {}
    bad = []
    for key in skeys + ekeys:
        inp = H.inputs_of(key, fix)
        r = H.check_step(inp, fix[key], oracle_step(inp), key)
        fam = key.split("/")[-1] if key.startswith("step/") else key.split("/")[0]
        fam += "/wide" if inp["d"] > 32 else ""
        worst.setdefault(fam, H.Ratios()).merge(r)
        if not all(v <= 1.0 for v in r.values()):
            bad.append((key, dict(r)))
    for fam, r in sorted(worst.items()):
        print(f"proposal_hp WORST oracle one step {fam}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert not bad, bad[:6]


@pytest.mark.parametrize("key", PC.chain_keys())
def test_oracle_is_within_the_bounds_chain(fix, key):
    inp = H.inputs_of(key, fix)
    r = H.check_chain(inp, fix[key], oracle_chain(inp), key)
    r.assert_ok(f"oracle {key}")


def test_oracle_membership_counts_of_the_three_ellipsoids(fix):
    """The draws' x, idx and q as the oracle's multi_sample(return_q=True) makes them, off the one generator."""
    from oracle import bounding_ref as B
    key = "draw/multi/5"
    inp = H.inputs_of(key, fix)
    lens = np.linalg.norm(inp["axes"], axis=1)
    m = B.stack_ells([B.Ell(inp["ctrs"][j], np.linalg.inv(inp["ams"][j]), inp["ams"][j], inp["axes"][j], lens[j],
                            float(inp["logvol_ells"][j])) for j in range(3)])
    g = PC.generator_of(inp["state0"])
    got = [B.multi_sample(m, g, return_q=True) for _ in range(inp["k"])]
    np.testing.assert_array_equal([i for _, i, _ in got], inp["idx"])
    xs = np.array([x for x, _, _ in got])
    assert H.check_membership(inp, xs, [q for _, _, q in got], key) > 0.98
    r = H.check_step(inp, fix[key], dict(u=xs, inside=np.ones(inp["k"], dtype=bool)), key)
    r.assert_ok("oracle multi_sample")
    np.testing.assert_array_equal(PC.state_words(g.bit_generator), H.draws(inp)[3][-1])


def test_oracle_uniform_sampler_over_the_three_ellipsoids(fix):
    """UniformBoundSampler.sample over the oracle's multi_sample from the walkers' start states: the point that is kept
    at the bound of its one step, one likelihood call, and the generator where the NumPy walk of the inputs left it."""
    from oracle import bounding_ref as B
    key = "draw/unifmulti/5"
    inp = H.inputs_of(key, fix)
    prob = inp["problem"]
    lens = np.linalg.norm(inp["axes"], axis=1)
    m = B.stack_ells([B.Ell(inp["ctrs"][j], np.linalg.inv(inp["ams"][j]), inp["ams"][j], inp["axes"][j], lens[j],
                            float(inp["logvol_ells"][j])) for j in range(3)])
    u = np.empty((inp["k"], inp["d"]))
    for i in range(inp["k"]):
        g = PC.generator_of(inp["start"][i])
        r = P.unif_bound(inp["loglstar"], P.unif_multi(m), prob.prior_transform, prob.loglikelihood, g, inp["d"], inp["d"])
        assert r["ncalls"] == 1
        u[i] = r["u"]
        np.testing.assert_array_equal(PC.state_words(g.bit_generator), inp["end"][i])
    H.check_step(inp, fix[key], dict(u=u, inside=np.ones(inp["k"], dtype=bool)), key).assert_ok("oracle unif_bound, 3 ellipsoids")


def test_the_four_lane_bound_has_no_exponent_term():
    """root_n is a Newton iteration on y^n = ur: at ur = 2^-53, n = 2 its step coefficient is 13 eps + 8e-16, where a
    pow evaluator's carries 18 eps more."""
    lane, quad = float(H.step_coeff(2, 2.0**-53)), float(H.step_coeff(2, 2.0**-53, exponent=False))
    assert quad == (2 + 1.5 + 2) * H.EPS + H.G_RSQ + H.G_ROOT
    assert abs((lane - quad) / H.EPS - 53 * np.log(2.0) / 2) < 1e-9


def _fma(a, b, c):
    from fractions import Fraction as Fr
    return float(Fr(float(a)) * Fr(float(b)) + Fr(float(c)))


def test_slices_with_fused_multiply_adds_are_within_the_bounds(fix, monkeypatch):
    """The oracle's slice step with exact fused multiply-adds in the two places slice_kernel has them --
    x = fma(r, width, left) and u + x direction -- on the principal-axes doubling case: the contraction drops the
    rounding of r * width, half an ulp of the window, which is what the abscissa grant of slice_walker is derived
    from.  Counts, end states and the bound hold."""
    import inspect
    src = inspect.getsource(P.slice_step)
    assert "x = left + rng.random() * width" in src and "u_new = u + x * direction" in src
    src = src.replace("x = left + rng.random() * width", "x = _fma(rng.random(), width, left)")
    src = src.replace("u_new = u + x * direction",
                      "u_new = np.array([_fma(x, direction[i], u[i]) for i in range(len(u))])")
    ns = dict(P.__dict__, _fma=_fma)
    exec(src, ns)
    monkeypatch.setattr(P, "slice_step", ns["slice_step"])
    key = "slice/p/5/prec/3/1/T"
    inp = H.inputs_of(key, fix)
    H.check_slice(inp, fix[key], oracle_slice(inp), key).assert_ok(f"fused multiply-adds {key}")


@pytest.mark.parametrize("key", PC.slice_keys())
def test_oracle_is_within_the_bounds_slice(fix, key):
    inp = H.inputs_of(key, fix)
    r = H.check_slice(inp, fix[key], oracle_slice(inp), key)
    if key in PC.feed_keys():
        dirs = np.array([inp["axes"][inp["idx"][i]] @ (lambda z: z / np.linalg.norm(z))(
            PC.generator_of(inp["states"][i]).standard_normal(inp["d"])) * inp["scale"] for i in range(inp["k"])])
        r.merge(H.check_feed(inp, fix[key], dirs, key))
        bad = H.check_feed(inp, fix[key], dirs * (1.0 + 1e-13), key)
        assert bad["direction"] > 1.0  # a direction 1e-13 too long is rejected
    r.assert_ok(f"oracle {key}")


@pytest.mark.parametrize("d", [2, 5, 13, 25, 32])
def test_a_radius_wrong_by_1e_13_is_rejected(fix, d):
    """What one Newton step less in root_n leaves: invisible at atol = 1e-12, counts unchanged."""
    key = PC.step_key(d, d, PC.K, "A")
    inp = H.inputs_of(key, fix)
    good, bad = fp64_step(inp), fp64_step(inp, radius_factor=1.0 + 1e-13)
    assert H.check_step(inp, fix[key], good, key)["u"] <= 1.0
    r = H.check_step(inp, fix[key], bad, key)  # inside flags, counts, end states: all as they should be
    print(f"proposal_hp wrong radius D={d}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert r["u"] > 1.0 and r["step"] > 1.0
    assert np.max(np.abs(bad["u"] - good["u"])) < 1e-13  # ... and a tenth of the old tolerance


@pytest.mark.parametrize("d", [2, 5, 25])
def test_a_reflection_of_the_wrong_parity_is_rejected(fix, d):
    key = PC.step_key(d, d, PC.K, "C")
    inp = H.inputs_of(key, fix)
    assert H.check_step(inp, fix[key], fp64_step(inp), key)["u"] <= 1.0
    r = H.check_step(inp, fix[key], fp64_step(inp, flip_reflection=True), key)
    assert r["u"] > 1e6


def test_how_much_tighter_than_1e_12(fix):
    """The largest bound of every family against the hand-set 1e-12 of tests/test_gpu_rwalkq.py, D <= 32."""
    top = {}
    for key in [s[0] for s in PC.step_sets() if s[1] <= 32]:
        inp = H.inputs_of(key, fix)
        ref = H.step_reference(inp, fix[key]["g_hi"], fix[key]["g_lo"])
        for f, fam in enumerate(PC.FAMILIES[inp["group"]]):
            b = ref["bound"][inp["idx"] == f][:, :inp["nc"]]
            top[fam] = max(top.get(fam, 0.0), float(b.max()))
    for fam, b in top.items():
        print(f"proposal_hp largest bound, {fam}: {b:.3g}  (1e-12 is {1e-12 / b:.3g} times that)")
    for fam in ("today", "long", "kappa", "late", "klate", "late2"):
        assert top[fam] < 1e-14
    assert top["late"] < 1e-16 and top["klate"] < 1e-16
