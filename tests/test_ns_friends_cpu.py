"""Context.ns_ensemble with RadFriends / SupFriends bounds, without a device: which combinations reach
dh_ns_ensemble (bound code 2 / 3 with the uniform sampler from PCG64 streams) and which are refused, and the host
mirror's restatement of the bootstrap replicas' in-sample masks."""
import numpy as np
import pytest

from dynesty_amd import _lib


class P:
    def __init__(self, ndim=2):
        self.ndim = ndim


def bare_ctx():
    return _lib.Context.__new__(_lib.Context)  # no device needed: validation comes first


@pytest.mark.parametrize("kw", [dict(bound='balls', sample='unif', rng='philox'),
                                dict(bound='cubes', sample='unif', rng='philox'),
                                dict(bound='balls', sample='rwalk'), dict(bound='balls', sample='slice'),
                                dict(bound='balls', sample='rslice'), dict(bound='cubes', sample='rwalk'),
                                dict(bound='cubes', sample='rslice'), dict(bound='none', sample='unif'),
                                dict(bound='none')])
def test_unsupported_friends_combinations_raise(kw):
    with pytest.raises(ValueError, match="not supported"):
        _lib.Context.ns_ensemble(bare_ctx(), P(), 2, 100, 16, **kw)


@pytest.mark.parametrize("bound", ["balls", "cubes"])
def test_friends_above_32_dimensions_raise(bound):
    with pytest.raises(ValueError, match="not supported"):
        _lib.Context.ns_ensemble(bare_ctx(), P(33), 2, 100, 16, bound=bound, sample='unif')


class RecordingLib:
    """Stands in for the loaded library: records every call, leaves the outputs as they are."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


@pytest.mark.parametrize("bound,code", [("balls", 2), ("cubes", 3), ("single", 0), ("multi", 1)])
def test_friends_bounds_reach_the_loop_with_their_codes(bound, code):
    ctx = bare_ctx()
    ctx.lib = RecordingLib()
    ctx.handle = None
    ctx.problem = lambda prob: 7
    _lib.Context.ns_ensemble(ctx, P(2), 3, 100, 16, bound=bound, sample='unif', bootstrap=0)
    calls = [a for n, a in ctx.lib.calls if n == "dh_ns_ensemble"]
    assert len(calls) == 1
    args = calls[0]
    # (handle, problem, runs, nlive, ndim, queue_size, sampler, walks, bound, ...)
    assert args[1] == 7 and args[2] == 3 and args[3] == 100 and args[4] == 2 and args[5] == 16
    assert args[6] == 6  # unif, PCG64 streams
    assert args[8] == code


def test_friends_defaults_are_the_references_for_unif():
    ctx = bare_ctx()
    ctx.lib = RecordingLib()
    ctx.handle = None
    ctx.problem = lambda prob: 0
    _lib.Context.ns_ensemble(ctx, P(2), 1, 50, 4, bound='cubes', sample='unif')
    args = [a for n, a in ctx.lib.calls if n == "dh_ns_ensemble"][0]
    assert args[11] == 1.0  # enlarge
    assert args[-2] == 5  # bootstrap


def test_mirror_bootstrap_masks_follow_bootstrap_points():
    """resident_friends_mirror.boot_mask against _bootstrap_points' rule (bounding.py:1593-1616) as
    dynesty_amd.bootstrap restates it, on the replica streams of fixed words (oracle.nested_ref.boot_generator),
    including the two repairs: n = 2 (fewer than two in the sample) and a draw that takes every point."""
    from resident_friends_mirror import boot_mask
    from dynesty_amd.bootstrap import resample_mask
    from oracle.nested_ref import boot_generator
    ent = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x1111222233334444, 0x5555666677778888]
    for n in (2, 3, 50, 500, 2000):
        for b in range(5):
            got = boot_mask(n, ent, b)
            want = resample_mask(n, boot_generator(ent, b))
            np.testing.assert_array_equal(got, want)
    # both repairs at n = 2: one distinct index drawn (n_in < 2: both points join) or both (n_in > n - 1: the first
    # leaves)
    seen = {}
    for b in range(64):
        k = len(np.unique(boot_generator(ent, b).integers(2, size=2)))
        seen[k] = boot_mask(2, ent, b).tolist()
    assert seen == {1: [True, True], 2: [False, True]}
