"""The device combiner's interface without a device: its symbols are declared, exported and bound; `keep=` and
`merge=` reach the backend as documented."""
import ctypes

import numpy as np
import pytest

from test_abi import header_functions

NEW = ("dh_ns_keep", "dh_ns_release", "dh_merge_runs", "dh_merge_kept", "dh_merged_fetch", "dh_merged_moments",
       "dh_merged_resample", "dh_merged_gather", "dh_merged_release")


def test_new_symbols_declared_exported_and_bound():
    from dynesty_amd import _lib
    fns = header_functions()
    lib = ctypes.CDLL(_lib.lib_path())
    for name in NEW:
        assert name in fns, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(fns[name]), name
    assert len(fns["dh_merge_runs"]) == 16 and len(fns["dh_merge_kept"]) == 4
    assert lib.dh_version() == 100


def test_field_codes_match_the_header():
    import os
    import re
    from dynesty_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "dynhip.h")).read()
    codes = {k.lower(): int(v) for k, v in re.findall(r"DH_MERGED_(\w+) = (\d+)", txt)}
    names = dict(weights="weight", samples_run="run", samples_seq="seq", samples_id="id", samples_it="it")
    assert len(codes) == len(_lib.MERGED_FIELDS) == 16
    for name, (code, _, _) in _lib.MERGED_FIELDS.items():
        assert codes[names.get(name, name)] == code, name


class FakeBackend:
    """Records what run_ensemble_merged asks of the backend."""

    def __init__(self):
        self.calls = []

    def ns_ensemble(self, prob, runs, nlive, queue_size, **kw):
        self.calls.append(("ns_ensemble", kw))
        out = dict(status=np.zeros(runs, dtype=np.int64), niter=np.full(runs, 2), logz=np.zeros(runs))
        if kw.get("want_samples"):
            rng = np.random.default_rng(0)
            out.update(dead_logl=np.sort(rng.random((runs, 2))) - 2, live_logl=rng.random((runs, nlive)),
                       dead_u=rng.random((runs, 2, 2)), live_u=rng.random((runs, nlive, 2)),
                       dead_id=np.zeros((runs, 2), dtype=np.int32), dead_it=np.zeros((runs, 2), dtype=np.int32),
                       dead_nc=np.ones((runs, 2), dtype=np.int32), live_it=np.zeros((runs, nlive), dtype=np.int32))
        return out

    def merge_kept(self, prob):
        self.calls.append(("merge_kept", prob))
        return dict(summary="device")

    def release_kept(self):
        self.calls.append(("release_kept",))

    def problem_eval(self, prob, u):
        return np.asarray(u) * 2, None


@pytest.fixture
def fake():
    from dynesty_amd import backend
    fb = FakeBackend()
    backend.set_backend(fb)
    yield fb
    backend.set_backend(None)


def test_merge_device_routing(fake):
    from dynesty_amd import ensemble
    m = ensemble.run_ensemble_merged("prob", 3, nlive=8, queue_size=4, merge='device', walks=5)
    assert [c[0] for c in fake.calls] == ["ns_ensemble", "merge_kept", "release_kept"]
    kw = fake.calls[0][1]
    assert kw["keep"] is True and kw["want_samples"] is False and kw["walks"] == 5
    assert fake.calls[1][1] == "prob"
    assert m["summary"] == "device" and "dead_u" not in m["runs"]


def test_merge_host_is_the_default_and_unchanged(fake):
    from dynesty_amd import ensemble
    m = ensemble.run_ensemble_merged("prob", 3, nlive=8, queue_size=4)
    assert [c[0] for c in fake.calls] == ["ns_ensemble"]
    kw = fake.calls[0][1]
    assert kw["want_samples"] is True and "keep" not in kw
    assert isinstance(m, ensemble.MergedRun) and m.niter == 3 * (2 + 8)
    np.testing.assert_array_equal(m.samples, m.samples_u * 2)


@pytest.mark.parametrize("bad", ["gpu", None, "Device", 1])
def test_merge_values_other_than_the_two_raise(fake, bad):
    from dynesty_amd import ensemble
    with pytest.raises(ValueError, match="merge="):
        ensemble.run_ensemble_merged("prob", 3, nlive=8, queue_size=4, merge=bad)
    assert fake.calls == []


def test_ns_ensemble_takes_keep():
    import inspect
    from dynesty_amd import _lib
    sig = inspect.signature(_lib.Context.ns_ensemble)
    assert sig.parameters["keep"].default is False
    assert {"merge_runs", "merge_kept", "release_kept"} <= set(dir(_lib.Context))
    for name in ("field", "mean_and_cov", "importance_weights", "resample_equal", "to_merged_run", "release"):
        assert hasattr(_lib.DeviceMergedRun, name)
