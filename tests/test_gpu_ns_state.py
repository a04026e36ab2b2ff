"""dh_ns_state_export / dh_ns_state_import: a kept ensemble saved, restored in another context, and taken further to
what the uninterrupted run gives, bit for bit; the image's size; more capacity on import; the checkpointed runner;
and the rejections, each of which leaves the context's kept ensemble as it was."""
import numpy as np
import pytest

import inputs
from test_gpu_ns_continue import CONFIGS, DLOGZ, K, MAX_ITER, NLIVE, RUNS, assert_same_runs, base_kw, full_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def saved_after_first_leg(ctx, cfg, **over):
    prob, kw = base_kw(cfg)
    kw.update(over)
    try:
        leg = ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=150, **kw)
        assert (leg["niter"] == 151).all()
        return ctx.ns_state()
    finally:
        ctx.release_kept()


@pytest.mark.parametrize("cfg", ["rwalk-multi", "unif-balls-boot5"])
def test_save_load_continue_in_a_new_context(ctx, cfg, tmp_path):
    from dynesty_amd import _lib
    ref = full_run(ctx, cfg)
    prob, kw = base_kw(cfg)
    path = tmp_path / "ensemble.dhns"
    try:
        ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=150, **kw)
        ctx.ns_save(path)
    finally:
        ctx.release_kept()
    other = _lib.Context(0)
    try:
        other.ns_load(inputs.problem(CONFIGS[cfg][0]), path)  # (the problem created anew)
        got = other.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        other.close()
    assert (got["rest"] > 0).any()
    assert_same_runs(got, ref)


def test_image_size_does_not_depend_on_max_iter(ctx):
    a = saved_after_first_leg(ctx, "rwalk-multi", max_iter=20000)
    b = saved_after_first_leg(ctx, "rwalk-multi", max_iter=200000)
    assert a.dtype == np.uint8 and a.size == b.size
    # ... and is what 151 dead points per run take, not what the capacity would
    assert a.size < 20000 * RUNS * 8


def test_import_with_more_capacity(ctx):
    prob, kw = base_kw("rwalk-multi")
    kw["max_iter"] = 40000
    ref = ctx.ns_ensemble(prob, dlogz=DLOGZ, want_samples=True, **kw)
    img = saved_after_first_leg(ctx, "rwalk-multi", max_iter=3000)
    try:
        ctx.ns_load(prob, img, max_iter=40000)
        got = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert got["dead_logl"].shape == (RUNS, 40000)
    assert_same_runs(got, ref)
    assert_same_runs(got, full_run(ctx, "rwalk-multi"))  # (the capacity is no part of the result)


def test_checkpointed_run_interrupted_and_resumed(ctx, tmp_path):
    from dynesty_amd import _lib, backend, ensemble
    ref = full_run(ctx, "rwalk-multi")
    prob, kw = base_kw("rwalk-multi")
    path = str(tmp_path / "ckpt.dhns")
    run_kw = {k: v for k, v in kw.items() if k not in ("runs", "nlive", "queue_size")}
    prev = backend._active
    try:
        backend.set_backend(ctx)
        part = ensemble.run_ensemble_checkpointed(prob, RUNS, NLIVE, K, checkpoint_file=path, checkpoint_fills=4,
                                                  max_legs=2, dlogz=DLOGZ, **run_kw)
        assert (part["status"] == 1).all() and (part["niter"] < ref["niter"]).all()
        ctx.release_kept()  # (the interruption: what is on the device is gone, the file is what is left)
        other = _lib.Context(0)
        backend.set_backend(other)
        got = ensemble.run_ensemble_checkpointed(prob, RUNS, NLIVE, K, checkpoint_file=path, checkpoint_fills=4,
                                                 resume=True, dlogz=DLOGZ, want_samples=True, **run_kw)
        other.close()
    finally:
        backend.set_backend(prev)
    assert_same_runs(got, ref)


def test_rejected_images_leave_the_kept_ensemble_intact(ctx):
    prob, kw = base_kw("rwalk-multi")
    ref = full_run(ctx, "rwalk-multi")
    img = saved_after_first_leg(ctx, "rwalk-multi")
    hdr = 88  # csrc/ns_state.h: Header
    bad = {}
    bad["magic"] = img.copy()
    bad["magic"][0] ^= 0xFF
    bad["version"] = img.copy()
    bad["version"][8:12] = np.frombuffer(np.uint32(int(np.frombuffer(img[8:12].tobytes(), np.uint32)[0]) + 1).tobytes(),
                                         np.uint8)
    bad["one byte short"] = img[:-1].copy()
    bad["cut in the header"] = img[:hdr - 8].copy()
    try:
        ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=150, **kw)
        for what, buf in bad.items():
            with pytest.raises(ValueError):
                ctx.ns_load(prob, buf)
        with pytest.raises(ValueError, match="ndim"):
            ctx.ns_load(inputs.problem("C1"), img)
        with pytest.raises(ValueError, match="max_iter"):
            ctx.ns_load(prob, img, max_iter=100)
        got = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert_same_runs(got, ref)
