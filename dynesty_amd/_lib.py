"""ctypes binding of libdynhip.so (C ABI: include/dynhip.h).

There is deliberately **no CPU fallback**: if the shared library is missing or
no HIP device is visible, importing the backend raises.  Build the library
with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C dynesty_amd/csrc``.
"""
import ctypes as C
import os
import sys

import numpy as np

from .errors import FIELDS as REAL_FIELDS, MAX_BOOT, Errors
from .marginals import Marginals

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_ENV = "DYNHIP_LIB"

DH_OK = 0
ERR_VALUE, ERR_CONTAIN, ERR_REGION, ERR_SLICE = -1, -2, -3, -4
ERR_HIP, ERR_ARG, ERR_QZERO, ERR_NOMEM = -5, -6, -7, -8

BC_HARD, BC_PERIODIC, BC_REFLECT = 0, 1, 2
# dh_ns_ensemble bound codes
BOUND_CODES = dict(single=0, multi=1, balls=2, cubes=3)


class DynHipError(RuntimeError):
    """HIP runtime / argument failures of libdynhip (no reference analogue)."""


def lib_path():
    p = os.environ.get(LIB_ENV)
    if p:
        return p
    return os.path.join(_HERE, "libdynhip.so")


_lib = None

_vp, _i, _u32, _u64, _dbl = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
_pd = C.POINTER(C.c_double)

# name -> (restype, argtypes); kept in step with include/dynhip.h (checked by
# tests/test_abi.py, which parses the header).
SIGNATURES = {
    "dh_version": (_i, []),
    "dh_device_count": (_i, []),
    "dh_create": (_vp, [_i]),
    "dh_destroy": (None, [_vp]),
    "dh_last_error": (C.c_char_p, [_vp]),
    "dh_sync": (_i, [_vp]),
    "dh_stream": (_vp, [_vp]),
    "dh_malloc": (_vp, [_vp, _u64]),
    "dh_free": (_i, [_vp, _vp]),
    "dh_memcpy_h2d": (_i, [_vp, _vp, _vp, _u64]),
    "dh_memcpy_d2h": (_i, [_vp, _vp, _vp, _u64]),
    "dh_memset": (_i, [_vp, _vp, _i, _u64]),
    "dh_event_create": (_vp, [_vp]),
    "dh_event_destroy": (_i, [_vp, _vp]),
    "dh_event_record": (_i, [_vp, _vp]),
    "dh_event_elapsed_ms": (_i, [_vp, _vp, _vp, _pd]),
    "dh_problem_create": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i]),
    "dh_problem_create_ex": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i]),
    "dh_problem_destroy": (_i, [_vp, _i]),
    "dh_problem_eval": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "dh_seed_children": (_i, [_vp, _vp, _i, _u32, _i, _vp]),
    "dh_rng_stream": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "dh_contains": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "dh_contains_runs": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "dh_rebuild": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                        _vp, _vp, _vp]),
    "dh_rebuild_batch_dev": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_rebuild_ragged_dev": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_ell_from_cov": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "dh_improve_covar_mat": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "dh_scale_to_logvol": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_enlarge_batch_dev": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                  _dbl]),
    "dh_enlarge_runs": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _dbl, _vp, _vp]),
    "dh_rwalk_propose": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _dbl, _vp, _vp,
                              _vp, _vp, _vp]),
    "dh_rwalk_batch": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl, _dbl,
                            _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_rwalk_batch_dev": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl,
                                _dbl, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp]),
    "dh_rwalk_batch_philox": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl, _dbl, _i, _vp, _u64,
                                   _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "dh_rwalk_batch_philox_dev": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl, _dbl, _i, _vp, _u64,
                                       _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "dh_slice_batch": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl, _dbl,
                            _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp]),
    "dh_slice_batch_dev": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl,
                                _dbl, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp]),
    "dh_unif_batch": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _dbl,
                           _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "dh_unif_batch_dev": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp,
                               _dbl, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp,
                               _vp, _vp]),
    "dh_ns_consume": (_i, [_vp, _i, _i, _i, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                           _vp, _vp, _vp, _vp]),
    "dh_ns_ensemble": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _dbl, _dbl,
                            C.c_int64, C.c_int64, _vp, _i, _u32, _vp, _vp,
                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i]),
    "dh_bootstrap_expand": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "dh_friends_update": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp]),
    "dh_friends_update_batch": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _i, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_friends_within": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "dh_friends_draw": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp,
                             _vp, _vp]),
    "dh_unif_friends_batch": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _dbl,
                                   _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp]),
    "dh_bound_draw": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp,
                           _vp, _vp, _vp]),
    "dh_slice_feed": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _dbl, _vp, _vp, _i, _vp,
                           _vp, _vp]),
    "dh_set_rwalk_form": (_i, [_vp, _i]),
    "dh_ns_set_option": (_i, [_vp, _i, _dbl]),
    "dh_ns_set_boundary": (_i, [_vp, _i, _vp]),
    "dh_ns_keep": (_i, [_vp, _i]),
    "dh_ns_release": (_i, [_vp]),
    "dh_ns_continue": (_i, [_vp, _dbl, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_ns_batch": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _dbl, _dbl, C.c_int64, C.c_int64, _vp, _i, _u32,
                         _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i,
                         _vp, _vp, _vp, _vp, _vp]),
    "dh_merged_batch_seed": (_i, [_vp, _u64, C.c_int64, _i, _i, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "dh_ns_state_size": (_i, [_vp, _vp]),
    "dh_ns_state_export": (_i, [_vp, _vp, _u64]),
    "dh_ns_state_import": (_i, [_vp, _i, _vp, _u64, C.c_int64]),
    "dh_merge_runs": (_i, [_vp, _i, _i, _i, _i, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_merge_kept": (_i, [_vp, _i, _vp, _vp]),
    "dh_merged_fetch": (_i, [_vp, _i, C.c_int64, C.c_int64, _vp]),
    "dh_merged_moments": (_i, [_vp, _vp, _vp]),
    "dh_merged_resample": (_i, [_vp, _dbl, C.c_int64, _vp]),
    "dh_merged_gather": (_i, [_vp, C.c_int64, _vp, _vp]),
    "dh_merged_gather_rows": (_i, [_vp, _i, C.c_int64, _vp, _vp]),
    "dh_merged_release": (_i, [_vp]),
    "dh_merged_fold": (_i, [_vp, _i, _i, _i, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _vp]),
    "dh_merged_quantile": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "dh_merged_hist1d": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp]),
    "dh_merged_hist2d": (_i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "dh_merged_realize": (_i, [_vp, _u64, C.c_int64, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "dh_merged_realization": (_i, [_vp, _u64, C.c_int64, _i, _vp, _i, C.c_int64, C.c_int64, _vp]),
    "dh_merged_bootstrap": (_i, [_vp, _u64, C.c_int64, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "dh_merged_bootstrap_run": (_i, [_vp, _u64, C.c_int64, _i, _vp, _i, C.c_int64, C.c_int64, _vp, _vp]),
    "dh_merged_kld": (_i, [_vp, _u64, C.c_int64, _i, _i, _vp, _vp, _vp, _vp]),
    "dh_merged_weight_function": (_i, [_vp, _dbl, _dbl, C.c_int64, _vp, _vp]),
    "dh_merged_weights": (_i, [_vp, _dbl, _i, C.c_int64, C.c_int64, _vp]),
    "dh_set_rwalk_items": (_i, [_vp, _i, C.c_longlong]),
    "dh_slice_batch_philox": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl, _dbl, _i, _i, _u64, _u64, _u64,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_slice_batch_philox_dev": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _dbl, _dbl, _i, _i, _u64, _u64,
                                       _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dh_unif_batch_philox": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _dbl, _vp, _u64, _u64, _u64,
                                  C.c_int64, _vp, _vp, _vp, _vp]),
    "dh_unif_batch_philox_dev": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _dbl, _vp, _u64, _u64, _u64,
                                      C.c_int64, _vp, _vp, _vp, _vp, _vp]),
}


def load():
    """Load libdynhip.so (once) and declare every prototype."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"libdynhip.so not found at {path}: the HIP extension is required "
            "(no CPU fallback). Build it with `make -C dynesty_amd/csrc` or "
            "__graft_entry__.build().")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def entropy_words(entropy):
    """numpy's SeedSequence coercion of a sequence of ints to uint32 words
    (bit_generator.pyx _coerce_to_uint32_array)."""
    out = []
    for n in np.atleast_1d(entropy).tolist():
        n = int(n)
        if n < 0:
            raise ValueError("entropy must be non-negative")
        if n == 0:
            out.append(0)
        while n > 0:
            out.append(n & 0xFFFFFFFF)
            n >>= 32
    return np.array(out, dtype=np.uint32)


def pcg_state_words(bitgen):
    """(4,) uint64 {state_hi, state_lo, inc_hi, inc_lo} of a numpy PCG64."""
    st = bitgen.state
    if st["bit_generator"] != "PCG64":
        raise TypeError("only numpy PCG64 streams are supported")
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = (1 << 64) - 1
    return np.array([s >> 64, s & m, inc >> 64, inc & m], dtype=np.uint64)


def pcg_state6(bitgen):
    """(6,) uint64: pcg_state_words + {has_uint32, uinteger} (the buffered half
    of numpy's 32-bit draws, which Generator.integers(n) consumes)."""
    st = bitgen.state
    return np.concatenate([pcg_state_words(bitgen),
                           np.array([st["has_uint32"], st["uinteger"]],
                                    dtype=np.uint64)])


def set_pcg_state6(bitgen, words):
    st = bitgen.state
    w = [int(x) for x in words]
    st["state"]["state"] = (w[0] << 64) | w[1]
    st["state"]["inc"] = (w[2] << 64) | w[3]
    st["has_uint32"] = w[4]
    st["uinteger"] = w[5]
    bitgen.state = st


def set_pcg_state_words(bitgen, words):
    """Write a device-advanced state back into a numpy PCG64 (keeps the
    buffered uint32 half exactly as numpy would: see SURVEY.md appendix A)."""
    st = bitgen.state
    w = [int(x) for x in words]
    st["state"]["state"] = (w[0] << 64) | w[1]
    st["state"]["inc"] = (w[2] << 64) | w[3]
    bitgen.state = st


def enlarge_bootstrap_defaults(sample, enlarge, bootstrap):
    """(enlarge, bootstrap) of a run as the reference's _get_enlarge_bootstrap
    decides them (dynesty.py:169-200)."""
    if enlarge is not None and bootstrap is None:
        if enlarge < 1:
            raise ValueError("enlarge must be >= 1")
        return float(enlarge), 0
    if enlarge is None and bootstrap is not None:
        if not (bootstrap > 1 or bootstrap == 0):
            raise ValueError("bootstrap must be 0 or > 1")
        return 1.0, int(bootstrap)
    if enlarge is None and bootstrap is None:
        return (1.0, 5) if sample == 'unif' else (1.25, 0)
    if bootstrap == 0 or enlarge == 1:
        return float(enlarge), int(bootstrap)
    raise ValueError('Enlarge and bootstrap together do not make sense unless bootstrap=0 or enlarge = 1')


# dh_merged_fetch: field name -> (DH_MERGED_* code, dtype, per-point row of ndim values)
MERGED_FIELDS = dict(logl=(0, np.float64, False), logvol=(1, np.float64, False), logwt=(2, np.float64, False),
                     logz=(3, np.float64, False), logzerr=(4, np.float64, False), information=(5, np.float64, False),
                     weights=(6, np.float64, False), samples_u=(7, np.float64, True), samples=(8, np.float64, True),
                     samples_run=(9, np.int32, False), samples_seq=(10, np.int32, False),
                     samples_n=(11, np.int32, False), final=(12, np.int32, False), samples_id=(13, np.int32, False),
                     samples_it=(14, np.int32, False), ncall=(15, np.int32, False))
# dh_merged_bootstrap_run: result name -> (DH_MERGED_* code, dtype)
BOOT_RUN_FIELDS = dict(idx=(16, np.int64), samples_n=(11, np.int32), logvol=(1, np.float64), logwt=(2, np.float64),
                       logz=(3, np.float64))
MERGED_KLD = 17  # DH_MERGED_KLD: the cumulative divergence (dh_merged_realization, dh_merged_bootstrap_run)
MERGED_BATCH = 18  # DH_MERGED_BATCH: the dynamic batch of every point (dh_merged_fetch); 0 on a run that holds none
# what DeviceMergedRun.field fetches: the fields of the enum and the batch column
FETCH_FIELDS = dict(MERGED_FIELDS, samples_batch=(MERGED_BATCH, np.int32, False))
SUMMARY_FIELDS = ("niter", "logz", "logzerr", "h", "ess", "ncall")


class DeviceMergedRun(dict, Marginals, Errors):
    """The merged run of Context.merge_runs / merge_kept: it lives on the device (one per context, replaced by the
    context's next merge); only what is asked for comes to the host.  `summary`: niter (points), logz, logzerr, h,
    ess, ncall (sum over the points; 0 without per-point bookkeeping).  quantile / histogram / histogram2d /
    corner_data (marginals.Marginals) are computed on the device too: dh_merged_quantile, _hist1d, _hist2d; so are
    logz_realizations / logz_error / jitter_run / realization / reweight (errors.Errors): dh_merged_realize,
    dh_merged_realization; and the strand bootstrap's bootstrap_realizations / resample_run / simulate_run /
    logz_error_sampling / logz_error_total: dh_merged_bootstrap, dh_merged_bootstrap_run (a merge with id / it / nc);
    and kld_realizations / kld_error / weight_function / stopping_function: dh_merged_kld, the KLD field of the two
    per-point calls, dh_merged_weight_function, dh_merged_weights.

    A run that Context.merged_fold folded dynamic batches into carries batch_nlive and batch_bounds (host lists with
    dynamic.merge_batch's conventions: entry 0 is the base run, then one entry per strand) and the per-point field
    samples_batch; both lists are empty on a run that holds no batch.  On such a run the strand bootstrap raises
    ValueError, as ensemble.MergedRun's does; the volume realizations, the weight function, the marginals, the moments
    and the resampling work unchanged."""

    def __init__(self, ctx, summary, ndim, have_pt, batch_nlive=(), batch_bounds=(), prob=None):
        super().__init__()
        self.ctx, self.ndim, self.have_pt = ctx, int(ndim), bool(have_pt)
        self.prob = prob  # the problem the run was merged with (dynamic.fold_batch folds with it)
        self.batch_nlive = [int(x) for x in batch_nlive]
        self.batch_bounds = [(float(lo), float(hi)) for lo, hi in batch_bounds]
        self.summary = dict(zip(SUMMARY_FIELDS, [float(x) for x in summary]))
        self.summary["niter"] = int(self.summary["niter"])
        self.summary["ncall"] = int(self.summary["ncall"])
        self.niter = self.summary["niter"]
        self._serial = ctx._merge_serial

    def _live(self):
        if self.ctx is None or self._serial != self.ctx._merge_serial:
            raise ValueError("this merged run is no longer on the device (released, or replaced by a later merge)")
        return self.ctx

    def field(self, name, first=0, count=None):
        """`count` points of one per-point field from point `first` on (FETCH_FIELDS names)."""
        ctx = self._live()
        if name not in FETCH_FIELDS:
            raise ValueError(f"merged field {name!r}: one of {sorted(FETCH_FIELDS)}")
        code, dtype, row = FETCH_FIELDS[name]
        if 13 <= code <= 15 and not self.have_pt:
            raise ValueError(f"merged field {name!r}: the merge was not given id / it / nc")
        first = int(first)
        count = self.niter - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self.niter:
            raise ValueError(f"merged field {name!r}: [{first}, {first + count}) of {self.niter} points")
        out = np.empty((count, self.ndim) if row else (count,), dtype=dtype)
        ctx._check_merge(ctx.lib.dh_merged_fetch(ctx.handle, code, first, count, _ptr(out)))
        return out

    def mean_and_cov(self):
        """utils.mean_and_cov(samples, importance_weights) computed on the device."""
        ctx = self._live()
        mean, cov = np.empty(self.ndim), np.empty((self.ndim, self.ndim))
        ctx._check_merge(ctx.lib.dh_merged_moments(ctx.handle, _ptr(mean), _ptr(cov)))
        return mean, cov

    def importance_weights(self):
        return self.field("weights")

    def resample_equal(self, n=None, rstate=None):
        """utils.resample_equal(samples, importance_weights, rstate): systematic resampling on the device, the
        shuffle (rstate.permutation) on the host applied to the indices, then a gather of the chosen rows.  With
        n = None (all points) the result equals the reference's row for row."""
        ctx = self._live()
        if rstate is None:
            rstate = np.random.default_rng()
        n = self.niter if n is None else int(n)
        if n < 1:
            raise ValueError("resample_equal: n must be positive")
        idx = np.empty(n, dtype=np.int64)
        ctx._check_merge(ctx.lib.dh_merged_resample(ctx.handle, float(rstate.random()), n, _ptr(idx)))
        return self.gather(idx[rstate.permutation(n)])

    def resample_indices(self, u0, n):
        """idx[i] = #{j : C_j <= (u0 + i) / n} over the normalised cumulative weights (no shuffle)."""
        ctx = self._live()
        idx = np.empty(int(n), dtype=np.int64)
        ctx._check_merge(ctx.lib.dh_merged_resample(ctx.handle, float(u0), int(n), _ptr(idx)))
        return idx

    def gather(self, idx, field="samples"):
        """Rows of the points `idx`: their parameters (field='samples') or their unit-cube rows ('samples_u')."""
        ctx = self._live()
        if field not in ("samples", "samples_u"):
            raise ValueError(f"gather: field {field!r} (one of 'samples', 'samples_u')")
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = np.empty((len(idx), self.ndim))
        if len(idx) and field == "samples":
            ctx._check_merge(ctx.lib.dh_merged_gather(ctx.handle, len(idx), _ptr(idx), _ptr(out)))
        elif len(idx):
            ctx._check_merge(ctx.lib.dh_merged_gather_rows(ctx.handle, MERGED_FIELDS[field][0], len(idx), _ptr(idx),
                                                           _ptr(out)))
        return out

    def batch_seeds(self, logl_min, nlive_new, strands, seed, first=0, want_rows=True, want_keys=False):
        """The start points of `strands` strands of one dynamic batch, chosen on the device (dh_merged_batch_seed;
        seeds.batch_seeds_host is the NumPy mirror, dynamic.batch_seed the Generator's form of the same law): dict(prior,
        idx (strands, nlive_new) or None, keys (with want_keys) or None, logl_min (effective), vol_idx, start, lo, count,
        n_pos, passes) and, with want_rows, seed_u (strands, nlive_new, ndim) and seed_logl (strands, nlive_new): the
        chosen points' unit-cube rows and ln L as Context.ns_batch takes them, gathered on the device (no column and
        no second call crosses for them).  Raises RuntimeError where no point lies above logl_min and ValueError where
        fewer than nlive_new points of positive weight do, as dynamic.batch_seed."""
        return self._live().merged_batch_seed(self, logl_min, nlive_new, strands, seed, first=first, want_rows=want_rows,
                                              want_keys=want_keys)

    def _cols_ptr(self, cols):
        """NULL for all columns in order (the C calls' own default), else the list."""
        return None if np.array_equal(cols, np.arange(self.ndim)) else _ptr(cols)

    def _quantile(self, q, cols):
        ctx = self._live()
        q, cols = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(cols, dtype=np.int32)
        out = np.empty((len(cols), len(q)))
        ctx._check_merge(ctx.lib.dh_merged_quantile(ctx.handle, len(q), _ptr(q), len(cols), self._cols_ptr(cols),
                                                    _ptr(out)))
        return out

    def _hist1d(self, cols, edges, weighted, ranges=None):
        ctx = self._live()
        cols, edges = np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(edges, dtype=np.float64)
        nb = edges.shape[1] - 1
        out = np.empty((len(cols), nb))
        ctx._check_merge(ctx.lib.dh_merged_hist1d(ctx.handle, len(cols), self._cols_ptr(cols), nb, _ptr(edges),
                                                  int(weighted), _ptr(out)))
        return out

    def _hist2d(self, pairs, xedges, yedges, weighted):
        ctx = self._live()
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        xedges, yedges = np.ascontiguousarray(xedges, dtype=np.float64), np.ascontiguousarray(yedges, dtype=np.float64)
        nbx, nby = xedges.shape[1] - 1, yedges.shape[1] - 1
        out = np.empty((len(pairs), nbx, nby))
        ctx._check_merge(ctx.lib.dh_merged_hist2d(ctx.handle, len(pairs), _ptr(pairs), nbx, nby, _ptr(xedges),
                                                  _ptr(yedges), int(weighted), _ptr(out)))
        return out

    def _err_logl(self):
        return self.field("logl")

    @staticmethod
    def _err_seed(seed):
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed: an unsigned 64-bit integer")
        return int(seed)

    def _err_logrwt(self, logrwt):
        if logrwt is None:
            return None
        logrwt = np.ascontiguousarray(logrwt, dtype=np.float64)
        if logrwt.shape != (self.niter,):
            raise ValueError(f"logrwt of shape {logrwt.shape} for {self.niter} points")
        return logrwt

    def _err_realize(self, seed, first, nreal, jitter, logrwt, means):
        ctx = self._live()
        seed, logrwt, nreal = self._err_seed(seed), self._err_logrwt(logrwt), int(nreal)
        if not -(1 << 63) <= int(first) < 1 << 63 or not -(1 << 31) <= nreal < 1 << 31:
            raise ValueError("first / nreal: out of range")
        n = max(nreal, 0)
        lz, h, ess = np.empty(n), np.empty(n), np.empty(n)
        mean = np.empty((n, self.ndim)) if means else None
        ctx._check_merge(ctx.lib.dh_merged_realize(ctx.handle, seed, int(first), nreal, int(jitter), _ptr(logrwt),
                                                   int(means), _ptr(lz), _ptr(h), _ptr(ess), _ptr(mean)))
        return lz, h, ess, mean

    def _err_field(self, seed, real, jitter, logrwt, field, first, count):
        ctx = self._live()
        seed, logrwt = self._err_seed(seed), self._err_logrwt(logrwt)
        if field not in REAL_FIELDS:
            raise ValueError(f"field {field!r}: one of {REAL_FIELDS}")
        first = int(first)
        count = self.niter - first if count is None else int(count)
        if not -(1 << 63) <= int(real) < 1 << 63 or first < 0 or count < 0 or first + count > self.niter:
            raise ValueError(f"realization {real}: [{first}, {first + count}) of {self.niter} points")
        out = np.empty(count)
        ctx._check_merge(ctx.lib.dh_merged_realization(ctx.handle, seed, int(real), int(jitter), _ptr(logrwt),
                                                       MERGED_FIELDS[field][0], first, count, _ptr(out)))
        return out

    def _err_mult(self, mult, nboot):
        if not self.have_pt:
            raise ValueError("the strand bootstrap needs the points' bookkeeping: the merge was not given id / it / nc")
        if mult is None:
            return None
        mult = np.ascontiguousarray(mult)
        if mult.ndim != 1 or mult.dtype.kind not in "iu" or len(mult) != int(self.field("samples_n", 0, 1)[0]):
            raise ValueError("mult: one integer per strand (run * nlive + slot)")
        if int(nboot) != 1:
            raise ValueError("mult: given multiplicities are one bootstrap (nboot = 1)")
        if (mult < 0).any() or (mult >= 1 << 31).any():
            raise ValueError("mult: multiplicities are non-negative 32-bit integers")
        return mult.astype(np.int32)

    def _err_bootstrap(self, seed, first, nboot, jitter, mult, means):
        ctx = self._live()
        seed, nboot, mult = self._err_seed(seed), int(nboot), self._err_mult(mult, nboot)
        if not 1 <= nboot <= MAX_BOOT or not 0 <= int(first) < (1 << 63) - nboot:
            raise ValueError(f"nboot {nboot} outside [1, {MAX_BOOT}], or first {first} not a bootstrap index")
        lz, h, ess, npts = np.empty(nboot), np.empty(nboot), np.empty(nboot), np.empty(nboot, dtype=np.int64)
        mean = np.empty((nboot, self.ndim)) if means else None
        ctx._check_merge(ctx.lib.dh_merged_bootstrap(ctx.handle, seed, int(first), nboot, int(jitter), _ptr(mult),
                                                     int(means), _ptr(lz), _ptr(h), _ptr(ess), _ptr(mean), _ptr(npts)))
        return lz, h, ess, mean, npts

    def _err_bootstrap_run(self, seed, boot, jitter, mult):
        ctx = self._live()
        seed, mult = self._err_seed(seed), self._err_mult(mult, 1)
        if not 0 <= int(boot) < (1 << 63) - 1:
            raise ValueError("boot: a non-negative bootstrap index")
        npts = np.zeros(1, dtype=np.int64)
        out = {}
        for k, (code, dtype) in BOOT_RUN_FIELDS.items():  # (the first call sizes the fetches)
            if not out:
                ctx._check_merge(ctx.lib.dh_merged_bootstrap_run(ctx.handle, seed, int(boot), int(jitter), _ptr(mult), code,
                                                                 0, 0, None, _ptr(npts)))
            out[k] = np.empty(int(npts[0]), dtype=dtype)
            ctx._check_merge(ctx.lib.dh_merged_bootstrap_run(ctx.handle, seed, int(boot), int(jitter), _ptr(mult), code,
                                                             0, int(npts[0]), _ptr(out[k]), None))
        return out

    def _err_kld(self, seed, first, n, mode, mult):
        ctx = self._live()
        seed, n = self._err_seed(seed), int(n)
        mult = self._err_mult(mult, n) if mode else None
        if not 1 <= n <= MAX_BOOT or not 0 <= int(first) < (1 << 63) - n:
            raise ValueError(f"n {n} outside [1, {MAX_BOOT}], or first {first} not an index")
        kld, lz, npts = np.empty(n), np.empty(n), np.empty(n, dtype=np.int64)
        ctx._check_merge(ctx.lib.dh_merged_kld(ctx.handle, seed, int(first), n, int(mode), _ptr(mult), _ptr(kld), _ptr(lz),
                                               _ptr(npts)))
        return kld, lz, npts

    def _err_kld_run(self, seed, index, mode, mult, first, count):
        ctx = self._live()
        seed, first = self._err_seed(seed), int(first)
        if not 0 <= int(index) < (1 << 63) - 1 or first < 0 or (count is not None and int(count) < 0):
            raise ValueError(f"index {index}, first {first}, count {count}: non-negative")
        if mode == 0:
            count = self.niter - first if count is None else int(count)
            if first + count > self.niter:
                raise ValueError(f"[{first}, {first + count}) of {self.niter} points")
            out = np.empty(count)
            ctx._check_merge(ctx.lib.dh_merged_realization(ctx.handle, seed, int(index), 1, None, MERGED_KLD, first, count,
                                                           _ptr(out)))
            return out
        mult = self._err_mult(mult, 1)
        npts = np.zeros(1, dtype=np.int64)
        if count is None:  # (a call without a slice sizes the fetch)
            ctx._check_merge(ctx.lib.dh_merged_bootstrap_run(ctx.handle, seed, int(index), int(mode == 2), _ptr(mult),
                                                             MERGED_KLD, 0, 0, None, _ptr(npts)))
            count = int(npts[0]) - first
            if count < 0:
                raise ValueError(f"first {first} beyond the {int(npts[0])} points of this bootstrap")
        out = np.empty(int(count))
        ctx._check_merge(ctx.lib.dh_merged_bootstrap_run(ctx.handle, seed, int(index), int(mode == 2), _ptr(mult), MERGED_KLD,
                                                         first, int(count), _ptr(out), None))
        return out

    def weights(self, pfrac=0.8, which="weight", first=0, count=None):
        """`count` points from `first` on of 'pweight', 'zweight' or 'weight' of the weight function (dh_merged_weights)."""
        ctx = self._live()
        names = ("pweight", "zweight", "weight")
        if which not in names:
            raise ValueError(f"which {which!r}: one of {names}")
        first = int(first)
        count = self.niter - first if count is None else int(count)
        if not 0. <= pfrac <= 1. or first < 0 or count < 0 or first + count > self.niter:
            raise ValueError(f"weights: pfrac {pfrac} in [0, 1], [{first}, {first + count}) of {self.niter} points")
        out = np.empty(count)
        ctx._check_merge(ctx.lib.dh_merged_weights(ctx.handle, float(pfrac), names.index(which), first, count, _ptr(out)))
        return out

    def _err_weights(self, pfrac):
        return tuple(self.weights(pfrac, w) for w in ("pweight", "zweight", "weight"))

    def _err_weight_function(self, pfrac, maxfrac, pad):
        ctx = self._live()
        bounds, idx = np.empty(2), np.empty(2, dtype=np.int64)
        rc = ctx.lib.dh_merged_weight_function(ctx.handle, pfrac, maxfrac, int(pad), _ptr(bounds), _ptr(idx))
        if rc == ERR_VALUE:  # (no weight above maxfrac x the largest: the host form's ValueError)
            raise ValueError(ctx.lib.dh_last_error(ctx.handle).decode())
        ctx._check_merge(rc)
        return (float(bounds[0]), float(bounds[1])), (int(idx[0]), int(idx[1]))

    def _err_summary(self):
        return self.summary["logzerr"], self.summary["ess"]

    def to_merged_run(self):
        """Everything downloaded into ensemble.MergedRun (merge_static_runs' field names)."""
        from .ensemble import MergedRun
        names = ["logl", "logvol", "logwt", "logz", "logzerr", "information", "samples_n", "samples_run",
                 "samples_seq", "samples_u", "samples"] + (["samples_id", "samples_it", "ncall"] if self.have_pt else [])
        out = MergedRun(niter=self.niter)
        for k in names:
            a = self.field(k)
            out[k] = a.astype(np.int64) if a.dtype == np.int32 else a
        if self.have_pt:
            out["eff"] = 100. * self.niter / float(out["ncall"].sum())
        if self.batch_nlive:
            out["samples_batch"] = self.field("samples_batch").astype(np.int64)
            out["batch_nlive"], out["batch_bounds"] = list(self.batch_nlive), list(self.batch_bounds)
        return out

    def release(self):
        if self.ctx is not None and self._serial == self.ctx._merge_serial:
            self.ctx._merge_serial += 1
            self.ctx._check(self.ctx.lib.dh_merged_release(self.ctx.handle))
        self.ctx = None


class Context:
    """One device + stream (dh_ctx).  Methods take/return NumPy arrays."""

    def __init__(self, device=0):
        self.lib = load()
        self.handle = self.lib.dh_create(int(device))
        if not self.handle:
            msg = self.lib.dh_last_error(None).decode()
            raise DynHipError(f"dh_create({device}) failed: {msg}")
        self.device = int(device)
        self._problems = {}
        self._merge_serial = 0  # which merge the context's merged run is (DeviceMergedRun)
        self._kept_shape = None  # (runs, nlive, ndim, max_iter) of the kept ensemble: ns_continue's host buffers

    def close(self):
        if getattr(self, "handle", None):
            self.lib.dh_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- errors -------------------------------------------------------------
    def _check(self, rc):
        if rc >= 0:
            return rc
        msg = self.lib.dh_last_error(self.handle).decode()
        if rc == ERR_VALUE:
            raise ValueError(msg)
        if rc in (ERR_CONTAIN, ERR_REGION, ERR_SLICE, ERR_QZERO):
            raise RuntimeError(msg)
        raise DynHipError(f"libdynhip error {rc}: {msg}")

    def _check_merge(self, rc):
        """Argument errors of the merge calls (shapes, no kept ensemble, a released run) are ValueError."""
        if rc == ERR_ARG:
            raise ValueError(self.lib.dh_last_error(self.handle).decode())
        return self._check(rc)

    # -- the combiner on the device (csrc/merge*.hip) --------------------------
    def _merged(self, rc):
        """After a merge call: an argument error touched nothing (an earlier DeviceMergedRun stays valid); anything
        else, success included, replaced or dropped the context's merged run."""
        if rc != ERR_ARG:
            self._merge_serial += 1
        return self._check_merge(rc)

    def merge_runs(self, prob, niter, dead_logl, live_logl, dead_u, live_u, dead_id=None, dead_it=None,
                   dead_nc=None, live_it=None):
        """dh_merge_runs: ensemble.merge_static_runs on the device.  dead_*: (R, >= max niter [, D]) arrays or
        per-run lists, live_*: (R, N [, D]) in slot order; dead_id / dead_it / dead_nc / live_it together or not
        at all.  Returns a DeviceMergedRun."""
        nd = prob.ndim
        niter = np.ascontiguousarray(niter, dtype=np.int64).reshape(-1)
        R = len(niter)
        live_logl = _f64(live_logl)
        if live_logl.ndim != 2 or live_logl.shape[0] != R:
            raise ValueError(f"merge_runs: live_logl of shape {live_logl.shape} for {R} runs")
        N = live_logl.shape[1]
        live_u = _f64(live_u)
        if live_u.shape != (R, N, nd):
            raise ValueError(f"merge_runs: live_u of shape {live_u.shape}, expected {(R, N, nd)}")
        stride = int(niter.max()) if R else 0
        if R and int(niter.min()) < 0:
            raise ValueError("merge_runs: negative niter")

        def rows(a, dtype, tail=()):
            out = np.zeros((R, max(stride, 1)) + tail, dtype=dtype)
            for r in range(R):
                row = np.asarray(a[r])
                if len(row) < niter[r]:
                    raise ValueError(f"merge_runs: run {r} has {len(row)} dead rows for niter {niter[r]}")
                out[r, :niter[r]] = row[:niter[r]]
            return out
        info = [dead_id, dead_it, dead_nc, live_it]
        if any(x is None for x in info) and not all(x is None for x in info):
            raise ValueError("merge_runs: dead_id, dead_it, dead_nc and live_it come together")
        have_pt = dead_id is not None
        dl, du = rows(dead_logl, np.float64), rows(dead_u, np.float64, (nd,))
        pid = rows(dead_id, np.int32) if have_pt else None
        pit = rows(dead_it, np.int32) if have_pt else None
        pnc = rows(dead_nc, np.int32) if have_pt else None
        lit = np.ascontiguousarray(live_it, dtype=np.int32).reshape(R, N) if have_pt else None
        summ = np.empty(6)
        self._merged(self.lib.dh_merge_runs(
            self.handle, self.problem(prob), R, N, nd, max(stride, 1) if stride else 0, _ptr(niter), _ptr(dl),
            _ptr(live_logl), _ptr(du), _ptr(live_u), _ptr(pid), _ptr(pit), _ptr(pnc), _ptr(lit), _ptr(summ)))
        return DeviceMergedRun(self, summ, nd, have_pt, prob=prob)

    def merged_fold(self, base, prob, niter, dead_logl, live_logl, dead_u, live_u, dead_id=None, dead_it=None,
                    dead_nc=None, live_it=None, logl_min=-np.inf, logl_max=np.inf):
        """dh_merged_fold: the strands of one dynamic batch folded into the merged run `base` on the device -- the
        host's dynamic.merge_strands.  The strand arrays are merge_runs' run arrays (R strands of N final live points);
        id / it / nc together, and only where `base` has them.  logl_min = -inf (a batch from the prior) is passed as the
        lowest finite double: every ln L lies above either.  Returns a new DeviceMergedRun; `base` goes stale.  On
        ValueError (shapes, a strand point at or below logl_min, an over-long plateau) `base` stays valid."""
        if not isinstance(base, DeviceMergedRun) or base.ctx is not self:
            raise ValueError("merged_fold: base must be this context's DeviceMergedRun")
        base._live()
        nd = prob.ndim
        niter = np.ascontiguousarray(niter, dtype=np.int64).reshape(-1)
        R = len(niter)
        live_logl = _f64(live_logl)
        if R < 1 or live_logl.ndim != 2 or live_logl.shape[0] != R or live_logl.shape[1] < 1:
            raise ValueError(f"merged_fold: live_logl of shape {live_logl.shape} for {R} strands")
        N = live_logl.shape[1]
        live_u = _f64(live_u)
        if live_u.shape != (R, N, nd):
            raise ValueError(f"merged_fold: live_u of shape {live_u.shape}, expected {(R, N, nd)}")
        if int(niter.min()) < 0:
            raise ValueError("merged_fold: negative niter")
        stride = int(niter.max())

        def rows(a, dtype, tail=()):
            out = np.zeros((R, max(stride, 1)) + tail, dtype=dtype)
            for r in range(R):
                row = np.asarray(a[r])
                if len(row) < niter[r] or row.shape[1:] != tail:
                    raise ValueError(f"merged_fold: strand {r} has dead rows of shape {row.shape} for niter {niter[r]}")
                out[r, :niter[r]] = row[:niter[r]]
            return out
        info = [dead_id, dead_it, dead_nc, live_it]
        if any(x is None for x in info) and not all(x is None for x in info):
            raise ValueError("merged_fold: dead_id, dead_it, dead_nc and live_it come together")
        have_pt = dead_id is not None
        if have_pt != base.have_pt:
            raise ValueError("merged_fold: id / it / nc on one side only")
        lmin, lmax = float(logl_min), float(logl_max)
        if np.isnan(lmin) or lmin == np.inf or not lmax > lmin:
            raise ValueError(f"merged_fold: bounds ({lmin}, {lmax})")
        dl, du = rows(dead_logl, np.float64), rows(dead_u, np.float64, (nd,))
        pid = rows(dead_id, np.int32) if have_pt else None
        pit = rows(dead_it, np.int32) if have_pt else None
        pnc = rows(dead_nc, np.int32) if have_pt else None
        lit = np.ascontiguousarray(live_it, dtype=np.int32).reshape(R, N) if have_pt else None
        b_nlive = list(base.batch_nlive) or [int(base.field("samples_n", 0, 1)[0])]
        b_bounds = list(base.batch_bounds) or [(-np.inf, np.inf)]
        summ = np.empty(6)
        rc = self.lib.dh_merged_fold(
            self.handle, self.problem(prob), R, N, max(stride, 1) if stride else 0, _ptr(niter), _ptr(dl),
            _ptr(live_logl), _ptr(du), _ptr(live_u), _ptr(pid), _ptr(pit), _ptr(pnc), _ptr(lit),
            max(lmin, -sys.float_info.max), lmax, _ptr(summ))
        if rc == 0:
            self._merge_serial += 1  # (every failure leaves the base run in place: the handle stays valid)
        self._check_merge(rc)
        return DeviceMergedRun(self, summ, nd, have_pt, b_nlive + [N] * R, b_bounds + [(lmin, lmax)] * R, prob=prob)

    def merged_batch_seed(self, base, logl_min, nlive_new, strands, seed, first=0, want_rows=True, want_keys=False):
        """dh_merged_batch_seed on the merged run `base` (DeviceMergedRun.batch_seeds documents the result)."""
        if not isinstance(base, DeviceMergedRun) or base.ctx is not self:
            raise ValueError("merged_batch_seed: base must be this context's DeviceMergedRun")
        base._live()
        strands, k = int(strands), int(nlive_new)
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed: an unsigned 64-bit integer")
        ok = 1 <= strands <= 65536 and 1 <= k <= 65535  # (the call refuses the rest: no buffers of a bad shape)
        idx = np.empty((strands, k), dtype=np.int64) if ok else None
        keys = np.empty((strands, k)) if ok and want_keys else None
        seed_u = np.empty((strands, k, base.ndim)) if ok and want_rows else None
        seed_l = np.empty((strands, k)) if ok and want_rows else None
        info = np.zeros(12)
        rc = self.lib.dh_merged_batch_seed(self.handle, int(seed), int(first), strands, k, float(logl_min), _ptr(idx),
                                           _ptr(keys), _ptr(seed_u), _ptr(seed_l), _ptr(info))
        if rc == ERR_VALUE:
            raise RuntimeError(self.lib.dh_last_error(self.handle).decode())
        self._check_merge(rc)
        prior, lo, count, n_pos = bool(info[0]), int(info[1]), int(info[2]), int(info[3])
        out = dict(prior=prior, idx=None, keys=None, logl_min=float(info[4]), vol_idx=int(info[5]),
                   start=None if prior else tuple(float(x) for x in info[6:11]), lo=lo, count=count, n_pos=n_pos,
                   passes=int(info[11]))
        if want_rows:
            out.update(seed_u=None, seed_logl=None)
        if prior and lo == 0 and count == base.niter and n_pos == 0:
            return out  # from the prior: no choice was made
        if n_pos < k:
            raise ValueError(f"batch_seeds: {n_pos} saved points of positive weight above ln L = {out['logl_min']}, "
                             f"nlive_new = {k} are needed (a batch on fewer live points is not supported)")
        out["idx"], out["keys"] = idx, keys
        if want_rows:
            out.update(seed_u=seed_u, seed_logl=seed_l)
        return out

    def merge_kept(self, prob, niter=None):
        """dh_merge_kept: the merged run of the ensemble the last ns_ensemble(keep=True) left on the device."""
        nit = None if niter is None else np.ascontiguousarray(niter, dtype=np.int64)
        summ = np.empty(6)
        self._merged(self.lib.dh_merge_kept(self.handle, self.problem(prob), _ptr(nit), _ptr(summ)))
        return DeviceMergedRun(self, summ, prob.ndim, True, prob=prob)

    def release_kept(self):
        self._check(self.lib.dh_ns_release(self.handle))
        self._kept_shape = None

    def set_rwalk_form(self, form):
        """0 (default) / 2: four lanes per walker + matrix cores (csrc/walkq.hip) wherever that kernel is
        built -- decided by the problem alone, never by the launch size; 1: one walker per lane always
        (csrc/walk.hip)."""
        self._check(self.lib.dh_set_rwalk_form(self.handle, int(form)))

    def set_rwalk_items(self, on=True, budget_bytes=0):
        """Four-lane rwalk: PCG64 item streams from a generator pass ahead of the walk (default) or drawn inside
        the walk kernel; `budget_bytes` > 0 bounds the pass's buffer (larger launches go in chunks of walkers)."""
        self._check(self.lib.dh_set_rwalk_items(self.handle, int(bool(on)), int(budget_bytes)))

    def sync(self):
        self._check(self.lib.dh_sync(self.handle))

    # -- device memory --------------------------------------------------------
    def malloc(self, nbytes):
        p = self.lib.dh_malloc(self.handle, int(nbytes))
        if not p:
            self._check(ERR_NOMEM)
        return p

    def free(self, dptr):
        self._check(self.lib.dh_free(self.handle, dptr))

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        self._check(self.lib.dh_memcpy_h2d(self.handle, p, _ptr(arr),
                                           arr.nbytes))
        return p

    def from_device(self, dptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._check(self.lib.dh_memcpy_d2h(self.handle, _ptr(out), dptr,
                                           out.nbytes))
        return out

    def event(self):
        return self.lib.dh_event_create(self.handle)

    def record(self, ev):
        self._check(self.lib.dh_event_record(self.handle, ev))

    def elapsed_ms(self, ev0, ev1):
        ms = C.c_double(0.0)
        self._check(self.lib.dh_event_elapsed_ms(self.handle, ev0, ev1,
                                                 C.byref(ms)))
        return ms.value

    # -- problems -------------------------------------------------------------
    def problem(self, prob):
        """Upload (once) a dynesty_amd.problems.Problem; returns the handle."""
        key = id(prob)
        if key in self._problems:
            return self._problems[key][0]
        like_id, like_par, prior_id, prior_par = prob.device_spec()
        lp, pp = _f64(like_par), _f64(prior_par)
        h = self._check(self.lib.dh_problem_create_ex(
            self.handle, prob.ndim, like_id, _ptr(lp), lp.size, prior_id,
            _ptr(pp) if pp.size else None, pp.size))
        self._problems[key] = (h, prob)  # keep prob alive: id() stays unique
        return h

    def problem_eval(self, prob, u):
        u = _f64(u).reshape(-1, prob.ndim)
        k = u.shape[0]
        v = np.empty_like(u)
        logl = np.empty(k)
        self._check(self.lib.dh_problem_eval(self.handle, self.problem(prob),
                                             k, _ptr(u), _ptr(v), _ptr(logl)))
        return v, logl

    # -- RNG ------------------------------------------------------------------
    def seed_children(self, entropy, first, k):
        words = entropy_words(entropy)
        out = np.empty((k, 4), dtype=np.uint64)
        self._check(self.lib.dh_seed_children(self.handle, _ptr(words),
                                              words.size, int(first), int(k),
                                              _ptr(out)))
        return out

    def rng_stream(self, state4, n_normal, n_unif):
        st = np.ascontiguousarray(state4, dtype=np.uint64)
        nrm = np.empty(max(n_normal, 1))
        unf = np.empty(max(n_unif, 1))
        out = np.empty(4, dtype=np.uint64)
        self._check(self.lib.dh_rng_stream(self.handle, _ptr(st), n_normal,
                                           n_unif, _ptr(nrm), _ptr(unf),
                                           _ptr(out)))
        return nrm[:n_normal], unf[:n_unif], out

    # -- membership -------------------------------------------------------------
    def contains(self, x, ctrs, ams, mode=0, want_mask=False, want_quad=False):
        x = _f64(x)
        if x.ndim == 1:
            x = x[None, :]
        k, d = x.shape
        ctrs = _f64(ctrs).reshape(-1, d)
        m = ctrs.shape[0]
        ams = _f64(ams).reshape(m, d, d)
        count = np.empty(k, dtype=np.int32)
        nw = (k + 63) // 64
        mask = np.empty((m, nw), dtype=np.uint64) if want_mask else None
        quad = np.empty((k, m)) if want_quad else None
        self._check(self.lib.dh_contains(self.handle, _ptr(x), k, d,
                                         _ptr(ctrs), _ptr(ams), m, mode,
                                         _ptr(count), _ptr(mask), _ptr(quad)))
        return count, mask, quad

    def contains_runs(self, x, wpr, ctrs, ams, nells=None, strict=1, run_mode=None, my_mode=0, bstatus=None,
                      flag=None, first=None):
        """The resident loop's membership test of its start points as one launch (dh_contains_runs, a diagnostic
        entry).  x (runs * wpr, d); ctrs (runs, max_ells, d); ams (runs, max_ells, d, d); nells / run_mode / bstatus
        (runs,) or None.  flag (default zeros) and first (None: not asked for) go up as given; returns the arrays that
        came back, (flag, first)."""
        ctrs = _f64(ctrs)
        runs, max_ells, d = ctrs.shape
        x = _f64(x).reshape(runs * wpr, d)
        ams = _f64(ams).reshape(runs, max_ells, d, d)

        def i32(a):
            return None if a is None else np.array(a, dtype=np.int32).reshape(runs)
        nells, run_mode, bstatus, first = i32(nells), i32(run_mode), i32(bstatus), i32(first)
        flag = np.zeros(runs, dtype=np.int32) if flag is None else i32(flag)
        self._check(self.lib.dh_contains_runs(self.handle, _ptr(x), runs, int(wpr), d, _ptr(ctrs), _ptr(ams),
                                              _ptr(nells), max_ells, int(strict), _ptr(run_mode), int(my_mode),
                                              _ptr(bstatus), _ptr(flag), _ptr(first)))
        return flag, first

    # -- rebuild ------------------------------------------------------------------
    def rebuild(self, points, multi=True, max_ells=None, want_labels=False):
        """MultiEllipsoid.update / Ellipsoid.update (see dh_rebuild).  Returns a
        dict of stacked arrays for the resulting ellipsoids."""
        pts = _f64(points)
        n, d = pts.shape
        if max_ells is None:
            max_ells = max(1, n // (2 * d)) if multi else 1
        nells = C.c_int32(0)
        nnodes = C.c_int32(0)
        ctrs = np.empty((max_ells, d))
        covs = np.empty((max_ells, d, d))
        ams = np.empty((max_ells, d, d))
        axes = np.empty((max_ells, d, d))
        axlens = np.empty((max_ells, d))
        logvols = np.empty(max_ells)
        lop = np.empty(n, dtype=np.int32) if want_labels else None
        self._check(self.lib.dh_rebuild(
            self.handle, _ptr(pts), n, d, 0 if multi else 1, max_ells,
            C.byref(nells), _ptr(ctrs), _ptr(covs), _ptr(ams), _ptr(axes),
            _ptr(axlens), _ptr(logvols), _ptr(lop), C.byref(nnodes)))
        m = nells.value
        return dict(nells=m, ctrs=ctrs[:m].copy(), covs=covs[:m].copy(),
                    ams=ams[:m].copy(), axes=axes[:m].copy(),
                    axlens=axlens[:m].copy(), logvol_ells=logvols[:m].copy(),
                    labels=lop, nnodes=nnodes.value)

    def rebuild_many(self, point_sets, multi=True):
        """One launch for several point sets of different sizes (bootstrap
        replicas): returns a list of rebuild() dicts."""
        sets = [_f64(p) for p in point_sets]
        B = len(sets)
        d = sets[0].shape[1]
        if d > 44:  # wide-D path: one rebuild per set (the ragged batch is a narrow-D kernel)
            return [self.rebuild(p, multi=multi) for p in sets]
        n_arr = np.array([len(p) for p in sets], dtype=np.int32)
        n_max = int(n_arr.max())
        pad = np.zeros((B, n_max, d))
        for i, p in enumerate(sets):
            pad[i, :len(p)] = p
        me = max(1, n_max // (2 * d)) if multi else 1
        d_pts = self.to_device(pad)
        d_n = self.to_device(n_arr)
        sizes = dict(nells=B * 4, status=B * 4, ctrs=B * me * d * 8,
                     covs=B * me * d * d * 8, ams=B * me * d * d * 8,
                     axes=B * me * d * d * 8, axl=B * me * d * 8, lv=B * me * 8)
        buf = {k: self.malloc(v) for k, v in sizes.items()}
        try:
            self._check(self.lib.dh_rebuild_ragged_dev(
                self.handle, B, d_pts, n_max, d_n, d, 0 if multi else 1, me,
                buf["nells"], buf["status"], buf["ctrs"], buf["covs"],
                buf["ams"], buf["axes"], buf["axl"], buf["lv"]))
            nells = self.from_device(buf["nells"], (B,), np.int32)
            status = self.from_device(buf["status"], (B,), np.int32)
            ctrs = self.from_device(buf["ctrs"], (B, me, d), np.float64)
            covs = self.from_device(buf["covs"], (B, me, d, d), np.float64)
            ams = self.from_device(buf["ams"], (B, me, d, d), np.float64)
            axes = self.from_device(buf["axes"], (B, me, d, d), np.float64)
            axl = self.from_device(buf["axl"], (B, me, d), np.float64)
            lv = self.from_device(buf["lv"], (B, me), np.float64)
        finally:
            for p in list(buf.values()) + [d_pts, d_n]:
                self.free(p)
        out = []
        for i in range(B):
            if status[i] != 0:
                self.lib.dh_last_error(self.handle)
                raise RuntimeError(f"bootstrap replica {i}: rebuild failed "
                                   f"with code {int(status[i])}")
            m = int(nells[i])
            out.append(dict(nells=m, ctrs=ctrs[i, :m], covs=covs[i, :m],
                            ams=ams[i, :m], axes=axes[i, :m],
                            axlens=axl[i, :m], logvol_ells=lv[i, :m]))
        return out

    def ell_from_cov(self, covs):
        """Ellipsoid.__init__ numerics for a stack of covariances."""
        covs = _f64(covs)
        if covs.ndim == 2:
            covs = covs[None]
        m, d, _ = covs.shape
        axes = np.empty((m, d, d))
        axlens = np.empty((m, d))
        ams = np.empty((m, d, d))
        lvs = np.empty(m)
        self._check(self.lib.dh_ell_from_cov(self.handle, m, d, _ptr(covs),
                                             _ptr(axes), _ptr(axlens),
                                             _ptr(ams), _ptr(lvs)))
        return axes, axlens, ams, lvs

    def improve_covar_mat(self, covs):
        """improve_covar_mat (bounding.py:1311-1384) for a stack of matrices:
        returns (good (m,) bool, cov, am, axes)."""
        covs = _f64(covs)
        if covs.ndim == 2:
            covs = covs[None]
        m, d, _ = covs.shape
        good = np.empty(m, dtype=np.int32)
        out = np.empty((m, d, d)); am = np.empty((m, d, d)); axes = np.empty((m, d, d))
        self._check(self.lib.dh_improve_covar_mat(self.handle, m, d, _ptr(covs), _ptr(good),
                                                  _ptr(out), _ptr(am), _ptr(axes)))
        return good.astype(bool), out, am, axes

    def scale_to_logvol(self, covs, ams, axes, axlens, logvols, targets):
        """In-place Ellipsoid.scale_to_logvol for a stack of ellipsoids; the
        arrays must be C-contiguous float64 (they are updated in place)."""
        m, d = axlens.shape
        for a in (covs, ams, axes, axlens, logvols):
            assert a.flags.c_contiguous and a.dtype == np.float64
        t = _f64(targets).reshape(m)
        self._check(self.lib.dh_scale_to_logvol(
            self.handle, m, d, _ptr(covs), _ptr(ams), _ptr(axes), _ptr(axlens),
            _ptr(logvols), _ptr(t)))

    def enlarge_runs(self, covs, ams, axes, axlens, logvols, nells, log_enlarge, active=None, run_shift=None):
        """The resident loop's enlarge launch as one launch (dh_enlarge_runs, a diagnostic entry), in place on
        covs / ams / axes (runs, max_ells, d, d), axlens (runs, max_ells, d) and logvols (runs, max_ells), which must
        be C-contiguous float64.  nells (runs,); active (runs,) int and run_shift (runs,) float or None."""
        runs, max_ells, d = axlens.shape
        for a in (covs, ams, axes, axlens, logvols):
            assert a.flags.c_contiguous and a.dtype == np.float64
        nells = np.array(nells, dtype=np.int32).reshape(runs)
        active = None if active is None else np.array(active, dtype=np.int32).reshape(runs)
        run_shift = None if run_shift is None else _f64(run_shift).reshape(runs)
        self._check(self.lib.dh_enlarge_runs(self.handle, runs, max_ells, _ptr(nells), d, _ptr(covs), _ptr(ams),
                                             _ptr(axes), _ptr(axlens), _ptr(logvols), float(log_enlarge),
                                             _ptr(active), _ptr(run_shift)))

    # -- proposals ----------------------------------------------------------------
    def rwalk_batch(self, prob, u0, axes, scale, loglstar, walks, rng_states,
                    axes_idx=None, ncdim=None, bc=None):
        """Batched RWalkSampler.sample (see dh_rwalk_batch)."""
        ndim = prob.ndim
        u0 = _f64(u0).reshape(-1, ndim)
        k = u0.shape[0]
        ncdim = ndim if ncdim is None else int(ncdim)
        axes = _f64(axes).reshape(-1, ncdim, ncdim)
        m = axes.shape[0]
        idx = None if axes_idx is None else np.ascontiguousarray(
            axes_idx, dtype=np.int32)
        bcarr = None if bc is None else np.ascontiguousarray(bc, dtype=np.int8)
        rng = np.ascontiguousarray(rng_states, dtype=np.uint64).reshape(k, 4)
        u = np.empty((k, ndim))
        v = np.empty((k, ndim))
        logl = np.empty(k)
        nacc = np.empty(k, dtype=np.int32)
        nrej = np.empty(k, dtype=np.int32)
        rng_out = np.empty((k, 4), dtype=np.uint64)
        self._check(self.lib.dh_rwalk_batch(
            self.handle, self.problem(prob), k, ndim, ncdim, _ptr(u0),
            _ptr(axes), m, _ptr(idx), float(scale), float(loglstar),
            int(walks), _ptr(bcarr), _ptr(rng), _ptr(u), _ptr(v), _ptr(logl),
            _ptr(nacc), _ptr(nrej), _ptr(rng_out)))
        return dict(u=u, v=v, logl=logl, accept=nacc, reject=nrej,
                    rng_out=rng_out)


    def rwalk_batch_philox(self, prob, u0, axes, scale, loglstar, walks, seed,
                           sequence0=0, offset=0, axes_idx=None, ncdim=None, bc=None):
        """Throughput mode of the batched RWalkSampler.sample (dh_rwalk_batch_philox):
        hiprand Philox4x32-10 keyed (seed, sequence0 + walker, offset)."""
        ndim = prob.ndim
        u0 = _f64(u0).reshape(-1, ndim)
        k = u0.shape[0]
        ncdim = ndim if ncdim is None else int(ncdim)
        axes = _f64(axes).reshape(-1, ncdim, ncdim)
        idx = None if axes_idx is None else np.ascontiguousarray(axes_idx, dtype=np.int32)
        bcarr = None if bc is None else np.ascontiguousarray(bc, dtype=np.int8)
        u = np.empty((k, ndim)); v = np.empty((k, ndim)); logl = np.empty(k)
        nacc = np.empty(k, dtype=np.int32); nrej = np.empty(k, dtype=np.int32)
        self._check(self.lib.dh_rwalk_batch_philox(
            self.handle, self.problem(prob), k, ndim, ncdim, _ptr(u0), _ptr(axes), axes.shape[0],
            _ptr(idx), float(scale), float(loglstar), int(walks), _ptr(bcarr), int(seed),
            int(sequence0), int(offset), _ptr(u), _ptr(v), _ptr(logl), _ptr(nacc), _ptr(nrej)))
        return dict(u=u, v=v, logl=logl, accept=nacc, reject=nrej)

    def rwalk_propose(self, u0, axes, scale, rng_states, axes_idx=None,
                      ncdim=None, bc=None):
        """One propose_ball_point per walker (dh_rwalk_propose)."""
        u0 = _f64(u0)
        k, ndim = u0.shape
        ncdim = ndim if ncdim is None else int(ncdim)
        axes = _f64(axes).reshape(-1, ncdim, ncdim)
        idx = None if axes_idx is None else np.ascontiguousarray(
            axes_idx, dtype=np.int32)
        bcarr = None if bc is None else np.ascontiguousarray(bc, dtype=np.int8)
        rng = np.ascontiguousarray(rng_states, dtype=np.uint64).reshape(k, 4)
        up = np.empty((k, ndim))
        inside = np.empty(k, dtype=np.int32)
        rng_out = np.empty((k, 4), dtype=np.uint64)
        self._check(self.lib.dh_rwalk_propose(
            self.handle, k, ndim, ncdim, _ptr(u0), _ptr(axes), axes.shape[0],
            _ptr(idx), float(scale), _ptr(bcarr), _ptr(rng), _ptr(up),
            _ptr(inside), _ptr(rng_out)))
        return up, inside.astype(bool), rng_out

    def slice_feed(self, kind, ndim, states6, consumed=None, nlook=0, axes=None,
                   axes_idx=None, scale=1.0):
        """Direction / axis order + uncommitted uniform lookahead of every
        walker's stream for one slice (dh_slice_feed).  kind: 'direction'
        (rslice), 'shuffle' (slice) or 'advance'.  Returns
        (states6, dirs | perm | None, look)."""
        kd = {'direction': 0, 'shuffle': 1, 'advance': 2}[kind]
        st = np.array(states6, dtype=np.uint64).reshape(-1, 6)
        k = st.shape[0]
        cons = None if consumed is None else np.ascontiguousarray(
            consumed, dtype=np.int32)
        ax = idx = dirs = perm = None
        m = 0
        if kd == 0:
            ax = _f64(axes).reshape(-1, ndim, ndim)
            m = ax.shape[0]
            idx = None if axes_idx is None else np.ascontiguousarray(
                axes_idx, dtype=np.int32)
            dirs = np.empty((k, ndim))
        elif kd == 1:
            perm = np.empty((k, ndim), dtype=np.int32)
        look = np.empty((k, int(nlook)))
        self._check(self.lib.dh_slice_feed(
            self.handle, k, int(ndim), kd, _ptr(ax), m, _ptr(idx), float(scale),
            _ptr(st), _ptr(cons), int(nlook), _ptr(dirs), _ptr(perm),
            _ptr(look) if nlook else None))
        return st, (dirs if kd == 0 else perm), look

    def slice_batch(self, prob, u0, axes, scale, loglstar, slices, rng_states,
                    principal=False, doubling=False, axes_idx=None):
        """Batched RSliceSampler.sample / SliceSampler.sample (dh_slice_batch)."""
        ndim = prob.ndim
        u0 = _f64(u0).reshape(-1, ndim)
        k = u0.shape[0]
        axes = _f64(axes).reshape(-1, ndim, ndim)
        idx = None if axes_idx is None else np.ascontiguousarray(
            axes_idx, dtype=np.int32)
        rng = np.ascontiguousarray(rng_states, dtype=np.uint64).reshape(k, 4)
        u = np.empty((k, ndim))
        v = np.empty((k, ndim))
        logl = np.empty(k)
        nc = np.empty(k, dtype=np.int32)
        ne = np.empty(k, dtype=np.int32)
        nt = np.empty(k, dtype=np.int32)
        fl = np.empty(k, dtype=np.int32)
        rng_out = np.empty((k, 4), dtype=np.uint64)
        self._check(self.lib.dh_slice_batch(
            self.handle, self.problem(prob), k, ndim, 1 if principal else 0,
            _ptr(u0), _ptr(axes), axes.shape[0], _ptr(idx), float(scale),
            float(loglstar), int(slices), 1 if doubling else 0, _ptr(rng),
            _ptr(u), _ptr(v), _ptr(logl), _ptr(nc), _ptr(ne), _ptr(nt),
            _ptr(fl), _ptr(rng_out)))
        return dict(u=u, v=v, logl=logl, ncalls=nc, n_expand=ne, n_contract=nt,
                    expansion_warning_set=(fl & 1).astype(bool),
                    rng_out=rng_out)

    def slice_batch_philox(self, prob, u0, axes, scale, loglstar, slices, seed, sequence0=0, offset=0,
                           axes_idx=None, principal=False, doubling=False):
        """Throughput mode of the batched slice samplers (dh_slice_batch_philox): hiprand
        Philox4x32-10 keyed (seed, sequence0 + walker, offset)."""
        ndim = prob.ndim
        u0 = _f64(u0).reshape(-1, ndim)
        k = u0.shape[0]
        axes = _f64(axes).reshape(-1, ndim, ndim)
        idx = None if axes_idx is None else np.ascontiguousarray(axes_idx, dtype=np.int32)
        u = np.empty((k, ndim)); v = np.empty((k, ndim)); logl = np.empty(k)
        nc = np.empty(k, dtype=np.int32); ne = np.empty(k, dtype=np.int32)
        nt = np.empty(k, dtype=np.int32); fl = np.empty(k, dtype=np.int32)
        self._check(self.lib.dh_slice_batch_philox(
            self.handle, self.problem(prob), k, ndim, 1 if principal else 0, _ptr(u0), _ptr(axes),
            axes.shape[0], _ptr(idx), float(scale), float(loglstar), int(slices), 1 if doubling else 0,
            int(seed), int(sequence0), int(offset), _ptr(u), _ptr(v), _ptr(logl), _ptr(nc), _ptr(ne),
            _ptr(nt), _ptr(fl)))
        return dict(u=u, v=v, logl=logl, ncalls=nc, n_expand=ne, n_contract=nt,
                    expansion_warning_set=(fl & 1).astype(bool))

    def unif_batch_philox(self, prob, loglstar, k, seed, sequence0=0, offset=0, ctrs=None, axes=None,
                          ams=None, logvol_ells=None, ncdim=None, bc=None, max_tries=0):
        """Throughput mode of the batched UniformBoundSampler.sample / UnitCubeSampler.sample
        (dh_unif_batch_philox) for k walkers."""
        ndim = prob.ndim
        ncdim = ndim if ncdim is None else int(ncdim)
        if ctrs is None:
            m, c, ax, am, cp = 0, None, None, None, None
        else:
            c = _f64(ctrs).reshape(-1, ncdim)
            m = c.shape[0]
            ax = _f64(axes).reshape(m, ncdim, ncdim)
            am = cp = None
            if m > 1:
                am = _f64(ams).reshape(m, ncdim, ncdim)
                cp = cumprob_of(logvol_ells)
        bcarr = None if bc is None else np.ascontiguousarray(bc, dtype=np.int8)
        u = np.empty((k, ndim)); v = np.empty((k, ndim)); logl = np.empty(k)
        nc = np.empty(k, dtype=np.int32)
        self._check(self.lib.dh_unif_batch_philox(
            self.handle, self.problem(prob), int(k), ndim, ncdim, m, _ptr(c), _ptr(ax), _ptr(am), _ptr(cp),
            float(loglstar), _ptr(bcarr), int(seed), int(sequence0), int(offset), int(max_tries),
            _ptr(u), _ptr(v), _ptr(logl), _ptr(nc)))
        return dict(u=u, v=v, logl=logl, ncalls=nc)

    def unif_batch(self, prob, loglstar, rng_states, ctrs=None, axes=None,
                   ams=None, logvol_ells=None, ncdim=None, bc=None,
                   max_tries=0):
        """Batched UniformBoundSampler.sample (ellipsoid bound given by
        ctrs/axes[/ams/logvol_ells]) or UnitCubeSampler.sample (ctrs=None)."""
        ndim = prob.ndim
        rng = np.ascontiguousarray(rng_states, dtype=np.uint64).reshape(-1, 4)
        k = rng.shape[0]
        ncdim = ndim if ncdim is None else int(ncdim)
        if ctrs is None:
            m, c, ax, am, cp = 0, None, None, None, None
        else:
            c = _f64(ctrs).reshape(-1, ncdim)
            m = c.shape[0]
            ax = _f64(axes).reshape(m, ncdim, ncdim)
            am = cp = None
            if m > 1:
                am = _f64(ams).reshape(m, ncdim, ncdim)
                cp = cumprob_of(logvol_ells)
        bcarr = None if bc is None else np.ascontiguousarray(bc, dtype=np.int8)
        u = np.empty((k, ndim))
        v = np.empty((k, ndim))
        logl = np.empty(k)
        nc = np.empty(k, dtype=np.int32)
        rng_out = np.empty((k, 4), dtype=np.uint64)
        self._check(self.lib.dh_unif_batch(
            self.handle, self.problem(prob), k, ndim, ncdim, m, _ptr(c),
            _ptr(ax), _ptr(am), _ptr(cp), float(loglstar), _ptr(bcarr),
            _ptr(rng), int(max_tries), _ptr(u), _ptr(v), _ptr(logl), _ptr(nc),
            _ptr(rng_out)))
        return dict(u=u, v=v, logl=logl, ncalls=nc, rng_out=rng_out)

    def unif_propose(self, ndim, rng_states, ctrs=None, axes=None, ams=None,
                     logvol_ells=None, ncdim=None, bc=None, friends=None):
        """Lock-step half of UniformBoundSampler for an arbitrary host
        likelihood: per walker the next candidate of its stream that lies in
        the bound and passes unitcheck (dh_unif_batch / dh_unif_friends_batch
        with problem = -1).  friends = (kind, ctrs, axes, axes_inv) selects a
        balls / cubes bound; rng_states then has 6 columns (the last two carry
        NumPy's buffered 32-bit half, which integers(n) consumes) and so has
        the returned state.  Returns (u (k, ndim), rng_out)."""
        rs = np.ascontiguousarray(rng_states, dtype=np.uint64)
        rs = rs.reshape(-1, 6 if friends is not None else 4)
        rng = np.ascontiguousarray(rs[:, :4])
        k = rng.shape[0]
        ncdim = ndim if ncdim is None else int(ncdim)
        bcarr = None if bc is None else np.ascontiguousarray(bc, dtype=np.int8)
        u = np.empty((k, ndim))
        rng_out = np.empty((k, 4), dtype=np.uint64)
        if friends is not None:
            kind, fc, fax, fai = friends
            c = _f64(fc).reshape(-1, ndim)
            r32 = np.ascontiguousarray(rs[:, 4:])
            r32o = np.empty((k, 2), dtype=np.uint64)
            self._check(self.lib.dh_unif_friends_batch(
                self.handle, -1, k, ndim, 0 if kind == 'balls' else 1, _ptr(c),
                c.shape[0], _ptr(_f64(fax)), _ptr(_f64(fai)), 0.0, _ptr(bcarr),
                _ptr(rng), 0, _ptr(u), None, None, None, _ptr(rng_out),
                _ptr(r32), _ptr(r32o)))
            return u, np.concatenate([rng_out, r32o], axis=1)
        if ctrs is None:
            m, c, ax, am, cp = 0, None, None, None, None
        else:
            c = _f64(ctrs).reshape(-1, ncdim)
            m = c.shape[0]
            ax = _f64(axes).reshape(m, ncdim, ncdim)
            am = cp = None
            if m > 1:
                am = _f64(ams).reshape(m, ncdim, ncdim)
                cp = cumprob_of(logvol_ells)
        self._check(self.lib.dh_unif_batch(
            self.handle, -1, k, ndim, ncdim, m, _ptr(c), _ptr(ax), _ptr(am),
            _ptr(cp), 0.0, _ptr(bcarr), _ptr(rng), 0, _ptr(u), None, None,
            None, _ptr(rng_out)))
        return u, rng_out

    def unif_friends_batch(self, prob, loglstar, rng_states, ctrs, kind, axes,
                           axes_inv, bc=None, max_tries=0):
        """Batched UniformBoundSampler.sample inside a RadFriends ('balls') /
        SupFriends ('cubes') bound (dh_unif_friends_batch)."""
        ndim = prob.ndim
        rng = np.ascontiguousarray(rng_states, dtype=np.uint64).reshape(-1, 4)
        k = rng.shape[0]
        c = _f64(ctrs).reshape(-1, ndim)
        bcarr = None if bc is None else np.ascontiguousarray(bc, dtype=np.int8)
        u = np.empty((k, ndim))
        v = np.empty((k, ndim))
        logl = np.empty(k)
        nc = np.empty(k, dtype=np.int32)
        rng_out = np.empty((k, 4), dtype=np.uint64)
        self._check(self.lib.dh_unif_friends_batch(
            self.handle, self.problem(prob), k, ndim,
            0 if kind == 'balls' else 1, _ptr(c), c.shape[0],
            _ptr(_f64(axes)), _ptr(_f64(axes_inv)), float(loglstar),
            _ptr(bcarr), _ptr(rng), int(max_tries), _ptr(u), _ptr(v),
            _ptr(logl), _ptr(nc), _ptr(rng_out), None, None))
        return dict(u=u, v=v, logl=logl, ncalls=nc, rng_out=rng_out)

    def ns_consume(self, live_logl, q_logl, q_ncalls, state, dlogz, live_it=None, plateau=None):
        """One queue consumption per run (dh_ns_consume).  live_logl (R, N) and
        state (R, 8) are updated in place; returns dict(dead_logl, dead_slot,
        dead_src (lists per run), stopped (R,) bool).  With live_it ((R, N) int32,
        updated in place: iteration at which each live point was proposed) also
        dead_it / dead_nc per run (the reference's per-point 'it' and 'nc').
        plateau: optional (R, 2) float64, updated in place -- the reference's
        likelihood-plateau mode carried between calls (deaths left, ln of the
        plateau's volume step; sampler.py:1112-1127)."""
        live = np.ascontiguousarray(live_logl, dtype=np.float64)
        assert live is live_logl and live.ndim == 2
        R, N = live.shape
        ql = _f64(q_logl).reshape(R, -1)
        K = ql.shape[1]
        qn = np.ascontiguousarray(q_ncalls, dtype=np.int32).reshape(R, K)
        assert state.dtype == np.float64 and state.shape == (R, 8) and state.flags.c_contiguous
        dl = np.empty((R, K)); ds = np.empty((R, K), dtype=np.int32); dj = np.empty((R, K), dtype=np.int32)
        nd = np.empty(R, dtype=np.int32); stp = np.empty(R, dtype=np.int32)
        dit = dnc = None
        if live_it is not None:
            assert live_it.dtype == np.int32 and live_it.shape == (R, N) and live_it.flags.c_contiguous
            dit = np.empty((R, K), dtype=np.int32)
            dnc = np.empty((R, K), dtype=np.int32)
        if plateau is not None:
            assert plateau.dtype == np.float64 and plateau.shape == (R, 2) and plateau.flags.c_contiguous
        self._check(self.lib.dh_ns_consume(self.handle, R, N, K, float(dlogz), _ptr(live), _ptr(ql),
                                           _ptr(qn), _ptr(state), _ptr(dl), _ptr(ds), _ptr(dj),
                                           _ptr(nd), _ptr(stp), _ptr(live_it), _ptr(dit), _ptr(dnc),
                                           _ptr(plateau)))
        out = dict(dead_logl=[dl[r, :nd[r]].copy() for r in range(R)],
                   dead_slot=[ds[r, :nd[r]].copy() for r in range(R)],
                   dead_src=[dj[r, :nd[r]].copy() for r in range(R)],
                   stopped=stp.astype(bool))
        if live_it is not None:
            out["dead_it"] = [dit[r, :nd[r]].copy() for r in range(R)]
            out["dead_nc"] = [dnc[r, :nd[r]].copy() for r in range(R)]
        return out

    def ns_ensemble(self, prob, runs, nlive, queue_size, walks=None,
                    bound='multi', dlogz=0.01, enlarge=None, entropy=(21,),
                    first_run=0, max_fills=0, max_iter=400000,
                    want_dead_logl=False, sample='rwalk', slices=None,
                    rebuild_sync=False, want_samples=False, rng='pcg64', bootstrap=None, rebuild_every=0,
                    update_interval=None, first_update=None, maxiter=None, maxcall=None, logl_max=None,
                    add_live=True, forced_exact=True, periodic=None, reflective=None, keep=False):
        """Device-resident ensemble of static NS runs (dh_ns_ensemble).

        keep=True: the finished ensemble stays on the device for merge_kept (dh_ns_keep); with want_samples=False
        the returned dict then has the records and no per-point arrays.

        periodic / reflective: lists of coordinate indices as NestedSampler takes them (dynesty.py:297-310); they reach
        the rwalk and uniform samplers (dh_ns_set_boundary), the slice samplers ignore them as the reference's do.

        forced_exact=True (the default): the reference's protocol -- propose_live's forced bound update
        (sampler.py:484-489) belongs to the fill that finds a start point outside the bound, and the regular bound is
        built before the newest point enters (DH_NS_OPT_FORCED_EXACT).  False: the late form (the run is flagged and
        rebuilds before its next fill): 9-20 % fewer bound updates than the reference, a few per cent faster.

        update_interval / first_update (NestedSampler, dynesty.py:213-234: a float update_interval is a multiple of
        nlive, an int a number of calls; first_update = dict(min_ncall=..., min_eff=...)) and maxiter / maxcall /
        logl_max / add_live (run_nested, sampler.py:1214-1300) as the reference takes them; None = its default.

        rebuild_every=n: bounds are built every n-th fill and runs that become due in
        between wait -- per-run results unchanged (bit-identical with PCG64 streams),
        fewer and fuller rebuild fills; 0 = chosen from the run's shape.

        sample: 'rwalk' | 'rslice' | 'slice' | 'unif'.  enlarge / bootstrap default as the reference's
        _get_enlarge_bootstrap (dynesty.py:169-200): (1.25, 0), and (1, 5) for 'unif'.

        bound: 'multi' | 'single' with every sampler; 'balls' (RadFriends) | 'cubes' (SupFriends) with
        sample='unif', rng='pcg64' and ndim <= 32 only -- the update batched over the due runs on the device, the
        shapes on each run's live points of the fill.  Every other combination raises ValueError.

        rebuild_sync=False keeps the reference's per-run update schedule
        (sampler.py:625-674): a run's result then depends only on its own seed,
        not on how the ensemble is sharded.  rebuild_sync=True lets all runs
        that already have a bound rebuild it together whenever any run is due
        (early, never late): fewer, fuller rebuild launches, but a run's
        schedule then depends on its shard mates."""
        nd = prob.ndim
        if bound not in ('multi', 'single', 'balls', 'cubes'):
            raise ValueError(f"ns_ensemble: bound={bound!r} is not supported by the device-resident "
                             "loop ('multi', 'single', or 'balls' / 'cubes' with sample='unif')")
        if bound in ('balls', 'cubes'):
            if sample != 'unif':
                raise ValueError(f"ns_ensemble: bound={bound!r} with sample={sample!r} is not supported by the "
                                 "device-resident loop (balls / cubes run with sample='unif' only)")
            if rng != 'pcg64':
                raise ValueError(f"ns_ensemble: bound={bound!r} with rng={rng!r} is not supported by the "
                                 "device-resident loop (balls / cubes need rng='pcg64')")
            if nd > 32:
                raise ValueError(f"ns_ensemble: bound={bound!r} at ndim={nd} is not supported by the "
                                 "device-resident loop (balls / cubes need ndim <= 32)")
        kind, walks, enlarge, bootstrap = self._ns_sampler("ns_ensemble", nd, sample, rng, walks, slices, enlarge, bootstrap)
        words = entropy_words(entropy)
        want_dead_logl = want_dead_logl or want_samples
        buf = self._ns_buffers(runs, nlive, nd, max_iter, want_dead_logl, want_samples)
        nf = C.c_int64(0)
        self._ns_arm(nd, nlive, update_interval, first_update, maxiter, maxcall, logl_max, add_live, forced_exact,
                     periodic, reflective)
        if keep:
            self._check(self.lib.dh_ns_keep(self.handle, 1))
        self._check(self.lib.dh_ns_ensemble(
            self.handle, self.problem(prob), int(runs), int(nlive), nd,
            int(queue_size), kind, int(walks),
            BOUND_CODES[bound],
            1 if rebuild_sync else 0, float(dlogz), float(enlarge), int(max_fills), int(max_iter),
            _ptr(words), words.size, int(first_run), _ptr(buf["rec"]), _ptr(buf["dead"]),
            _ptr(buf["livel"]), _ptr(buf["dead_u"]), _ptr(buf["live_u"]), C.byref(nf), _ptr(buf["pid"]), _ptr(buf["pit"]),
            _ptr(buf["pnc"]), _ptr(buf["lit"]), int(bootstrap), int(rebuild_every)))
        if keep:
            self._kept_shape = (int(runs), int(nlive), nd, int(max_iter))
        return self._ns_result(buf, nf, want_dead_logl, want_samples)

    # ---- what dh_ns_ensemble and dh_ns_batch take alike: one place for the argument handling of both ----
    @staticmethod
    def _ns_sampler(what, nd, sample, rng, walks, slices, enlarge, bootstrap):
        """(sampler code, walks or slices, enlarge, bootstrap) of sample / rng with the reference's defaults."""
        if sample not in ('rwalk', 'rslice', 'slice', 'unif'):
            raise ValueError(f"{what}: sample={sample!r} is not supported by the "
                             "device-resident loop ('rwalk', 'rslice', 'slice' or 'unif')")
        kind = dict(rwalk=0, rslice=1, slice=2, unif=6)[sample]
        if rng not in ('pcg64', 'philox'):
            raise ValueError(f"{what}: rng must be 'pcg64' or 'philox'")
        enlarge, bootstrap = enlarge_bootstrap_defaults(sample, enlarge, bootstrap)
        if kind == 6:
            walks = 1  # unused
        elif kind == 0:
            if walks is None:
                walks = nd + 20  # dynesty.py:128
        else:
            walks = slices if slices is not None else \
                (3 + nd if kind == 1 else 3)
        if rng == 'philox':
            kind += 1 if kind == 6 else 3
        return kind, walks, enlarge, bootstrap

    def _ns_arm(self, nd, nlive, update_interval, first_update, maxiter, maxcall, logl_max, add_live, forced_exact,
                periodic, reflective):
        """The one-shot options and boundary flags of the next dh_ns_ensemble / dh_ns_batch call."""
        nan = float('nan')
        if update_interval is not None:
            # dynesty.py:213-234: a float is a multiple of nlive, an int a number of calls
            # (np.floating is not a Python float: an np.float32 ratio used to be truncated by int(); any value is
            # clamped to >= 1 call like the reference's max(min(round(ratio * nlive), maxsize), 1), dynesty.py:646-649)
            if isinstance(update_interval, (int, np.integer)) and not isinstance(update_interval, bool):
                update_interval = max(1, int(update_interval))
            else:
                update_interval = max(1, int(round(float(update_interval) * nlive)))
        fu = first_update or {}
        opts = [nan if update_interval is None else float(update_interval),
                float(fu['min_ncall']) if 'min_ncall' in fu else nan,
                float(fu['min_eff']) if 'min_eff' in fu else nan,
                nan if maxiter is None else float(maxiter), nan if maxcall is None else float(maxcall),
                nan if logl_max is None else float(logl_max), nan if add_live else 0.0,
                1.0 if forced_exact else 0.0]
        for key, val in enumerate(opts):
            self._check(self.lib.dh_ns_set_option(self.handle, key, val))
        bc = None
        if periodic is not None or reflective is not None:
            bc = np.zeros(nd, dtype=np.int8)
            if periodic is not None:
                bc[np.asarray(periodic, dtype=int)] = BC_PERIODIC
            if reflective is not None:
                bc[np.asarray(reflective, dtype=int)] = BC_REFLECT
        self._check(self.lib.dh_ns_set_boundary(self.handle, nd if bc is not None else 0, _ptr(bc)))

    @staticmethod
    def _ns_buffers(runs, nlive, nd, max_iter, want_dead_logl, want_samples):
        """The host arrays a call writes: records always, the rest where asked for (None otherwise)."""
        def maybe(want, shape, dtype=np.float64):
            return np.empty(shape, dtype=dtype) if want else None
        return dict(rec=np.empty((runs, 8)),
                    dead=maybe(want_dead_logl, (runs, max_iter)), livel=maybe(want_dead_logl, (runs, nlive)),
                    # runs x max_iter x ndim: only the niter rows a run produced are touched
                    dead_u=maybe(want_samples, (runs, max_iter, nd)), live_u=maybe(want_samples, (runs, nlive, nd)),
                    # the reference's per-point id / it / nc (sampler.py:1165-1182) travel with the samples
                    pid=maybe(want_samples, (runs, max_iter), np.int32), pit=maybe(want_samples, (runs, max_iter), np.int32),
                    pnc=maybe(want_samples, (runs, max_iter), np.int32), lit=maybe(want_samples, (runs, nlive), np.int32))

    @staticmethod
    def _ns_result(buf, nf, want_dead_logl, want_samples):
        rec = buf["rec"]
        out = dict(logz=rec[:, 0], logzerr=rec[:, 1],
                   niter=rec[:, 2].astype(np.int64),
                   ncall=rec[:, 3].astype(np.int64), h=rec[:, 4],
                   nbound=rec[:, 5].astype(np.int64),
                   status=rec[:, 6].astype(np.int64), eff=rec[:, 7],
                   nfills=nf.value)
        if want_dead_logl:
            out["dead_logl"] = buf["dead"]
            out["live_logl"] = buf["livel"]
        if want_samples:
            out["dead_u"] = buf["dead_u"]
            out["live_u"] = buf["live_u"]
            out["dead_id"], out["dead_it"], out["dead_nc"], out["live_it"] = buf["pid"], buf["pit"], buf["pnc"], buf["lit"]
        return out

    def ns_batch(self, prob, seed_u, seed_logl, logl_min, start, queue_size, logl_max=None, walks=None,
                 bound='multi', dlogz=0.01, enlarge=None, entropy=(21,), first_run=0, max_fills=0, max_iter=400000,
                 sample='rwalk', slices=None, bootstrap=None, rebuild_every=0, update_interval=None, maxiter=None,
                 maxcall=None, add_live=True, forced_exact=True, periodic=None, reflective=None, want_samples=True,
                 rng='pcg64', keep=False):
        """One dynamic batch on the device (dh_ns_batch): `runs` strands of nlive_new live points inside the ln L range
        (logl_min, logl_max] of a finished run.  seed_u (runs, nlive_new, ndim) / seed_logl (runs, nlive_new): every
        strand's seeds, points of the finished run above logl_min (dynamic.batch_seed chooses them); start (runs, 6) or
        (6,): logvol, logz, h, logzvar and ln L of the finished run's row at logl_min, and the scale the strand starts
        with.  Everything else as ns_ensemble takes it, with sample in 'rwalk' | 'rslice' | 'slice' | 'unif' on PCG64
        streams and bound in 'multi' | 'single'; a request the device refuses raises DynHipError (DH_ERR_ARG) and leaves
        the context usable.  A batch from the prior (logl_min = -inf) is ns_ensemble(nlive=nlive_new, logl_max=...).

        Returns ns_ensemble's dict (niter: the strand's own deaths; logz / logzerr / h: running values continued from
        the start row, which steer the dlogz stop and are not results) plus start_u, start_logl, start_nc (the live set
        the sampling phase began with), seed_ncall and seed_rng (the strand's generator at the hand-over)."""
        nd = prob.ndim
        seed_u = np.ascontiguousarray(seed_u, dtype=np.float64)
        seed_logl = np.ascontiguousarray(seed_logl, dtype=np.float64)
        if seed_u.ndim != 3 or seed_u.shape[2] != nd or seed_logl.shape != seed_u.shape[:2]:
            raise ValueError(f"ns_batch: seed_u {seed_u.shape} / seed_logl {seed_logl.shape} are not "
                             f"(runs, nlive_new, {nd}) / (runs, nlive_new)")
        runs, nlive = seed_logl.shape
        start = np.ascontiguousarray(np.broadcast_to(np.asarray(start, dtype=np.float64), (runs, 6)))
        if bound not in BOUND_CODES:
            raise ValueError(f"ns_batch: bound={bound!r}")
        # (rng='philox', the friends bounds and keep=True are passed on: the device refuses them and says why)
        kind, walks, enlarge, bootstrap = self._ns_sampler("ns_batch", nd, sample, rng, walks, slices, enlarge, bootstrap)
        words = entropy_words(entropy)
        buf = self._ns_buffers(runs, nlive, nd, max_iter, True, want_samples)
        start_u = np.empty((runs, nlive, nd))
        start_logl = np.empty((runs, nlive))
        start_nc = np.empty((runs, nlive), dtype=np.int32)
        seed_ncall = np.zeros(runs, dtype=np.int64)
        seed_rng = np.zeros((runs, 4), dtype=np.uint64)
        nf = C.c_int64(0)
        self._ns_arm(nd, nlive, update_interval, None, maxiter, maxcall, logl_max, add_live, forced_exact, periodic,
                     reflective)
        if keep:
            self._check(self.lib.dh_ns_keep(self.handle, 1))
        self._check(self.lib.dh_ns_batch(
            self.handle, self.problem(prob), int(runs), int(nlive), nd, int(queue_size), kind, int(walks),
            BOUND_CODES[bound], float(dlogz), float(enlarge), int(max_fills), int(max_iter), _ptr(words), words.size,
            int(first_run), _ptr(seed_u), _ptr(seed_logl), float(logl_min), _ptr(start), _ptr(buf["rec"]),
            _ptr(buf["dead"]), _ptr(buf["livel"]), _ptr(buf["dead_u"]), _ptr(buf["live_u"]), C.byref(nf), _ptr(buf["pid"]),
            _ptr(buf["pit"]), _ptr(buf["pnc"]), _ptr(buf["lit"]), int(bootstrap), int(rebuild_every), _ptr(start_u),
            _ptr(start_logl), _ptr(start_nc), _ptr(seed_ncall), _ptr(seed_rng)))
        out = self._ns_result(buf, nf, True, want_samples)
        out.update(start_u=start_u, start_logl=start_logl, start_nc=start_nc, seed_ncall=seed_ncall, seed_rng=seed_rng)
        return out

    def ns_continue(self, dlogz=0.01, max_fills=0, maxiter=None, maxcall=None, logl_max=None, add_live=True,
                    want_dead_logl=False, want_samples=False):
        """dh_ns_continue: takes the ensemble that ns_ensemble(keep=True) (or ns_load) left on the device further, as
        calling run_nested again does in the reference.  dlogz, maxiter, maxcall, logl_max and add_live are this
        call's; maxiter and maxcall are TOTALS of the run (iterations and calls since it began -- the reference counts
        them per call: add the records' niter / ncall for a per-call budget).  Everything else is the first call's.
        Runs the criteria already stop stay as they are (unchanged criteria: a no-op with nfills 0); runs that
        max_fills stopped (status 1) go on; failed runs stay failed.  max_fills bounds the fills of THIS call.
        Returns the dict of ns_ensemble (arrays over the whole run, dead rows runs x max_iter of the first call) plus
        `rest`: per run, the queue entries behind the stop that the run took over.  The ensemble stays kept."""
        if self._kept_shape is None:
            raise ValueError("ns_continue: the context holds no kept ensemble (ns_ensemble(keep=True) or ns_load)")
        runs, nlive, nd, max_iter = self._kept_shape
        rec = np.empty((runs, 8))
        want_dead_logl = want_dead_logl or want_samples
        dead = np.empty((runs, max_iter)) if want_dead_logl else None
        livel = np.empty((runs, nlive)) if want_dead_logl else None
        dead_u = np.empty((runs, max_iter, nd)) if want_samples else None
        live_u = np.empty((runs, nlive, nd)) if want_samples else None
        pid = np.empty((runs, max_iter), dtype=np.int32) if want_samples else None
        pit = np.empty((runs, max_iter), dtype=np.int32) if want_samples else None
        pnc = np.empty((runs, max_iter), dtype=np.int32) if want_samples else None
        lit = np.empty((runs, nlive), dtype=np.int32) if want_samples else None
        rest = np.zeros(runs, dtype=np.int32)
        nf = C.c_int64(0)
        nan = float('nan')
        # (only the four options a continuation takes are set: one of the others, set by the caller, is refused)
        for key, val in ((3, nan if maxiter is None else float(maxiter)), (4, nan if maxcall is None else float(maxcall)),
                         (5, nan if logl_max is None else float(logl_max)), (6, nan if add_live else 0.0)):
            self._check(self.lib.dh_ns_set_option(self.handle, key, val))
        self._check_merge(self.lib.dh_ns_continue(
            self.handle, float(dlogz), int(max_fills), _ptr(rec), _ptr(dead), _ptr(livel), _ptr(dead_u), _ptr(live_u),
            C.byref(nf), _ptr(pid), _ptr(pit), _ptr(pnc), _ptr(lit), _ptr(rest)))
        out = dict(logz=rec[:, 0], logzerr=rec[:, 1], niter=rec[:, 2].astype(np.int64),
                   ncall=rec[:, 3].astype(np.int64), h=rec[:, 4], nbound=rec[:, 5].astype(np.int64),
                   status=rec[:, 6].astype(np.int64), eff=rec[:, 7], nfills=nf.value, rest=rest.astype(np.int64))
        if want_dead_logl:
            out["dead_logl"] = dead
            out["live_logl"] = livel
        if want_samples:
            out["dead_u"] = dead_u
            out["live_u"] = live_u
            out["dead_id"], out["dead_it"], out["dead_nc"], out["live_it"] = pid, pit, pnc, lit
        return out

    def ns_state(self):
        """dh_ns_state_export: the kept ensemble as one np.uint8 array -- a header, the first call's plan and the state
        arrays, the dead points' by the rows each run produced (the size does not depend on max_iter)."""
        n = C.c_uint64(0)
        self._check_merge(self.lib.dh_ns_state_size(self.handle, C.byref(n)))
        buf = np.empty(int(n.value), dtype=np.uint8)
        self._check_merge(self.lib.dh_ns_state_export(self.handle, _ptr(buf), buf.size))
        return buf

    def ns_save(self, path):
        """ns_state() written to `path` (through a temporary file beside it, renamed when complete)."""
        tmp = f"{path}.tmp"
        with open(tmp, "wb") as f:
            f.write(self.ns_state().tobytes())
        os.replace(tmp, path)

    def ns_load(self, prob, path_or_array, max_iter=None):
        """dh_ns_state_import: installs a saved ensemble as the context's kept one (ns_continue, merge_kept).  prob
        must be the problem the ensemble was run on -- only its ndim can be checked; max_iter: the dead-point capacity,
        None = as saved, else >= every run's niter.  A rejected image (ValueError) leaves the context as it was."""
        if isinstance(path_or_array, (str, bytes, os.PathLike)):
            buf = np.fromfile(path_or_array, dtype=np.uint8)
        else:
            buf = np.ascontiguousarray(path_or_array, dtype=np.uint8).reshape(-1)
        self._check_merge(self.lib.dh_ns_state_import(self.handle, self.problem(prob), _ptr(buf), buf.size,
                                                      0 if max_iter is None else int(max_iter)))
        hdr = np.frombuffer(buf[:88].tobytes(), dtype=np.int32)  # csrc/ns_state.h: Header
        cap = int(np.frombuffer(buf[40:48].tobytes(), dtype=np.int64)[0])
        self._kept_shape = (int(hdr[6]), int(hdr[7]), int(hdr[8]), cap if max_iter is None else int(max_iter))

    # ---- RadFriends / SupFriends ------------------------------------------
    def bootstrap_expand(self, points, ent, bootstrap, multi, want_n_in=False):
        """dh_bootstrap_expand: points (runs, n, d), ent (runs, 4) uint64 ->
        (runs,) expansion factors (bounding.py:1619-1648, max over replicas)
        [, (runs, bootstrap) sample sizes]."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim == 2:
            pts = pts[None]
        runs, n, d = pts.shape
        ent = np.ascontiguousarray(ent, dtype=np.uint64).reshape(runs, 4)
        out = np.empty(runs)
        nin = np.empty((runs, int(bootstrap)), dtype=np.int32) if want_n_in else None
        self._check(self.lib.dh_bootstrap_expand(self.handle, runs, _ptr(pts), n, d, 1 if multi else 0,
                                                 int(bootstrap), _ptr(ent), _ptr(out), _ptr(nin)))
        return (out, nin) if want_n_in else out

    def friends_update(self, points, kind, am_prev=None, in_masks=None):
        """RadFriends.update / SupFriends.update (dh_friends_update).
        kind 'balls' | 'cubes'; am_prev = previous metric (None: no
        clustering); in_masks = (B, n) bool resampling masks or None (LOO)."""
        pts = _f64(points)
        n, d = pts.shape
        prev = None if am_prev is None else _f64(am_prev)
        nb, mk = 0, None
        if in_masks is not None and len(in_masks):
            mk = np.ascontiguousarray(in_masks, dtype=np.uint8)
            nb = mk.shape[0]
        cov = np.empty((d, d)); am = np.empty((d, d))
        axes = np.empty((d, d)); axes_inv = np.empty((d, d))
        lv = C.c_double(0.); rmax = C.c_double(0.); ncl = C.c_int32(0)
        self._check(self.lib.dh_friends_update(
            self.handle, _ptr(pts), n, d, 0 if kind == 'balls' else 1,
            _ptr(prev), nb, _ptr(mk), _ptr(cov), _ptr(am), _ptr(axes),
            _ptr(axes_inv), C.byref(lv), C.byref(rmax), C.byref(ncl)))
        return dict(cov=cov, am=am, axes=axes, axes_inv=axes_inv,
                    logvol=lv.value, rmax=rmax.value, nclusters=ncl.value)

    def friends_update_batch(self, points, kind, am_prev=None, in_masks=None, active=None, out=None):
        """dh_friends_update over runs at once (dh_friends_update_batch).  points (runs, n, d); am_prev (runs, d, d)
        or None (no clustering); in_masks (runs, B, n) bool or None (leave-one-out); active (runs,) bool or None (all).
        out: optional dict of arrays as returned, whose inactive (and failed) runs are left untouched; returns dict
        cov / am / axes / axes_inv (runs, d, d), logvol / rmax (runs,), nclusters / status (runs,) int32."""
        pts = np.ascontiguousarray(points, dtype=np.float64)
        runs, n, d = pts.shape
        prev = None if am_prev is None else np.ascontiguousarray(am_prev, dtype=np.float64).reshape(runs, d, d)
        nb, mk = 0, None
        if in_masks is not None and np.asarray(in_masks).shape[1]:
            mk = np.ascontiguousarray(in_masks, dtype=np.uint8).reshape(runs, -1, n)
            nb = mk.shape[1]
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32).reshape(runs)
        if out is None:
            out = dict(cov=np.zeros((runs, d, d)), am=np.zeros((runs, d, d)), axes=np.zeros((runs, d, d)),
                       axes_inv=np.zeros((runs, d, d)), logvol=np.zeros(runs), rmax=np.zeros(runs),
                       nclusters=np.zeros(runs, dtype=np.int32), status=np.zeros(runs, dtype=np.int32))
        self._check(self.lib.dh_friends_update_batch(
            self.handle, runs, _ptr(pts), n, d, 0 if kind == 'balls' else 1, _ptr(prev), nb, _ptr(mk), _ptr(act),
            _ptr(out["cov"]), _ptr(out["am"]), _ptr(out["axes"]), _ptr(out["axes_inv"]), _ptr(out["logvol"]),
            _ptr(out["rmax"]), _ptr(out["nclusters"]), _ptr(out["status"])))
        return out

    def friends_within(self, ctrs, kind, axes_inv, x, want_bits=False):
        """Counts (and optionally index bit rows) of the balls / cubes that
        contain each row of x (dh_friends_within)."""
        c = _f64(ctrs)
        n, d = c.shape
        xs = _f64(x).reshape(-1, d)
        m = xs.shape[0]
        counts = np.empty(m, dtype=np.int32)
        bits = np.empty((m, (n + 63) // 64), dtype=np.uint64) if want_bits \
            else None
        self._check(self.lib.dh_friends_within(
            self.handle, _ptr(c), n, d, 0 if kind == 'balls' else 1,
            _ptr(_f64(axes_inv)), _ptr(xs), m, _ptr(counts), _ptr(bits)))
        return counts, bits

    def friends_draw(self, state6, nsamp, ctrs, kind, axes, axes_inv,
                     return_q=False):
        """Bound.samples from one generator state (dh_friends_draw)."""
        c = _f64(ctrs)
        n, d = c.shape
        st = np.ascontiguousarray(state6, dtype=np.uint64)
        xs = np.empty((nsamp, d))
        qs = np.empty(nsamp, dtype=np.int32)
        out = np.empty(6, dtype=np.uint64)
        self._check(self.lib.dh_friends_draw(
            self.handle, _ptr(st), int(nsamp), _ptr(c), n, d,
            0 if kind == 'balls' else 1, _ptr(_f64(axes)),
            _ptr(_f64(axes_inv)), 1 if return_q else 0, _ptr(xs), _ptr(qs),
            _ptr(out)))
        return xs, qs, out

    def bound_draw(self, state4, nsamp, ctrs, axes, ams=None, logvol_ells=None,
                   return_q=False):
        """Bound.samples from one generator state (dh_bound_draw)."""
        c = _f64(ctrs)
        if c.ndim == 1:
            c = c[None, :]
        m, d = c.shape
        ax = _f64(axes).reshape(m, d, d)
        am = cp = None
        if m > 1:
            am = _f64(ams).reshape(m, d, d)
            cp = cumprob_of(logvol_ells)
        st = np.ascontiguousarray(state4, dtype=np.uint64)
        xs = np.empty((nsamp, d))
        idxs = np.empty(nsamp, dtype=np.int32)
        qs = np.empty(nsamp, dtype=np.int32)
        out = np.empty(4, dtype=np.uint64)
        self._check(self.lib.dh_bound_draw(
            self.handle, _ptr(st), int(nsamp), d, m, _ptr(c), _ptr(ax),
            _ptr(am), _ptr(cp), 1 if return_q else 0, _ptr(xs), _ptr(idxs),
            _ptr(qs), _ptr(out)))
        return xs, idxs, qs, out


def cumprob_of(logvol_ells):
    """cumsum(exp(logvol_ells - logsumexp(logvol_ells))) exactly as
    rand_choice sees it (bounding.py:543, 1300-1308)."""
    from scipy.special import logsumexp
    lv = np.asarray(logvol_ells, dtype=np.float64)
    return np.ascontiguousarray(np.cumsum(np.exp(lv - logsumexp(lv))))


_default_ctx = {}


def default_context(device=0):
    """Process-wide context per device (created lazily)."""
    ctx = _default_ctx.get(device)
    if ctx is None or ctx.handle is None:
        ctx = Context(device)
        _default_ctx[device] = ctx
    return ctx
