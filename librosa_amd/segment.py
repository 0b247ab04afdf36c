"""Neighbour graphs of feature sequences: ``librosa.segment.cross_similarity`` and ``recurrence_matrix`` (``librosa/segment.py:67-357``,
``:361-706``, ``__affinity_bandwidth`` ``:1332-1437``).

Both have the reference's signatures, argument checks, ``ParameterError`` texts, shapes, dtypes and orientation (the result is ``[n_ref, n]``, the
transpose of the neighbour graph).  The host validates and reshapes as the reference does (``atleast_2d``, ``swapaxes``, the F-order flatten, the
``width`` bound, the defaults of ``k``); all arithmetic on the data runs on the device (``csrc/lra_knn.h``):

* ``knn_select`` finds the ``k`` nearest candidates of every frame without ever forming the ``n x n_ref`` distance matrix: a workgroup owns
  ``KNN_ROWS`` query frames, sweeps the candidates in tiles of ``KNN_TILE`` frames, and keeps each row's running list in LDS.  Device memory is
  ``O(n k + n d)``.  The candidates of ``recurrence_matrix`` are the frames ``j`` with ``|i - j| >= width`` (the reference asks for ``k + 2 width``
  neighbours, clears the band and keeps the ``k`` smallest non-zero links: the survivors are the nearest out-of-band frames); those of
  ``cross_similarity`` are all of ``data_ref``, ``min(n_ref, k)`` of them kept.  Ties in distance go to the lower index.
* ``knn_sort_rows``, ``knn_mutual`` (``sym``), ``knn_bandwidth`` / ``knn_median`` (the affinity bandwidths and their status words) and ``knn_emit``
  turn the lists into the compressed arrays or the dense result.
* where every candidate is kept (``full=True``, or ``k`` at least the candidate count) ``knn_dense`` writes the transposed matrix straight from
  the distances; ``knn_select`` still supplies the rows' ``bandwidth_k`` statistics.

A stored distance of exactly zero is dropped in ``distance`` and ``affinity`` mode, as the reference's ``eliminate_zeros`` does.  Results are
``bool`` for connectivity and ``float64`` otherwise.  NumPy in gives NumPy or ``scipy.sparse.csc_array`` (sorted ``int32`` indices, no explicit
zeros) out; a device tensor in gives a device tensor out: dense, or for ``sparse=True`` a ``torch.sparse_csc_tensor`` over the device arrays, whose
``ccol_indices`` and ``row_indices`` are ``int32`` (torch takes ``int32`` or ``int64`` there, both of one type).  The input is never written.

Differences from the reference:

1. ``recurrence_matrix(mode="connectivity")`` returns the pattern of the ``k`` nearest out-of-band frames -- what the docstring promises and what
   ``mode="distance"`` returns.  The reference cuts its ``k + 2 width`` neighbours down with ``np.argsort`` over a row of ones, so which links it
   keeps depends on NumPy's sort of equal keys.  Where ``k`` covers every candidate nothing is cut and the two agree.
2. ``metric`` is one of ``euclidean``, ``sqeuclidean``, ``cityblock`` (``manhattan``) and ``cosine``; anything else raises ``ParameterError``.
3. Distances are float64 direct sums over the features in ascending order (``sequence.dtw``'s metric body with every operation rounded on its
   own, float32 input widened exactly), not scikit-learn's kd-tree or GEMM expansion: values agree to rounding.
4. Integer and bool features are widened to float64; complex or empty input raises ``ParameterError``.
5. A ``k`` above ``KNN_MAX_K`` = 2048 that does not cover every candidate raises ``ParameterError`` (a row's list lives in LDS); so does a
   ``bandwidth_k`` above it where a string ``bandwidth`` needs the rows' statistics.  ``k < 1`` raises ``ParameterError``.
6. The per-point bandwidths of ``cross_similarity`` index the query frames' statistics by the reference frame, as the reference does; where
   ``n_ref > n`` that index can leave the table (the reference: ``IndexError``) and ``ParameterError`` is raised.
7. A sparse result of the dense route is made from the dense matrix, so an affinity that underflows to 0 is not stored.
"""
from __future__ import annotations

import numpy as np

from . import _arrays
from .util.exceptions import ParameterError
from .util.utils import is_torch_tensor

__all__ = ["cross_similarity", "recurrence_matrix"]   # the neighbour graphs (pinned by tests/test_knn_host.py); the path-enhancement and time-lag functions
ENHANCE_NAMES = ["path_enhance", "recurrence_to_lag", "lag_to_recurrence", "timelag_filter"]   # below are public attributes of this module as well

KNN_ROWS = 0        # query frames per workgroup of the selection kernel: 0 for the library's choice, or a power of two up to 16
KNN_TILE = 0        # candidate frames per tile: 0 for the library's choice, or a power of two from 4 to 1024 (rows * tile at most 2048)
KNN_MAX_K = 2048    # LRA_KNN_MAX_K: the longest list a row keeps in LDS

METRICS = {"euclidean": "euclidean", "sqeuclidean": "sqeuclidean", "cityblock": "cityblock", "manhattan": "cityblock", "cosine": "cosine"}
_MODES = ["connectivity", "distance", "affinity"]
_BW_MODES = ["med_k_scalar", "mean_k", "gmean_k", "mean_k_avg", "gmean_k_avg", "mean_k_avg_and_pair"]


def _atleast_2d(x):
    if not (is_torch_tensor(x) or isinstance(x, np.ndarray)):
        x = np.asarray(x)
    if x.ndim >= 2:
        return x
    return x.reshape((1, -1)) if x.ndim == 1 else x.reshape((1, 1))


def _frames(x, axis):
    """``np.swapaxes(x, axis, 0).reshape((n, -1), order="F")`` transposed: the features of every frame as the contiguous table [d][n] the
    kernels read (``(n, d)`` in F order has the leading axes fastest: it is the C-order flatten of the reversed axes).  Returns (table, n)."""
    x = x.swapaxes(axis, 0)
    n = int(x.shape[0])
    rev = tuple(range(x.ndim - 1, -1, -1))
    x = x.permute(rev) if is_torch_tensor(x) else x.transpose(rev)
    if n == 0 or int(np.prod(x.shape[:-1])) == 0:
        raise ParameterError(f"the features are empty: {n} frames of {int(np.prod(x.shape[:-1]))} features")
    return x.reshape((-1, n)), n


def _real_type(*arrays):
    """float32 where every table is float32, else float64; complex raises."""
    kinds = []
    for a in arrays:
        if is_torch_tensor(a):   # (any integer width, bool and the half types are widened by the upload)
            kinds.append(np.dtype(np.complex128 if a.is_complex() else np.float32 if a.dtype == _arrays.torch_dtype(np.float32) else np.float64))
        else:
            kinds.append(np.dtype(_arrays.numpy_dtype_of(a)))
    for k in kinds:
        if k.kind not in "biuf":
            raise ParameterError(f"the features must be real-valued, given dtype={k}")
    return np.dtype(np.float32) if all(k == np.float32 for k in kinds) else np.dtype(np.float64)


def _same_kind(sess, a, real):
    """``a`` as the session's kind of array, of type ``real``."""
    if sess.is_torch:
        import torch

        if not is_torch_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=real)).to(sess.device)
        return a.to(sess.device)
    if is_torch_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _check_metric(metric):
    if not isinstance(metric, str) or metric not in METRICS:
        raise ParameterError(f"metric={metric!r} is not served on the device: one of {', '.join(METRICS)}")
    return METRICS[metric]


def _check_mode(mode):
    if mode not in _MODES:
        raise ParameterError(f"Invalid mode='{mode}'. Must be one of ['connectivity', 'distance', 'affinity']")


def _check_bandwidth(bandwidth, shape):
    """``__affinity_bandwidth``'s checks that need no data (:1340-1376).  Returns ("matrix", array) | ("scalar", float) | (mode name, None)."""
    if isinstance(bandwidth, np.ndarray) or is_torch_tensor(bandwidth):
        if tuple(bandwidth.shape) != tuple(shape):
            raise ParameterError(f"Invalid matrix bandwidth shape: {tuple(bandwidth.shape)}.Should be {tuple(shape)}.")
        return "matrix", bandwidth
    if isinstance(bandwidth, (int, float)):
        scalar_bandwidth = float(bandwidth)
        if scalar_bandwidth <= 0:
            raise ParameterError(f"Invalid scalar bandwidth={scalar_bandwidth}. Must be strictly positive.")
        return "scalar", scalar_bandwidth
    if bandwidth is None:
        bandwidth = "med_k_scalar"
    if not isinstance(bandwidth, str) or bandwidth not in _BW_MODES:
        raise ParameterError(
            f"Invalid bandwidth='{bandwidth}'. Must be either a positive scalar or one of "
            "['med_k_scalar', 'mean_k', 'gmean_k', 'mean_k_avg', 'gmean_k_avg', 'mean_k_avg_and_pair']"
        )
    return bandwidth, None


def _too_large(name, value):
    return ParameterError(f"{name}={value} is too large for the device's neighbour search: a frame keeps at most KNN_MAX_K={KNN_MAX_K} neighbours unless k covers every candidate")


def _graph(data, data_ref, q, r, n, n_ref, *, k, bandwidth_k, width, metric, sym, sparse, mode, bandwidth, self_link, recurrence):
    """The result [n_ref, n] of the neighbour graph of the query table ``q`` [d][n] against ``r`` [d][n_ref] (``r is q`` for a recurrence matrix):
    row i of the graph holds the ``k`` nearest of the frames j with ``|i - j| >= width``."""
    affinity, connectivity = mode == "affinity", mode == "connectivity"
    max_candidates = n_ref - width   # (of the first and the last frame; a frame in the middle has fewer)
    k_sel = min(k, max_candidates)
    dense_route = k >= max_candidates
    if not dense_route and k_sel > KNN_MAX_K:
        raise _too_large("k", k)
    kind, bw = _check_bandwidth(bandwidth, (n, n_ref)) if affinity else ("scalar", 1.0)
    per_point = kind not in ("matrix", "scalar", "med_k_scalar")
    stats = affinity and kind not in ("matrix", "scalar")
    if per_point and n_ref > n:
        raise ParameterError(f"bandwidth='{kind}' needs a statistic of every frame of data_ref, but only the n={n} frames of data have one (n_ref={n_ref})")
    k_stats = min(bandwidth_k, max_candidates)
    if stats and dense_route and k_stats > KNN_MAX_K:
        raise _too_large("bandwidth_k", bandwidth_k)
    real = _real_type(q) if r is q else _real_type(q, r)
    stored_self = bool(self_link) and mode != "distance"
    skip_zero = recurrence and not connectivity   # (the reference's top-k loop looks at non-zero links only; cross_similarity's takes every neighbour it asked for)

    sess = _arrays.Session(data)
    try:
        ctx = sess.ctx
        metric_code, mode_code = ctx.DTW_METRICS[metric], ctx.KNN_MODES[mode]
        q_ptr = sess.input_raw(_same_kind(sess, q, real), real)
        r_ptr = q_ptr if r is q else sess.input_raw(_same_kind(sess, r, real), real)
        d = int(q.shape[0])
        work = sess.scratch(ctx.KNN_WORK_BYTES)
        matrix_ptr = 0
        if kind == "matrix":
            matrix_ptr = sess.input_raw(_same_kind(sess, bw, np.float64), np.float64)
            if ctx.knn_bw_check_exec(matrix_ptr, n * n_ref, work) & ctx.KNN_STATUS_NON_POSITIVE:
                raise ParameterError("Invalid bandwidth. All entries must be strictly positive.")

        def lists(k_list, zero_skipped):
            cnt = sess.scratch(4 * n)
            idx = sess.scratch(4 * n * k_list)
            dist = sess.scratch(8 * n * k_list)
            ctx.knn_select_exec(q_ptr, r_ptr, real, d, n, n_ref, metric_code, k_list, width, zero_skipped, KNN_ROWS, KNN_TILE, cnt, idx, dist)
            return cnt, idx, dist

        def statistics(k_list, cnt, dist, keep):
            """(bw_mode, bw_on_device, sigma) of a string bandwidth, from the rows' stored distances."""
            dist_to_k, avg = sess.scratch(8 * n), sess.scratch(8 * n)
            status, first_empty = ctx.knn_bandwidth_exec(n, k_list, cnt, dist, keep, stored_self and affinity, bandwidth_k, kind == "med_k_scalar", dist_to_k, avg, work)
            if per_point and status & ctx.KNN_STATUS_ROW_EMPTY:
                raise ParameterError(f"The sample at time point {first_empty} has no neighbors")
            if not per_point and status & ctx.KNN_STATUS_EMPTY_GRAPH:
                raise ParameterError("Cannot estimate bandwidth from an empty graph")
            return ctx.KNN_BW_MODES[kind], not per_point, avg if "avg" in kind else dist_to_k

        bw_mode, bw_on_device, sigma = (ctx.KNN_BW_MATRIX if kind == "matrix" else ctx.KNN_BW_SCALAR), False, 0
        out_type = np.uint8 if connectivity else np.float64

        def finish(a):
            if not connectivity:
                return a
            return a.view(_arrays._torch().bool) if sess.is_torch else a.view(np.bool_)

        if dense_route:
            if stats:
                cnt, idx, dist = lists(k_stats, True)
                bw_mode, bw_on_device, sigma = statistics(k_stats, cnt, dist, 0)
            out_ptr, out_h = sess.output((n_ref, n), out_type)
            ctx.knn_dense_exec(q_ptr, r_ptr, real, d, n, n_ref, metric_code, width, stored_self, mode_code, bw_mode, bw if kind == "scalar" else 0.0, bw_on_device, sigma, matrix_ptr, work,
                               out_ptr)
            out = finish(sess.result(out_h))
            if not sparse:
                return out
            if sess.is_torch:
                torch = _arrays._torch()
                csc = out.to_sparse_csc()
                return torch.sparse_csc_tensor(csc.ccol_indices().to(torch.int32), csc.row_indices().to(torch.int32), csc.values(), size=(n_ref, n))
            import scipy.sparse

            return scipy.sparse.csc_array(out)

        cnt, idx, dist = lists(k_sel, skip_zero)
        keep = sess.scratch(n * k_sel)
        ctx.knn_mutual_exec(n, k_sel, cnt, idx, dist, sym, not connectivity, keep)
        if stats:
            bw_mode, bw_on_device, sigma = statistics(k_sel, cnt, dist, keep)
        common = (n, n_ref, k_sel, cnt, idx, dist, keep, stored_self, mode_code, bw_mode, bw if kind == "scalar" else 0.0, bw_on_device, sigma, matrix_ptr, work)
        if not sparse:
            out_ptr, out_h = sess.output((n_ref, n), out_type)
            ctx.knn_emit_exec(*common, 0, 0, 0, 0, out_ptr)
            return finish(sess.result(out_h))
        cap = n * (k_sel + 1)
        if cap >= 2**31:
            raise ParameterError(f"a sparse result of up to {cap} entries does not fit int32 index arrays")
        indptr_ptr, indptr_h = sess.output((n + 1,), np.int32)
        indices_ptr, indices_h = sess.output((cap,), np.int32)
        data_ptr, data_h = sess.output((cap,), out_type)
        total = ctx.knn_emit_exec(*common, sess.scratch(4 * n), indptr_ptr, indices_ptr, data_ptr, 0)
        indptr, indices, values = sess.result(indptr_h), sess.result(indices_h)[:total], finish(sess.result(data_h)[:total])
        if sess.is_torch:
            return _arrays._torch().sparse_csc_tensor(indptr, indices, values, size=(n_ref, n))
        import scipy.sparse

        return scipy.sparse.csc_array((values.copy(), indices.copy(), indptr), shape=(n_ref, n))
    finally:
        sess.close()


def cross_similarity(data, data_ref, *, k=None, metric="euclidean", sparse=False, mode="connectivity", bandwidth=None, full=False):
    """Cross-similarity of two feature sequences (``librosa/segment.py:67-357``): ``xsim[i, j]`` links frame ``j`` of ``data`` to frame ``i`` of
    ``data_ref`` where ``i`` is among the ``k`` nearest frames of ``data_ref``; shape (n_ref, n), bool for ``mode="connectivity"`` and float64
    otherwise, computed on the device.  NumPy input gives ``np.ndarray`` or ``scipy.sparse.csc_array``, a tensor on the device gives a tensor there
    (``torch.sparse_csc_tensor`` with int32 indices for ``sparse=True``).  Differences from the reference: the module docstring."""
    data_ref = _atleast_2d(data_ref)
    data = _atleast_2d(data)
    if tuple(data_ref.shape[:-1]) != tuple(data.shape[:-1]):
        raise ParameterError(f"data_ref.shape={tuple(data_ref.shape)} and data.shape={tuple(data.shape)} do not match on leading dimension(s)")
    r, n_ref = _frames(data_ref, -1)
    q, n = _frames(data, -1)
    _check_mode(mode)
    metric = _check_metric(metric)
    if k is None:
        k = min(n_ref, 2 * np.ceil(np.sqrt(n_ref)))
    k = int(k)
    if k < 1:
        raise ParameterError(f"k={k} must be a positive integer")
    bandwidth_k = k
    if full and (mode != "connectivity"):
        k = n
    return _graph(data, data_ref, q, r, n, n_ref, k=min(n_ref, k), bandwidth_k=bandwidth_k, width=0, metric=metric, sym=False, sparse=sparse, mode=mode, bandwidth=bandwidth,
                  self_link=False, recurrence=False)


def recurrence_matrix(data, *, k=None, width=1, metric="euclidean", sym=False, sparse=False, mode="connectivity", bandwidth=None, self=False, axis=-1, full=False):
    """Recurrence matrix of a feature sequence (``librosa/segment.py:361-706``): ``rec[i, j]`` links frame ``j`` to frame ``i`` where ``i`` is among
    the ``k`` nearest frames at least ``width`` frames away; shape (t, t), bool for ``mode="connectivity"`` and float64 otherwise, computed on the
    device.  NumPy input gives ``np.ndarray`` or ``scipy.sparse.csc_array``, a tensor on the device gives a tensor there
    (``torch.sparse_csc_tensor`` with int32 indices for ``sparse=True``).  Differences from the reference: the module docstring."""
    data = _atleast_2d(data)
    q, t = _frames(data, axis)
    if width < 1 or width >= (t - 1) // 2:
        raise ParameterError("width={} must be at least 1 and at most (data.shape[{}] - 1) // 2={}".format(width, axis, (t - 1) // 2))
    _check_mode(mode)
    metric = _check_metric(metric)
    if k is None:
        k = 2 * np.ceil(np.sqrt(t - 2 * width + 1))
    k = int(k)
    if k < 1:
        raise ParameterError(f"k={k} must be a positive integer")
    bandwidth_k = k
    width = int(width)
    if full and (mode != "connectivity"):
        k, width = t, 1   # (every other frame: the band is not cleared, the diagonal is)
    return _graph(data, data, q, q, t, t, k=k, bandwidth_k=bandwidth_k, width=width, metric=metric, sym=sym, sparse=sparse, mode=mode, bandwidth=bandwidth, self_link=self,
                  recurrence=True)


# ---------------------------------------------------------------------------------------------------
# path_enhance and the time-lag view: librosa/segment.py:1167-1329, :709-972
# ---------------------------------------------------------------------------------------------------
ENHANCE_ROWS = 0          # output rows per workgroup of the enhancement kernel: 0 (with ENHANCE_COLS 0) for the library's choice, or 1 .. 256
ENHANCE_COLS = 0          # output columns per workgroup: 0, or 16, 32 or 64 (rows * cols at most 4096; tile plus halo must fit the LDS)
ENHANCE_MAX_REACH = 124   # LRA_ENHANCE_MAX_REACH: the largest filter side is ENHANCE_MAX_REACH + 1 (the halo lives in LDS next to the tile)

_ND_MODES = {"reflect": "reflect", "grid-mirror": "reflect", "constant": "constant", "grid-constant": "constant", "nearest": "nearest", "mirror": "mirror", "wrap": "wrap",
             "grid-wrap": "wrap"}
_ND_EPS = float(np.finfo(np.float64).eps)   # scipy.ndimage visits the weights with fabs(w) > DBL_EPSILON
_INVALID_ORIGIN = "Invalid origin; origin must satisfy -(weights.shape[k] // 2) <= origin[k] <= (weights.shape[k]-1) // 2"


def _filter_taps(kernels, origin=(0, 0)):
    """The tap table of ``scipy.ndimage.convolve`` for a list of 2-D kernels: per kernel the weights of the flipped kernel that
    ``scipy.ndimage`` visits (``fabs(w) > DBL_EPSILON``: exact zeros, rounding noise of the rotation and NaN are left out) in row-major order, each a row offset, a column offset and the weight (``_native.Context.ENHANCE_TAP``), and the kernels' ranges ``starts``.  With
    ``Kf = K[::-1, ::-1]``, side ``m`` and ``o = -origin - (1 if m is even else 0)`` per axis, ``out[i, j]`` sums ``R[ext(i + a - m // 2 - o),
    ext(j + b - m // 2 - o)] * Kf[a, b]`` over ``(a, b)``.  An origin outside SciPy's bounds raises ``ParameterError`` with SciPy's text."""
    from ._native import Context

    parts, starts = [], [0]
    for K in kernels:
        K = np.asarray(K, dtype=np.float64)
        Kf = K[::-1, ::-1]
        shift = []
        for m, org in zip(K.shape, origin):
            o = -int(org) - (0 if m & 1 else 1)
            if o < -(m // 2) or o > (m - 1) // 2:
                raise ParameterError(_INVALID_ORIGIN)
            shift.append(m // 2 + o)
        a, b = np.nonzero(np.abs(Kf) > _ND_EPS)   # (row-major; scipy.ndimage's footprint test, which also leaves a NaN weight out)
        taps = np.empty(a.size, dtype=Context.ENHANCE_TAP)
        taps["dr"], taps["dc"], taps["w"] = a - shift[0], b - shift[1], Kf[a, b]
        parts.append(taps)
        starts.append(starts[-1] + int(a.size))
    return np.concatenate(parts), np.asarray(starts, dtype=np.int32)


def _enhance_kwargs(kwargs, ndim):
    """(mode, cval, (origin_row, origin_col)) of the keyword arguments ``scipy.ndimage.convolve`` takes here."""
    for key in kwargs:
        if key not in ("mode", "cval", "origin"):
            raise ParameterError(f"path_enhance: the keyword argument {key!r} of scipy.ndimage.convolve is not served on the device (mode, cval and origin are)")
    mode = kwargs.get("mode", "reflect")
    if not isinstance(mode, str):
        raise ParameterError(f"path_enhance: the keyword argument 'mode' must be one string for all axes, given {mode!r}")
    if mode not in _ND_MODES:
        raise ParameterError(f"path_enhance: mode={mode!r} is not a boundary mode of scipy.ndimage.convolve: one of {', '.join(_ND_MODES)}")
    cval = float(kwargs.get("cval", 0.0))
    origin = kwargs.get("origin", 0)
    if np.ndim(origin) == 0:
        origin = [int(origin)] * ndim
    else:
        origin = [int(o) for o in origin]
        if len(origin) == 2 and ndim > 2:
            origin = [0] * (ndim - 2) + origin   # (a pair: the matrix axes)
        if len(origin) != ndim:
            raise ParameterError(f"path_enhance: origin must be an integer or a pair, given {len(origin)} entries")
    if any(origin[:-2]):   # (the kernel has side 1 along a channel axis)
        raise ParameterError(_INVALID_ORIGIN)
    return _ND_MODES[mode], cval, (origin[-2], origin[-1])


def path_enhance(R, n, *, window="hann", max_ratio=2.0, min_ratio=None, n_filters=7, zero_mean=False, clip=True, **kwargs):
    """Multi-angle path enhancement of a self- or cross-similarity matrix (``librosa/segment.py:1167-1329``): the element-wise maximum of ``R``
    convolved with ``n_filters`` diagonal smoothing filters (``filters.diagonal_filter``) whose slopes run from ``min_ratio`` to ``max_ratio``,
    clipped at 0 with ``clip``.  ``R`` is ``(..., h, w)``, float32 or float64; leading axes are independent channels.  One launch computes every
    filter (``csrc/lra_enhance.h``); each response has the bits ``scipy.ndimage.convolve`` gives.  ``**kwargs``: ``mode``, ``cval`` and ``origin`` of
    ``scipy.ndimage.convolve``.  NumPy in gives NumPy out, a device tensor gives a device tensor; the input is never written.

    Differences from the reference: bool and integer ``R`` raise ``ParameterError`` (SciPy would truncate every response to the
    input's type); so do complex or sparse ``R``, fewer than 2 dimensions, ``n_filters < 1``, any other keyword argument, and filters wider than
    ``ENHANCE_MAX_REACH + 1`` cells."""
    from . import filters

    if min_ratio is None:
        min_ratio = 1.0 / max_ratio
    elif min_ratio > max_ratio:
        raise ParameterError(f"min_ratio={min_ratio} cannot exceed max_ratio={max_ratio}")
    if n_filters is None or int(n_filters) < 1:
        raise ParameterError(f"n_filters={n_filters} must be a positive integer")
    if not (is_torch_tensor(R) or isinstance(R, np.ndarray)):
        if hasattr(R, "tocsr") or hasattr(R, "todense"):
            raise ParameterError("path_enhance does not support sparse input: convert R to a dense array")
        R = np.asarray(R)
    if is_torch_tensor(R) and (R.is_sparse or R.layout != _arrays._torch().strided):
        raise ParameterError("path_enhance does not support sparse input: convert R to a dense tensor")
    if R.ndim < 2:
        raise ParameterError(f"R must have at least 2 dimensions, given R.shape={tuple(R.shape)}")
    if is_torch_tensor(R):
        torch = _arrays._torch()
        if R.is_complex():
            raise ParameterError(f"R must be real-valued, given dtype={R.dtype}")
        if R.dtype not in (torch.float32, torch.float64):
            raise ParameterError(f"R must be float32 or float64, given dtype={R.dtype}: convert it (an integer matrix would truncate every filter response)")
        real = np.dtype(np.float32 if R.dtype == torch.float32 else np.float64)
    else:
        if R.dtype.kind == "c":
            raise ParameterError(f"R must be real-valued, given dtype={R.dtype}")
        if R.dtype not in (np.float32, np.float64):
            raise ParameterError(f"R must be float32 or float64, given dtype={R.dtype}: convert it (an integer matrix would truncate every filter response)")
        real = R.dtype
    mode, cval, origin = _enhance_kwargs(kwargs, R.ndim)
    ratios = np.logspace(np.log2(min_ratio), np.log2(max_ratio), num=int(n_filters), base=2)
    kernels = [filters.diagonal_filter_cached(window, n, slope=ratio, zero_mean=zero_mean) for ratio in ratios]
    side = max(max(K.shape) for K in kernels)
    if side - 1 > ENHANCE_MAX_REACH:
        raise ParameterError(f"path_enhance: the widest of the filters spans {side} cells, above ENHANCE_MAX_REACH + 1 = {ENHANCE_MAX_REACH + 1}: its halo does not fit the LDS next to a tile")
    taps, starts = _filter_taps(kernels, origin)
    shape = tuple(int(s) for s in R.shape)
    h, w = shape[-2:]
    channels = int(np.prod(shape[:-2], dtype=np.int64))
    if channels * h * w == 0:
        raise ParameterError(f"R is empty: R.shape={shape}")
    halo = (int(taps["dr"].max(initial=0) - taps["dr"].min(initial=0)), int(taps["dc"].max(initial=0) - taps["dc"].min(initial=0)))
    sess = _arrays.Session(R)
    try:
        ctx = sess.ctx
        if (ENHANCE_ROWS or ENHANCE_COLS) and not ctx.lib.lra_enhance_lds_bytes(int(ENHANCE_ROWS), int(ENHANCE_COLS), *halo):
            raise ParameterError(f"ENHANCE_ROWS={ENHANCE_ROWS}, ENHANCE_COLS={ENHANCE_COLS}: rows 1 .. 256, cols 16, 32 or 64, rows * cols at most 4096, and the tile with its halo of "
                                 f"{halo[0]} rows and {halo[1]} columns must fit ENHANCE_LDS_MAX={ctx.ENHANCE_LDS_MAX} bytes of LDS as float64")
        r_ptr = sess.input_raw(R, real)
        table = sess.scratch(ctx.enhance_table_bytes(taps.size, starts.size - 1))
        out_ptr, out_h = sess.output(shape, real)
        ctx.path_enhance_exec(r_ptr, real, channels, h, w, taps, starts, ctx.ENHANCE_MODES[mode], cval, clip, ENHANCE_ROWS, ENHANCE_COLS, table, out_ptr)
        return sess.result(out_h)
    finally:
        sess.close()


def recurrence_to_lag(rec, *, pad=True, axis=-1):
    """Recurrence matrix to lag matrix, ``lag[i, j] == rec[i + j, j]`` (``librosa/segment.py:709-813``).  A dense matrix of any real or bool type,
    NumPy or a device tensor, is moved by one gather launch, the zero padding of ``pad=True`` folded in; ``scipy.sparse`` input is handled on
    the host as the reference does (index arithmetic only), its format kept."""
    from .util.utils import _is_scipy_sparse, _shear_dense, shear

    axis = int(np.abs(axis))
    if rec.ndim != 2 or rec.shape[0] != rec.shape[1]:
        raise ParameterError(f"non-square recurrence matrix shape: {tuple(rec.shape)}")
    if _is_scipy_sparse(rec):
        import scipy.sparse

        fmt = rec.format
        if pad:
            padding = np.asarray([[1, 0]], dtype=rec.dtype).swapaxes(axis, 0)
            rec = scipy.sparse.kron(padding, rec, format="csr" if axis == 0 else "csc")
        return shear(rec, factor=-1, axis=axis).asformat(fmt)
    t = int(rec.shape[axis])
    out_shape = [t, t]
    if pad:
        out_shape[1 - axis] = 2 * t
    return _shear_dense(rec, factor=-1, axis=axis, period=out_shape[1 - axis], out_shape=tuple(out_shape))


def lag_to_recurrence(lag, *, axis=-1):
    """Lag matrix to recurrence matrix (``librosa/segment.py:816-891``): the shear and the slice of the padded half in one gather launch for a
    dense matrix; ``scipy.sparse`` input on the host as the reference does."""
    from .util.utils import _is_scipy_sparse, _shear_dense, shear

    if axis not in [0, 1, -1]:
        raise ParameterError(f"Invalid target axis: {axis}")
    axis = int(np.abs(axis))
    if lag.ndim != 2 or (lag.shape[0] != lag.shape[1] and lag.shape[1 - axis] != 2 * lag.shape[axis]):
        raise ParameterError(f"Invalid lag matrix shape: {tuple(lag.shape)}")
    t = int(lag.shape[axis])
    if _is_scipy_sparse(lag):
        rec = shear(lag, factor=+1, axis=axis)
        sub_slice = [slice(None)] * rec.ndim
        sub_slice[1 - axis] = slice(t)
        if rec.format == "coo":   # (not subscriptable: sliced in a compressed form, the format put back)
            return rec.tocsc()[tuple(sub_slice)].asformat("coo")
        return rec[tuple(sub_slice)]
    return _shear_dense(lag, factor=+1, axis=axis, period=int(lag.shape[1 - axis]), out_shape=(t, t))


def timelag_filter(function, pad=True, index=0):
    """Wrap ``function`` so that it filters in the time-lag domain (``librosa/segment.py:895-972``): the argument at ``index`` goes through
    ``recurrence_to_lag(pad=pad)``, the result through ``lag_to_recurrence``."""
    import functools

    @functools.wraps(function)
    def wrapped(*args, **kwargs):
        args = list(args)
        args[index] = recurrence_to_lag(args[index], pad=pad)
        return lag_to_recurrence(function(*args, **kwargs))

    return wrapped
