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

__all__ = ["cross_similarity", "recurrence_matrix"]

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
