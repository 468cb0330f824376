"""Impute, relevance table and selection for a feature matrix that already is a tensor: the other half of the tensor front door.

`extract_features_tensor` / `extract_rolled_features_tensor` leave the float64 feature matrix on the GPU; `calculate_relevance_table`
and `select_features` take a DataFrame and a Series.  Here the matrix stays where it is: `tsfa_impute` runs in place, the
statistics sweep of `tsfa_relevance_*` hands its per-column statistics to the tails kernels in HBM (`tsfa_relevance_tails_*`: Mann-
Whitney's normal tail, Fisher's exact tail, Kendall's asymptotic tail), the FDR step-up runs on the p-value array
(`tsfa_relevance_fdr`), and the selected columns are compacted and gathered on the device (`tsfa_compact_mask`,
`tsfa_gather_columns_device`).  What crosses PCIe is the target (n values in), one byte per column (the feature types, for the
constant-features warning and the number of tested hypotheses), the count of selected columns and their indices.

Two tails stay on the host by default and are evaluated by the functions the frame entry points use: the exact Mann-Whitney
distribution (a class or its complement with at most 8 rows, no ties) and every Kolmogorov-Smirnov tail
(`test_for_binary_target_real_feature="smir"`, binary features under a real target).  The kernels flag those cells
(`routes`), the statistics of the run come back only when such cells can occur, and the values are written into the device
array before the FDR step.

`ks_tail="device"` moves the exact Kolmogorov-Smirnov tail (samples of at most 10 000 rows) onto the GPU as well
(`csrc/rel_ks.h`, route `TSFA_ROUTE_KS_EXACT`): the same float64 expressions as `ks_2samp_pvalue`, equal bit for bit.  What is
left for the host then are the cells beyond 10 000 rows (scipy's `kstwo`), the rare exact value that rounding pushes outside
[0, 1] (`ks_2samp_pvalue` falls through to `kstwo` there, and so does this), and the exact Mann-Whitney cells; only the
triples of those cells are fetched.
"""
import warnings

import numpy as np

from tsfresh_amd import _native
from tsfresh_amd.tensor import _synchronize, _to_device


class RelevanceTensors:
    """The result of `calculate_relevance_tensor`: device tensors over the m columns and the T tables (T = number of labels for
    classification -- every label against the rest, also for two labels, as the reference does -- and 1 for regression).

    types [m] int8 (0 constant, 1 binary, 2 real); p_values [m, T] float64; relevant_per_table [m, T] bool; relevant [m] bool;
    n_significant [m] int32 (tables that reject the column); p_value [m] float64 (the smallest over the tables, NaN for a
    constant column); routes [m, T] uint8 (`_native.TSFA_ROUTE_*`: who evaluated the cell); labels: the ascending distinct
    values of y behind the tables (empty for regression); host_cells: how many cells the host evaluated; columns: the names
    given, or None."""

    __slots__ = ("types", "p_values", "relevant_per_table", "relevant", "n_significant", "p_value", "routes", "labels",
                 "host_cells", "columns", "ml_task")

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields[name])


def _matrix(torch, X, device):
    """X as a torch.float64 [n, m] tensor with contiguous rows on its HIP device -> (tensor, device ordinal)."""
    from tsfresh_amd.feature_extraction import extraction
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X))
    if not isinstance(X, torch.Tensor):
        raise TypeError("X must be a torch.Tensor or a numpy array, not {}".format(type(X).__name__))
    if X.ndim != 2:
        raise ValueError("X must be two-dimensional (rows x feature columns): got {} dimensions".format(X.ndim))
    if device is None:
        device = X.device.index if X.is_cuda else extraction._default_device()
    device = int(device)
    X = _to_device(X, device)
    if X.dtype != torch.float64:
        X = X.to(torch.float64)
    n, m = X.shape
    if m and not (X.stride(1) == 1 and (n <= 1 or X.stride(0) >= m)):
        X = X.contiguous()
    return X, device


def _ld(X):
    n, m = X.shape
    return int(X.stride(0)) if (n > 1 and m) else max(int(m), 1)


def _target(torch, y, n):
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError("y must be one-dimensional with one entry per row of X ({}): got shape {}".format(n, tuple(y.shape)))
    if y.dtype.kind not in "biuf":
        raise TypeError("y must be of integer, bool or floating dtype, not {}".format(y.dtype))
    return y


def impute_tensor(X):
    """`impute` in place on a tensor: per column +inf -> the largest finite value, -inf -> the smallest, NaN -> the median of the
    finite values (a column without a finite value counts as zeros), by `tsfa_impute`.

    :param X: `torch.float64` tensor `[n, m]` with contiguous rows (`stride(1) == 1`, `stride(0) >= m`: a row-strided view is
        fine), on the GPU (imputed where it is) or on the CPU (staged through the default device).  Anything else raises a
        `ValueError`: the call works in place, so nothing is converted or copied.
    :return: X."""
    import torch

    from tsfresh_amd.feature_extraction import extraction
    if not isinstance(X, torch.Tensor) or X.dtype != torch.float64 or X.ndim != 2:
        raise ValueError("impute_tensor needs a two-dimensional torch.float64 tensor (it works in place)")
    n, m = X.shape
    if n == 0 or m == 0:
        return X
    if X.stride(1) != 1 or (n > 1 and X.stride(0) < m):
        raise ValueError("impute_tensor needs contiguous rows (stride(1) == 1 and stride(0) >= the number of columns): "
                         "got strides {}".format(tuple(X.stride())))
    if X.is_cuda:
        _synchronize(torch, X.device.index)
        _native.impute_ptr(X.data_ptr(), n, m, _ld(X), _native.TSFA_DEVICE, X.device.index)
    else:
        _native.impute_ptr(X.data_ptr(), n, m, _ld(X), _native.TSFA_HOST, extraction._default_device())
    return X


def _relevance(torch, X, device, y, columns, ml_task, multiclass, n_significant, test_for_binary_target_real_feature, fdr_level,
               hypotheses_independent, check_nan, ks_tail="host"):
    from tsfresh_amd.feature_selection.significance_tests import ks_2samp_pvalue, mannwhitney_pvalue, target_tie_statistics
    if ks_tail not in ("host", "device"):
        raise ValueError("ks_tail must be 'host' or 'device', not {!r}".format(ks_tail))
    on_device = (ks_tail == "device")
    n, m = X.shape
    y = _target(torch, y, n)
    if columns is not None:
        columns = list(columns)
        if len(columns) != m:
            raise ValueError("columns must name the {} columns of X: got {} names".format(m, len(columns)))
    if len(np.unique(y)) < 2:
        raise ValueError("Feature selection is only possible if more than 1 label/class is provided")
    if ml_task not in ["auto", "classification", "regression"]:
        raise ValueError("ml_task must be one of: 'auto', 'classification', 'regression'")
    elif ml_task == "auto":
        ml_task = "regression" if y.dtype.kind == "f" else "classification"
    if multiclass:
        assert ml_task == "classification", "ml_task must be classification for multiclass problem"
        assert len(np.unique(y)) >= n_significant, "n_significant must not exceed the total number of classes"
        if len(np.unique(y)) <= 2:
            warnings.warn("Two or fewer classes, binary feature selection will be used (multiclass = False)")
            multiclass = False
    if ml_task == "classification" and test_for_binary_target_real_feature not in ("mann", "smir"):
        raise ValueError("Please use a valid entry for test_for_binary_target_real_feature. "
                         "Valid entries are 'mann' and 'smir'.")
    smir = (test_for_binary_target_real_feature == "smir")
    name = (lambda j: columns[j]) if columns is not None else (lambda j: j)
    if check_nan and m:
        bad = torch.isnan(X).any(dim=0)
        if bool(bad.any().item()):   # one word back
            raise ValueError("Feature {} contains NaN values".format(name(int(torch.nonzero(bad)[0].item()))))
    if y.dtype.kind == "f" and np.isnan(y).any():
        raise ValueError("Target contains NaN values")

    dev = X.device
    T = len(np.unique(y)) if ml_task == "classification" else 1
    p = torch.empty((m, T), dtype=torch.float64, device=dev)
    routes = torch.empty((m, T), dtype=torch.uint8, device=dev)
    types = torch.empty(m, dtype=torch.uint8, device=dev)
    rel_table = torch.zeros((m, T), dtype=torch.uint8, device=dev)
    relevant = torch.zeros(m, dtype=torch.uint8, device=dev)
    n_sig = torch.zeros(m, dtype=torch.int32, device=dev)
    p_min = torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
    _synchronize(torch, device)   # X's producer and the fills above are done before the library's null stream works on them

    host_cells, labels = 0, []
    if ml_task == "classification":
        labels = np.unique(y)
        codes = np.searchsorted(labels, y).astype(np.int32)
        class_n = np.bincount(codes, minlength=T)
        # the host routes can only occur under 'smir' or with a class (or its complement) of at most 8 rows: only then
        # are the statistics copied out
        if smir and on_device:
            # every real cell is a Kolmogorov-Smirnov cell (no exact Mann-Whitney under 'smir'); the distances stay in HBM and
            # of the cells left to the host only the triples are fetched
            ks_dev = torch.empty((m, T), dtype=torch.float64, device=dev)
            host_cells, _ = _native.relevance_tails_classes(X.data_ptr(), n, m, _ld(X), codes, T, p.data_ptr(), routes.data_ptr(),
                                                            types.data_ptr(), device=device, with_ks=True, want_stats=False,
                                                            ks_tail="device", ks_d_ptr=ks_dev.data_ptr())
            if host_cells:
                flat = torch.nonzero(routes.view(-1) == _native.TSFA_ROUTE_HOST_KS).view(-1)
                k, dist = (flat % T).cpu().numpy(), ks_dev.view(-1)[flat].cpu().numpy()
                vals = [ks_2samp_pvalue(class_n[k[q]], n - class_n[k[q]], dist[q]) for q in range(len(k))]
                p.view(-1)[flat] = torch.as_tensor(vals, dtype=torch.float64, device=dev)
        else:
            want_stats = smir or bool(((class_n <= 8) | (n - class_n <= 8)).any())
            host_cells, stats_ = _native.relevance_tails_classes(X.data_ptr(), n, m, _ld(X), codes, T, p.data_ptr(), routes.data_ptr(),
                                                                 types.data_ptr(), device=device, with_ks=smir, want_stats=want_stats)
            if host_cells:
                _, tie_term, rank_sums, _, ks_d = stats_
                r = routes.cpu().numpy()
                cells = np.argwhere((r == _native.TSFA_ROUTE_HOST_MWU_EXACT) | (r == _native.TSFA_ROUTE_HOST_KS))
                vals = [ks_2samp_pvalue(class_n[k], n - class_n[k], ks_d[j, k]) if r[j, k] == _native.TSFA_ROUTE_HOST_KS
                        else mannwhitney_pvalue(rank_sums[j, k], class_n[k], n - class_n[k], tie_term[j]) for j, k in cells]
                p.view(-1)[torch.as_tensor(cells[:, 0] * T + cells[:, 1], device=dev)] = torch.as_tensor(vals, dtype=torch.float64,
                                                                                                       device=dev)
        labels = labels.tolist()
    else:
        yv = y.astype(np.float64)
        if on_device:
            n_hi_dev = torch.empty(m, dtype=torch.int64, device=dev)
            ks_dev = torch.empty(m, dtype=torch.float64, device=dev)
            host_cells, _ = _native.relevance_tails_real(X.data_ptr(), n, m, _ld(X), yv, target_tie_statistics, p.data_ptr(),
                                                         routes.data_ptr(), types.data_ptr(), device=device, want_stats=False,
                                                         ks_tail="device", n_hi_ptr=n_hi_dev.data_ptr(), ks_d_ptr=ks_dev.data_ptr())
            if host_cells:   # only the triples of the cells that are left
                flat = torch.nonzero(routes.view(-1) == _native.TSFA_ROUTE_HOST_KS).view(-1)
                n_hi, dist = n_hi_dev[flat].cpu().numpy(), ks_dev[flat].cpu().numpy()
                vals = [ks_2samp_pvalue(n_hi[q], n - n_hi[q], dist[q]) for q in range(len(n_hi))]
                p.view(-1)[flat] = torch.as_tensor(vals, dtype=torch.float64, device=dev)
        else:
            host_cells, rec = _native.relevance_tails_real(X.data_ptr(), n, m, _ld(X), yv, target_tie_statistics, p.data_ptr(),
                                                           routes.data_ptr(), types.data_ptr(), device=device, want_stats=True)
            if host_cells:
                r = routes.cpu().numpy()[:, 0]
                cells = np.nonzero(r == _native.TSFA_ROUTE_HOST_KS)[0]
                vals = [ks_2samp_pvalue(rec["n_hi"][j], n - rec["n_hi"][j], rec["ks_d"][j]) for j in cells]
                p.view(-1)[torch.as_tensor(cells, device=dev)] = torch.as_tensor(vals, dtype=torch.float64, device=dev)

    types_host = types.cpu().numpy()   # one byte per column: the constant columns' names and the number of hypotheses
    constant = np.nonzero(types_host == 0)[0]
    if len(constant):
        warnings.warn("[test_feature_significance] Constant features: {}".format(", ".join(str(name(int(j))) for j in constant)),
                      RuntimeWarning)
    n_tested = m - len(constant)
    if n_tested:
        c_m = 1.0 if hypotheses_independent else float(np.sum(1.0 / np.arange(1, n_tested + 1)))
        _synchronize(torch, device)
        _native.relevance_fdr(p.data_ptr(), types.data_ptr(), m, T, fdr_level, c_m, n_significant, multiclass, rel_table.data_ptr(),
                              relevant.data_ptr(), n_sig.data_ptr(), p_min.data_ptr(), device=device)
        if not bool(relevant.any().item()):
            warnings.warn(
                "No feature was found relevant for {} for fdr level = {} (which corresponds to the maximal percentage "
                "of irrelevant features, consider using an higher fdr level or add other features.".format(ml_task, fdr_level),
                RuntimeWarning)
    return RelevanceTensors(types=types.view(torch.int8), p_values=p, relevant_per_table=rel_table.view(torch.bool),
                            relevant=relevant.view(torch.bool), n_significant=n_sig, p_value=p_min, routes=routes, labels=labels,
                            host_cells=int(host_cells), columns=columns, ml_task=ml_task)


def calculate_relevance_tensor(X, y, columns=None, ml_task="auto", multiclass=False, n_significant=1,
                               test_for_binary_target_real_feature="mann", fdr_level=0.05, hypotheses_independent=False,
                               device=None, check_nan=True, ks_tail="host"):
    """`calculate_relevance_table` for a feature matrix held as a tensor; every result stays on the GPU.

    :param X: `torch.float64` tensor `[n, m]`.  A CPU tensor or a numpy array is moved to `device` with torch; another dtype, or a
        layout whose rows are not contiguous, is converted or copied with torch (a row-strided view is used as it is).
    :param y: torch tensor (any device) or numpy array of n entries; it is copied to the host.  Integer or bool dtype means
        classification, floating dtype regression (`ml_task="auto"`); an explicit `ml_task` wins.  The labels of a classification
        are the ascending distinct values; more than 256 of them raise the native error.
    :param columns: optional m names, used in the warnings and the `ValueError` of a NaN column.
    :param ml_task, multiclass, n_significant, test_for_binary_target_real_feature, fdr_level, hypotheses_independent: as in
        `calculate_relevance_table`, with its `ValueError`s, assertions and warnings (constant features, no relevant feature,
        the multiclass fall-back at two or fewer classes).  A target with fewer than two distinct values raises
        `ValueError("Feature selection is only possible if more than 1 label/class is provided")`.
    :param device: HIP device ordinal.  Default: the device X lives on, else the rule of `extract_features`.
    :param check_nan: True (default): a NaN in X raises `ValueError("Feature <name> contains NaN values")` for the first such
        column; False skips the check and its read-back of one word.
    :param ks_tail: who evaluates the exact Kolmogorov-Smirnov tails ("smir"; binary features under a real target).  "host"
        (default): `ks_2samp_pvalue`, one cell at a time.  "device": the GPU, for samples of at most 10 000 rows, with equal
        p-values (`routes` then shows `TSFA_ROUTE_KS_EXACT`, and `host_cells` counts what is left to the host).  Anything else
        raises `ValueError`.
    :return: a `RelevanceTensors`.

    Synchronous, like `extract_features_tensor`: X is read after everything queued on torch's current stream has finished."""
    import torch
    X, device = _matrix(torch, X, device)
    return _relevance(torch, X, device, y, columns, ml_task, multiclass, n_significant, test_for_binary_target_real_feature,
                      fdr_level, hypotheses_independent, check_nan, ks_tail)


def select_features_tensor(X, y, columns=None, ml_task="auto", multiclass=False, n_significant=1,
                           test_for_binary_target_real_feature="mann", fdr_level=0.05, hypotheses_independent=False, device=None,
                           check_nan=True, ks_tail="host"):
    """`select_features` for a feature matrix held as a tensor: the relevant columns, gathered on the GPU.

    Parameters as in `calculate_relevance_tensor`.

    :return: `(X_selected, selected_columns, indices)`: `X_selected` a new `torch.float64` device tensor `[n, k]` holding the
        relevant columns of X; `selected_columns` their names when `columns` was given, else their indices as a list;
        `indices` an int32 device tensor `[k]`.  The columns come in ASCENDING COLUMN INDEX.  (`select_features` orders them by
        the p-value sort of its table, which is not determined among equal p-values; the set is the same.)  With no relevant
        column `X_selected` is `[n, 0]` and the reference's warning is given."""
    import torch
    X, device = _matrix(torch, X, device)
    res = _relevance(torch, X, device, y, columns, ml_task, multiclass, n_significant, test_for_binary_target_real_feature,
                     fdr_level, hypotheses_independent, check_nan, ks_tail)
    n, m = X.shape
    indices = torch.empty(m, dtype=torch.int32, device=X.device)
    _synchronize(torch, device)
    k = _native.compact_mask(res.relevant.data_ptr(), m, indices.data_ptr(), device=device)   # the count comes back
    indices = indices[:k]
    out = torch.empty((n, k), dtype=torch.float64, device=X.device)
    if n and k:
        _synchronize(torch, device)
        _native.gather_columns_device(X.data_ptr(), n, _ld(X), indices.data_ptr(), k, out.data_ptr(), k, device=device)
    picked = indices.tolist()
    return out, ([res.columns[j] for j in picked] if res.columns is not None else picked), indices


def extract_relevant_features_tensor(x, y, lengths=None, kinds=None, channels_last=False, default_fc_parameters=None,
                                     kind_to_fc_parameters=None, ml_task="auto", multiclass=False, n_significant=1,
                                     test_for_binary_target_real_feature="mann", fdr_level=0.05, hypotheses_independent=False,
                                     device=None, check_nan=True, ks_tail="host", nan_policy="raise", times=None, time_unit="ns"):
    """`extract_relevant_features` for a batch held as a tensor: `extract_features_tensor`, `impute_tensor` and
    `select_features_tensor` on one matrix that never leaves the GPU.

    :param x, lengths, kinds, channels_last, default_fc_parameters, kind_to_fc_parameters, device, check_nan: as in
        `extract_features_tensor` (check_nan is about the samples; the imputed matrix holds no NaN).
    :param y: one target value per series, as in `calculate_relevance_tensor`; the selection options (`ks_tail` among them)
        likewise.
    :param times, time_unit: as in `extract_features_tensor`: the batch's clock, which adds the `linear_trend_timewise`
        columns to the matrix the selection runs on.
    :param nan_policy: as in `extract_features_tensor`: "drop" extracts from the steps the wide frame keeps after
        `dropna()`; `y` stays one value per series.  Not offered here either: a validity mask, per-kind lengths, the frame
        entries, an enqueue-only mode.
    :return: `(features, columns)`: the relevant columns `[B, k]` on the device, in ascending column index of the extracted
        matrix, and their names."""
    from tsfresh_amd.tensor import extract_features_tensor
    if ks_tail not in ("host", "device"):   # before the extraction runs
        raise ValueError("ks_tail must be 'host' or 'device', not {!r}".format(ks_tail))
    features, columns = extract_features_tensor(x, lengths=lengths, kinds=kinds, channels_last=channels_last,
                                                default_fc_parameters=default_fc_parameters,
                                                kind_to_fc_parameters=kind_to_fc_parameters, device=device, check_nan=check_nan,
                                                nan_policy=nan_policy, times=times, time_unit=time_unit)
    impute_tensor(features)
    selected, names, _ = select_features_tensor(features, y, columns=columns, ml_task=ml_task, multiclass=multiclass,
                                                n_significant=n_significant,
                                                test_for_binary_target_real_feature=test_for_binary_target_real_feature,
                                                fdr_level=fdr_level, hypotheses_independent=hypotheses_independent,
                                                device=features.device.index, check_nan=False, ks_tail=ks_tail)
    return selected, names
