"""Device-side verification of an ensemble against an observation (csrc/ensemble_score.hip): the accumulators
and the per-batch call shared by ``Model.score_ensemble`` (members produced on the device) and ``metrics.ensemble_scores`` (members
the caller already has on the host)."""
import ctypes

import numpy as np

from . import _lib
from ._exact import finite_float32, int_ratio, quotient, ratio_exact, wide
from .device import DeviceArray

U64 = 0xFFFFFFFFFFFFFFFF


def check_score_args(fair, scale=None, sample_shape=None):
    """``fair`` must be a bool; ``scale`` None or something that broadcasts to one sample -> float32 array of ``sample_shape`` (or
    None).  Looks at its arguments only (no library, no device)."""
    if not isinstance(fair, (bool, np.bool_)):
        raise ValueError(f'`fair` must be True or False, got {fair!r}')
    if scale is None or sample_shape is None:
        return None
    try:
        s = np.broadcast_to(np.asarray(scale, np.float64), tuple(sample_shape))
    except ValueError:
        raise ValueError(f'`scale` of shape {np.shape(scale)} does not broadcast to one sample {tuple(sample_shape)}') from None
    return np.ascontiguousarray(s, np.float32)


def as_signed64(v):
    v = int(v) & U64
    return v - (1 << 64) if v >> 63 else v


class _Accumulators:
    """What the scorers of one verification run share: ``score`` is called once per batch of whole samples while the batch's
    member stack is resident (the library call of the subclass, then the download of the batch's per-sample sums and, with
    ``return_fields``, of its fields: ``_launch`` and ``_download_fields``); ``result`` downloads the run's sums and derives the
    scores on the host; ``free`` releases the device buffers, all of which live in ``dev``.
    ``sums``, ``dtype``: the shape and type of one sample's sums."""

    def __init__(self, n_members, n_samples, sample_shape, return_fields, bmax, sums, dtype):
        self.lib = _lib.lib()
        self.K, self.N, self.sample_shape = int(n_members), int(n_samples), tuple(sample_shape)
        self.per = int(np.prod(self.sample_shape, dtype=np.int64))
        self.return_fields = bool(return_fields)
        self.bmax = int(bmax)
        self.dev = dict(sample=DeviceArray((self.bmax,) + sums, dtype))
        self.sample_sums = np.zeros((self.N,) + sums, dtype)

    def score(self, stack_ptr, stride, obs_ptr, first, b):
        """samples [first, first + b) of the run: their members at stack_ptr (member stride ``stride`` elements), their observation at
        obs_ptr"""
        self._launch(stack_ptr, stride, obs_ptr, first, b)
        self.dev['sample'].download(self.sample_sums[first:first + b])
        if self.return_fields:
            self._download_fields(first, b)

    def free(self):
        for a in self.dev.values():
            a.free()
        self.dev = {}


class Scorer(_Accumulators):
    """Accumulators of the CRPS / rank-histogram / spread-skill verification on the device (csrc/ensemble_score.hip); ``result``
    takes the means in float64."""

    def __init__(self, n_members, n_samples, sample_shape, q32, fair, seed, scale, return_fields, bmax):
        super().__init__(n_members, n_samples, sample_shape, return_fields, bmax, (4,), np.float64)
        self.q = np.asarray(q32, np.float32)
        self.nq = len(self.q)
        self.qc = (ctypes.c_float * max(self.nq, 1))(*self.q.tolist())
        self.fair, self.seed = int(bool(fair)), as_signed64(0 if seed is None else seed)
        self.n_cells_excluded = 0
        self.dev.update(cell=DeviceArray.zeros((4, self.per), np.float64), hist=DeviceArray.zeros((self.K + 1,), np.uint64),
                        cov=DeviceArray.zeros((max(self.nq, 1),), np.uint64))
        if scale is not None:
            scale = np.ascontiguousarray(scale, np.float32).reshape(self.per)
            with np.errstate(invalid='ignore'):
                self.n_cells_excluded = int(np.count_nonzero(~(np.isfinite(scale) & (scale > 0))))
            self.dev['scale'] = DeviceArray.from_numpy(scale)
        self.fields = {}
        if self.return_fields:
            for k in ('crps', 'sqerr', 'var', 'rank'):
                self.dev[k] = DeviceArray((self.bmax * self.per,), np.int32 if k == 'rank' else np.float32)
                self.fields[k + '_field'] = np.empty((self.N,) + self.sample_shape, self.dev[k].dtype)

    def _launch(self, stack_ptr, stride, obs_ptr, first, b):
        d = self.dev
        ptr = lambda k: d[k].ptr if k in d else None                                       # noqa: E731
        _lib.check(self.lib.dl4ds_ensemble_score(stack_ptr, self.K, b * self.per, stride, obs_ptr, b, first * self.per, ptr('scale'),
                                                 self.fair, self.seed, self.qc, self.nq, ptr('crps'), ptr('sqerr'), ptr('var'),
                                                 ptr('rank'), d['sample'].ptr, d['cell'].ptr, d['hist'].ptr, d['cov'].ptr))

    def _download_fields(self, first, b):
        for k in ('crps', 'sqerr', 'var', 'rank'):
            self.dev[k].download(self.fields[k + '_field'][first:first + b])

    def result(self):
        cell = self.dev['cell'].numpy()
        hist = self.dev['hist'].numpy().astype(np.int64)
        covered = self.dev['cov'].numpy()[:self.nq].astype(np.int64)
        s = self.sample_sums
        n_valid = int(round(s[:, 3].sum()))
        tot = s[:, :3].sum(axis=0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = tot / n_valid if n_valid else np.full(3, np.nan)
            res = dict(crps=float(mean[0]), spread=float(np.sqrt(mean[2])), rmse=float(np.sqrt(mean[1])))
            res['spread_skill'] = float(np.float64(res['spread']) / np.float64(res['rmse']))
            per_sample = np.where(s[:, 3:4] > 0, s[:, :3] / s[:, 3:4], np.nan)
            res.update(crps_per_sample=per_sample[:, 0], spread_per_sample=np.sqrt(per_sample[:, 2]),
                       rmse_per_sample=np.sqrt(per_sample[:, 1]))
            maps = np.where(cell[3] > 0, cell[:3] / cell[3], np.nan).reshape((3,) + self.sample_shape)
            res.update(crps_map=maps[0], spread_map=np.sqrt(maps[2]), rmse_map=np.sqrt(maps[1]))
            res.update(rank_histogram=hist, covered=covered,
                       coverage=covered / np.float64(n_valid) if n_valid else np.full(self.nq, np.nan),
                       n_valid=n_valid, n_valid_per_sample=np.rint(s[:, 3]).astype(np.int64),
                       n_valid_map=np.rint(cell[3]).astype(np.int64).reshape(self.sample_shape),
                       sample_sums=s.copy(), cell_sums=cell.reshape((4,) + self.sample_shape),
                       n_cells_excluded=self.n_cells_excluded)
        res.update(self.fields)
        return res


# ------------------------------------------------------------------------------------------------ exceedance probabilities
EXCEEDANCE_MAX_THRESHOLDS = 16                     # cap of dl4ds_ensemble_exceedance: thresholds and counters live in registers


def check_exceedance_args(thresholds, sample_shape):
    """Thresholds of the exceedance verification -> float32 array shaped (T,) (one value per threshold) or (T,) + sample_shape (a
    threshold field per cell; NaN inside a field is legal and excludes that cell for that threshold).  Refuses an empty sequence,
    more than 16 thresholds, anything that is not numeric, a scalar threshold that is not finite (as float32), and fields that do
    not have one sample's shape (``sample_shape=None``: the shape of fields is not looked at; for a caller that does not know the
    sample's shape yet).  Looks at its arguments only (no library, no device)."""
    sample_shape = None if sample_shape is None else tuple(int(v) for v in sample_shape)
    try:
        t64 = np.asarray(getattr(thresholds, 'values', thresholds))
        if t64.dtype == bool or t64.dtype == object or not np.issubdtype(t64.dtype, np.number) or np.iscomplexobj(t64):
            raise TypeError
        t64 = t64.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'`thresholds` must be numbers, or one field of numbers per threshold, got {thresholds!r}') from None
    if t64.ndim == 0:
        t64 = t64.reshape(1)
    if t64.shape[0] == 0:
        raise ValueError('`thresholds` must not be empty')
    if t64.shape[0] > EXCEEDANCE_MAX_THRESHOLDS:
        raise ValueError(f'at most {EXCEEDANCE_MAX_THRESHOLDS} thresholds per call, got {t64.shape[0]}')
    if t64.ndim == 1:
        return finite_float32(t64, 'scalar `thresholds`')
    if sample_shape is not None and tuple(t64.shape[1:]) != sample_shape:
        raise ValueError(f'per-cell `thresholds` must be shaped (T,) + {sample_shape}, one field per threshold, got {t64.shape}')
    with np.errstate(over='ignore'):
        return np.ascontiguousarray(t64, np.float32)


def exceedance_from_counts(table, cell_sums, sample_sums, n_members, thresholds):
    """The result dict of the exceedance verification from the integer outputs of ``dl4ds_ensemble_exceedance`` (host arithmetic
    only, no library): ``table`` (T, K + 1, 2), ``cell_sums`` (T, 4) + sample_shape, ``sample_sums`` (N, T, 4).  Every quotient of
    integers is evaluated on Python integers (or on fp64 operands that hold them exactly) and rounded once; a quotient with a zero
    denominator is NaN."""
    from fractions import Fraction
    K = int(n_members)
    table = np.asarray(table).astype(np.int64)
    cell = np.asarray(cell_sums).astype(np.int64)
    samp = np.asarray(sample_sums).astype(np.int64)
    T = table.shape[0]
    if table.shape != (T, K + 1, 2) or cell.shape[:2] != (T, 4) or samp.ndim != 3 or samp.shape[1:] != (T, 4):
        raise ValueError(f'expected table (T, {K + 1}, 2), cell_sums (T, 4, ...) and sample_sums (N, T, 4), got {table.shape}, '
                         f'{cell.shape}, {samp.shape}')
    res = dict(thresholds=np.asarray(thresholds, np.float32), n_members=K, table=table)
    nan = float('nan')
    keys = ('base_rate', 'brier', 'brier_fair', 'reliability', 'resolution', 'uncertainty', 'bss', 'roc_auc')
    out = {k: np.full(T, nan) for k in keys}
    n_valid, n_events = np.zeros(T, np.int64), np.zeros(T, np.int64)
    obs_freq, fc_count = np.full((T, K + 1), nan), np.zeros((T, K + 1), np.int64)
    pod, pofd = np.full((T, K + 2), nan), np.full((T, K + 2), nan)
    ratio = int_ratio                                           # (Python integers: correctly rounded)
    for t in range(T):
        m = [int(v) for v in table[t, :, 0]]                    # non-events with c = i
        a = [int(v) for v in table[t, :, 1]]                    # events with c = i
        ni = [x + y for x, y in zip(m, a)]
        n, N1 = sum(ni), sum(a)
        N0 = n - N1
        n_valid[t], n_events[t] = n, N1
        fc_count[t] = ni
        obs_freq[t] = [ratio(a[i], ni[i]) for i in range(K + 1)]
        num = sum(i * i * m[i] + (K - i) * (K - i) * a[i] for i in range(K + 1))
        out['base_rate'][t] = ratio(N1, n)
        out['brier'][t] = ratio(num, K * K * n)
        out['brier_fair'][t] = ratio((K - 1) * num - sum(ni[i] * i * (K - i) for i in range(K + 1)), K * K * (K - 1) * n)
        out['uncertainty'][t] = ratio(N1 * N0, n * n)
        out['bss'][t] = ratio(K * K * N1 * N0 - num * n, K * K * N1 * N0)
        if n:
            # n_i (i/K - a_i/n_i)^2 = (i n_i - K a_i)^2 / (K^2 n_i);  n_i (a_i/n_i - N1/n)^2 = (a_i n - N1 n_i)^2 / (n_i n^2)
            rel = sum((Fraction((i * ni[i] - K * a[i]) ** 2, ni[i]) for i in range(K + 1) if ni[i]), Fraction(0))
            rsl = sum((Fraction((a[i] * n - N1 * ni[i]) ** 2, ni[i]) for i in range(K + 1) if ni[i]), Fraction(0))
            out['reliability'][t] = float(rel / (K * K * n))
            out['resolution'][t] = float(rsl / (n * n * n))
        below, twice = 0, 0                                     # twice = 2 sum_i a_i (sum_{i' < i} m_i' + m_i / 2)
        for i in range(K + 1):
            twice += a[i] * (2 * below + m[i])
            below += m[i]
        out['roc_auc'][t] = ratio(twice, 2 * N1 * N0)
        hit = fa = 0
        pod[t, 0], pofd[t, 0] = ratio(0, N1), ratio(0, N0)
        for j in range(1, K + 2):                               # point j: warn iff c >= K + 1 - j
            hit += a[K + 1 - j]
            fa += m[K + 1 - j]
            pod[t, j], pofd[t, j] = ratio(hit, N1), ratio(fa, N0)
    res.update(n_valid=n_valid, n_events=n_events, **out)
    res.update(forecast_probability=ratio_exact(np.arange(K + 1).astype(object), np.full(K + 1, K, object)),
               observed_frequency=obs_freq, forecast_count=fc_count, roc_pod=pod, roc_pofd=pofd)
    # per sample and per cell: n_valid, sum o, sum c, sum (c - K o)^2
    snv = wide(samp[..., 0], K * K * (int(samp[..., 0].max()) if samp.size else 0))
    res.update(sample_sums=samp, n_valid_per_sample=samp[..., 0].copy(), brier_per_sample=quotient(samp[..., 3], K * K * snv))
    top = int(cell[:, 0].max()) if cell.size else 0             # valid samples of the fullest cell
    nv, so, sc, sq = (wide(cell[:, i], K * K * top * top * max(top, 1)) for i in range(4))
    unc = K * K * so * (nv - so)
    res.update(cell_sums=cell, n_valid_map=cell[:, 0].copy(), brier_map=quotient(sq, K * K * nv), base_rate_map=quotient(so, nv),
               forecast_rate_map=quotient(sc, K * nv), bss_map=quotient(unc - sq * nv, unc))
    return res


class ExceedanceScorer(_Accumulators):
    """The counterpart of ``Scorer`` for exceedance probabilities (csrc/exceedance.hip): the integer
    accumulators of one run on the device; ``result`` derives the scores on the host (``exceedance_from_counts``).  ``thr32``: what
    ``check_exceedance_args`` returned."""

    def __init__(self, n_members, n_samples, sample_shape, thr32, return_fields, bmax):
        self.thr = np.ascontiguousarray(thr32, np.float32)
        self.T = int(self.thr.shape[0])
        self.per_cell = int(self.thr.ndim > 1)
        super().__init__(n_members, n_samples, sample_shape, return_fields, bmax, (self.T, 4), np.int64)
        self.dev.update(thr=DeviceArray.from_numpy(self.thr.reshape(-1)), cell=DeviceArray.zeros((self.T, 4, self.per), np.int64),
                        table=DeviceArray.zeros((self.T, self.K + 1, 2), np.uint64))
        self.count_field = None
        if self.return_fields:
            self.dev['count'] = DeviceArray((self.T * self.bmax * self.per,), np.int16)
            self.count_field = np.empty((self.N, self.T) + self.sample_shape, np.int16)

    def _launch(self, stack_ptr, stride, obs_ptr, first, b):
        d = self.dev
        _lib.check(self.lib.dl4ds_ensemble_exceedance(stack_ptr, self.K, b * self.per, stride, obs_ptr, b, d['thr'].ptr, self.T,
                                                      self.per_cell, d['count'].ptr if self.return_fields else None,
                                                      d['sample'].ptr, d['cell'].ptr, d['table'].ptr))

    def _download_fields(self, first, b):
        part = np.empty((self.T, b, self.per), np.int16)                                   # the entry's layout: [T][n]
        self.dev['count'].download(part)
        self.count_field[first:first + b] = part.transpose(1, 0, 2).reshape((b, self.T) + self.sample_shape)

    def result(self):
        cell = self.dev['cell'].numpy().reshape((self.T, 4) + self.sample_shape)
        res = exceedance_from_counts(self.dev['table'].numpy(), cell, self.sample_sums, self.K, self.thr)
        if self.return_fields:
            c = self.count_field
            res['count_field'] = c
            res['probability_field'] = np.where(c >= 0, c.astype(np.float32) / np.float32(self.K), np.float32(np.nan))
        return res


# ------------------------------------------------------------------------------------------------ neighbourhood probabilities
NEIGHBOURHOOD_MAX_MEMBERS = 256                    # caps of dl4ds_ensemble_fss
NEIGHBOURHOOD_MAX_THRESHOLDS = 16
NEIGHBOURHOOD_DEFAULT_WINDOWS = (1, 3, 5, 9, 17, 33, 65)       # metrics.FSS_DEFAULT_WINDOWS
NEIGHBOURHOOD_SUM_BOUND = 1 << 62                  # H*W*(K*m)^2 must stay below it: the 64-bit sums of dl4ds_ensemble_fss are exact


def largest_neighbourhood_window(n_members, h, w):
    """The largest window size n whose sums stay exact: H*W*(K*m)^2 < 2^62 with m = min(n, H)*min(n, W); None when every window
    is legal (the whole field is).  Window 1 always is: H*W < 2^31 and K <= 256."""
    K, h, w = int(n_members), int(h), int(w)
    legal = lambda n: h * w * (K * min(n, h) * min(n, w)) ** 2 < NEIGHBOURHOOD_SUM_BOUND           # noqa: E731
    if legal(max(h, w)):
        return None
    lo, hi = 1, max(h, w)                                       # legal(lo), not legal(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if legal(mid) else (lo, mid)
    return lo


def check_neighbourhood_ensemble_args(sample_shape, n_members, thresholds, windows):
    """Validation of the neighbourhood verification of an ensemble (no library call) -> (thresholds as float32 (T,), windows as
    int32 (S,)): ``metrics.check_neighbourhood_args`` (finite, strictly increasing thresholds; positive, strictly increasing
    integer windows; H*W < 2^31) plus what the ensemble adds: 1 ... 256 members, at most 16 thresholds, a sample shaped (H, W, C)
    and the overflow rule with the members in it, H*W*(K*m)^2 < 2^62 for m = min(n, H)*min(n, W).  ``sample_shape=None``: the
    shape is not looked at (for a caller that does not know it yet)."""
    from .metrics import check_neighbourhood_args
    K = int(n_members)
    if not 1 <= K <= NEIGHBOURHOOD_MAX_MEMBERS:
        raise ValueError(f'`n_members` must be in [1, {NEIGHBOURHOOD_MAX_MEMBERS}], got {n_members}')
    if sample_shape is None:
        shape = (1, 1, 1)
    else:
        shape = tuple(int(v) for v in sample_shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f'one sample must be shaped (H, W, C), got {shape}')
    h, w, _ = shape
    if sample_shape is not None and h * w < 1 << 31:
        top = largest_neighbourhood_window(K, h, w)
        for n in np.atleast_1d(np.asarray(windows)).ravel().tolist() if top is not None else ():
            if isinstance(n, int) and not isinstance(n, bool) and n > top:
                m = min(n, h) * min(n, w)
                raise ValueError(f'window {n} on a {h} x {w} field with {K} members: H*W*(K*m)^2 = {h * w * (K * m) ** 2} with '
                                 f'm = min(n, H)*min(n, W) = {m} must stay below 2^62 for the exact 64-bit sums; the largest '
                                 f'legal window for K = {K}, H = {h}, W = {w} is {top}')
    thr, win = check_neighbourhood_args((1,) + shape, thresholds, windows)
    if len(thr) > NEIGHBOURHOOD_MAX_THRESHOLDS:
        raise ValueError(f'at most {NEIGHBOURHOOD_MAX_THRESHOLDS} thresholds per call, got {len(thr)}')
    return thr, win


def neighbourhood_from_sums(sums, cont, nvalid, n_members, thresholds, windows):
    """The result dict of the neighbourhood verification of an ensemble from the integer outputs of ``dl4ds_ensemble_fss`` (host
    arithmetic only, no library): ``sums`` (N, C, T, S, 5) = D, F, O, Fv, X, ``cont`` (N, C, T, 2) = E, Cs, ``nvalid`` (N, C).
    Every score is a quotient of Python integers rounded to fp64 once (``pfss`` is 1 minus such a quotient), NaN on a zero
    denominator; n^4 of a large window and sums pooled beyond int64 are harmless."""
    K = int(n_members)
    sums, cont, nvalid = np.asarray(sums).astype(np.int64), np.asarray(cont).astype(np.int64), np.asarray(nvalid).astype(np.int64)
    win = np.asarray(windows).astype(np.int64).reshape(-1)
    N, C = nvalid.shape
    T, S = cont.shape[2], len(win)
    if sums.shape != (N, C, T, S, 5) or cont.shape != (N, C, T, 2):
        raise ValueError(f'expected sums (N, C, T, {S}, 5), cont (N, C, T, 2) and nvalid (N, C), got {sums.shape}, {cont.shape}, '
                         f'{nvalid.shape}')
    so = sums.astype(object)
    D, F, O, Fv, X = (so[..., q] for q in range(5))
    E, Cs, nv = cont[..., 0].astype(object), cont[..., 1].astype(object), nvalid.astype(object)
    n2 = np.asarray([int(n) ** 2 for n in win], object)        # the REQUESTED n, also where the kernel clamps the window
    kn = K * K * n2 * n2                                        # K^2 n^4, (S,)
    num = Fv - 2 * K * n2 * X + kn * E[..., None]               # K^2 n^4 n_valid times the neighbourhood Brier score
    den = np.broadcast_to(kn * nv[..., None, None], num.shape)
    pool = lambda a: np.sum(a, axis=(0, 1))                     # noqa: E731  (Python integers: cannot overflow)
    pE, pCs, pn = pool(E), pool(Cs), int(pool(nv))
    res = dict(sums=sums, events=cont[..., 0].copy(), member_events=cont[..., 1].copy(), n_valid=nvalid, n_members=K,
               thresholds=np.asarray(thresholds, np.float32), windows=win)
    res['pfss'] = 1.0 - ratio_exact(D, F + K * K * O)
    res['pfss_pooled'] = 1.0 - ratio_exact(pool(D), pool(F + K * K * O))
    res['nbs'] = ratio_exact(num, den)
    pnum, pden = pool(num), pool(den)
    res['nbs_pooled'] = ratio_exact(pnum, pden)
    unc = kn * (pE * (pn - pE))[:, None]                        # K^2 n^4 n_valid^2 f_o (1 - f_o)
    res['nbss_pooled'] = ratio_exact(unc - pnum * pn, unc)
    base = ratio_exact(pE, np.full(pE.shape, pn, object))
    res.update(base_rate=base, forecast_rate=ratio_exact(pCs, np.full(pCs.shape, K * pn, object)), fss_random=base.copy(),
               fss_useful=0.5 + base / 2.0)
    with np.errstate(invalid='ignore'):
        reach = res['pfss_pooled'] >= res['fss_useful'][:, None]          # NaN compares false
    res['useful_window'] = np.where(reach.any(1), win[np.argmax(reach, 1)], -1).astype(np.int64)
    return res


class NeighbourhoodScorer(_Accumulators):
    """The counterpart of ``Scorer`` for neighbourhood probabilities (csrc/ensemble_fss.hip): per batch
    the entry writes the per-field integer sums, which come back with the batch; ``result`` derives the scores on the host
    (``neighbourhood_from_sums``).  ``thr32``, ``win32``: what ``check_neighbourhood_ensemble_args`` returned.  There are no
    per-element fields to return."""

    def __init__(self, n_members, n_samples, sample_shape, thr32, win32, bmax):
        self.thr = np.ascontiguousarray(thr32, np.float32)
        self.win = np.ascontiguousarray(win32, np.int32)
        self.T, self.S = len(self.thr), len(self.win)
        self.H, self.W, self.C = (int(v) for v in sample_shape)
        super().__init__(n_members, n_samples, sample_shape, False, bmax, (self.C, self.T, self.S, 5), np.int64)
        self.dev.update(cont=DeviceArray((self.bmax, self.C, self.T, 2), np.int64), valid=DeviceArray((self.bmax, self.C), np.int64))
        self.cont = np.zeros((self.N, self.C, self.T, 2), np.int64)
        self.valid = np.zeros((self.N, self.C), np.int64)

    def _launch(self, stack_ptr, stride, obs_ptr, first, b):
        d = self.dev
        _lib.check(self.lib.dl4ds_ensemble_fss(stack_ptr, self.K, b * self.per, stride, obs_ptr, b, self.H, self.W, self.C,
                                               self.thr.ctypes.data, self.T, self.win.ctypes.data, self.S, d['sample'].ptr,
                                               d['cont'].ptr, d['valid'].ptr))
        d['cont'].download(self.cont[first:first + b])
        d['valid'].download(self.valid[first:first + b])

    def result(self):
        return neighbourhood_from_sums(self.sample_sums, self.cont, self.valid, self.K, self.thr, self.win)


# ------------------------------------------------------------------------------------------------ energy and variogram scores
MULTIVARIATE_MIN_MEMBERS, MULTIVARIATE_MAX_MEMBERS = 2, 128       # caps of dl4ds_ensemble_energy / dl4ds_ensemble_variogram
MULTIVARIATE_MAX_LAG = 8
VARIOGRAM_ORDERS = {0.5: 0, 1.0: 1, 2.0: 2}                       # order -> the entry's order code


def check_multivariate_args(max_lag, order, lag_weights, fair, weights, sample_shape, n_members=None):
    """Arguments of the multivariate verification -> (max_lag as int, the entry's order code, weights as a float32 array of
    ``sample_shape`` or None).  ``max_lag``: an integer in 1 ... 8; ``order``: 0.5, 1 or 2; ``lag_weights``: 'inverse' or
    'uniform'; ``fair``: a bool; ``weights``: None or finite numbers >= 0 that broadcast to one sample (what
    ``losses.latitude_weights`` returns does); ``sample_shape``: (H, W, C) or (T, H, W, C), or None: the shape of ``weights`` is
    not looked at (for a caller that does not know the sample's shape yet); ``n_members``: None or 2 ... 128.  Looks at its
    arguments only (no library, no device)."""
    if isinstance(max_lag, (bool, np.bool_)) or not isinstance(max_lag, (int, np.integer)) or not 1 <= max_lag <= MULTIVARIATE_MAX_LAG:
        raise ValueError(f'`max_lag` must be an integer in 1 ... {MULTIVARIATE_MAX_LAG}, got {max_lag!r}')
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, float, np.integer, np.floating)) \
            or float(order) not in VARIOGRAM_ORDERS:
        raise ValueError(f'`order` must be 0.5, 1 or 2, got {order!r}')
    if not isinstance(lag_weights, str) or lag_weights not in ('inverse', 'uniform'):
        raise ValueError(f"`lag_weights` must be 'inverse' or 'uniform', got {lag_weights!r}")
    if not isinstance(fair, (bool, np.bool_)):
        raise ValueError(f'`fair` must be True or False, got {fair!r}')
    if n_members is not None and not MULTIVARIATE_MIN_MEMBERS <= int(n_members) <= MULTIVARIATE_MAX_MEMBERS:
        raise ValueError(f'the energy and variogram scores take {MULTIVARIATE_MIN_MEMBERS} ... {MULTIVARIATE_MAX_MEMBERS} members, '
                         f'got {n_members}')
    if sample_shape is not None:
        sample_shape = tuple(int(v) for v in sample_shape)
        if len(sample_shape) not in (3, 4) or min(sample_shape) < 1:
            raise ValueError(f'one sample must be shaped (H, W, C) or (T, H, W, C), got {sample_shape}')
    w32 = None
    if weights is not None:
        try:
            w = np.asarray(getattr(weights, 'values', weights))
            if w.dtype == bool or w.dtype == object or not np.issubdtype(w.dtype, np.number) or np.iscomplexobj(w):
                raise TypeError
            w = w.astype(np.float64)
        except (TypeError, ValueError):
            raise ValueError(f'`weights` must be numbers, got {weights!r}') from None
        with np.errstate(over='ignore'):
            w32 = w.astype(np.float32)
        if not np.isfinite(w32).all() or (w32 < 0).any():
            raise ValueError('`weights` must be finite (as float32) and >= 0')
        if sample_shape is not None:
            try:                                                # (an (H, W) map, as `latitude_weights` makes it, gets the channel axis)
                w32 = np.ascontiguousarray(np.broadcast_to(w32[..., None] if w32.ndim == 2 else w32, sample_shape))
            except ValueError:
                raise ValueError(f'`weights` of shape {w.shape} do not broadcast to one sample {sample_shape}') from None
    return int(max_lag), VARIOGRAM_ORDERS[float(order)], w32


def variogram_lags(max_lag):
    """The lag list of ``dl4ds_variogram_lags`` (the library's own, so host and device cannot disagree; no device needed) ->
    int array (L, 2) of (dy, dx)."""
    lib = _lib.load()
    out, count = (ctypes.c_int * (2 * 98))(), ctypes.c_int(0)
    _lib.check(lib.dl4ds_variogram_lags(int(max_lag), out, ctypes.byref(count)))
    return np.asarray(out[:2 * count.value], np.int64).reshape(count.value, 2)


def multivariate_from_sums(dist, nvalid, npairs, sums, K, lags, lag_weights, fair):
    """The result dict of the multivariate verification from the outputs of ``dl4ds_ensemble_energy`` and
    ``dl4ds_ensemble_variogram`` (host arithmetic only, no library): ``dist`` (N, K (K + 1) / 2) fp64 (D_k, then G_kj over k < j),
    ``nvalid`` (N,), ``npairs`` (N, L), ``sums`` (N, L, 3) (sum (o - e)^2, sum o, sum e), ``lags`` (L, 2).  Sums over members,
    pairs, lags and samples go through ``math.fsum`` (samples in their order); a quotient with a zero denominator is NaN, and a
    sample without a valid element has the energy score NaN and takes no part in the mean."""
    import math
    K = int(K)
    dist = np.asarray(dist, np.float64)
    nvalid = np.asarray(nvalid).astype(np.int64)
    npairs = np.asarray(npairs).astype(np.int64)
    sums = np.asarray(sums, np.float64)
    lags = np.asarray(lags).astype(np.int64).reshape(-1, 2)
    N, L = dist.shape[0], lags.shape[0]
    if dist.shape != (N, K * (K + 1) // 2) or nvalid.shape != (N,) or npairs.shape != (N, L) or sums.shape != (N, L, 3):
        raise ValueError(f'expected dist (N, {K * (K + 1) // 2}), nvalid (N,), npairs (N, {L}) and sums (N, {L}, 3), got '
                         f'{dist.shape}, {nvalid.shape}, {npairs.shape}, {sums.shape}')
    nan = float('nan')
    c = 1.0 / (K * (K - 1)) if fair else 1.0 / (K * K)
    member = np.sqrt(dist[:, :K])
    pair = np.sqrt(dist[:, K:])
    es = np.full(N, nan)
    for i in range(N):
        if nvalid[i] > 0:
            es[i] = math.fsum(member[i].tolist()) / K - c * math.fsum(pair[i].tolist())
    scored = [float(v) for v, m in zip(es, nvalid) if m > 0]
    lag_distance = np.sqrt((lags.astype(np.float64) ** 2).sum(axis=1))
    omega = 1.0 / lag_distance if lag_weights == 'inverse' else np.ones(L)
    om = omega.tolist()

    def weighted(s, n):                                         # sum_l w_l s_l / sum_l w_l n_l
        den = math.fsum(w * float(v) for w, v in zip(om, n))
        return math.fsum(w * float(v) for w, v in zip(om, s)) / den if den > 0 else nan

    vs = np.asarray([weighted(sums[i, :, 0], npairs[i]) for i in range(N)], np.float64).reshape(N)
    tot_n = [int(npairs[:, l].sum()) for l in range(L)]
    tot = [[math.fsum(sums[:, l, q].tolist()) for q in range(3)] for l in range(L)]
    per_lag = lambda q: np.asarray([tot[l][q] / tot_n[l] if tot_n[l] else nan for l in range(L)], np.float64).reshape(L)  # noqa: E731
    return dict(energy_score=math.fsum(scored) / len(scored) if scored else nan, energy_score_per_sample=es,
                member_distance=member, pair_distance=pair,
                variogram_score=weighted([t[0] for t in tot], tot_n), variogram_score_per_sample=vs,
                lags=lags, lag_distance=lag_distance, lag_weight=omega,
                variogram_obs=per_lag(1), variogram_ens=per_lag(2), variogram_error=per_lag(0),
                n_pairs=npairs, n_valid_per_sample=nvalid, n_members=K, fair=bool(fair),
                dist_sums=dist, variogram_sums=sums)


class MultivariateScorer(_Accumulators):
    """The counterpart of ``Scorer`` for the energy and variogram scores (csrc/ensemble_multi.hip): per
    batch the two entries write the per-sample sums, which come back with the batch; ``result`` derives the scores on the host
    (``multivariate_from_sums``).  ``max_lag``, ``order_code``, ``w32``: what ``check_multivariate_args`` returned."""

    def __init__(self, n_members, n_samples, sample_shape, max_lag, order, order_code, lag_weights, fair, w32, bmax):
        npo = int(n_members) * (int(n_members) + 1) // 2
        super().__init__(n_members, n_samples, sample_shape, False, bmax, (npo,), np.float64)
        self.max_lag, self.order, self.order_code = int(max_lag), float(order), int(order_code)
        self.lag_weights, self.fair = lag_weights, bool(fair)
        self.lags = variogram_lags(self.max_lag)
        L = self.lags.shape[0]
        shape = self.sample_shape
        self.planes = int(np.prod(shape[:-3], dtype=np.int64))
        self.H, self.W, self.C = shape[-3:]
        self.dev.update(nvalid=DeviceArray((self.bmax,), np.int64), npairs=DeviceArray((self.bmax, L), np.int64),
                        vsums=DeviceArray((self.bmax, L, 3), np.float64))
        if w32 is not None:
            self.dev['weight'] = DeviceArray.from_numpy(np.ascontiguousarray(w32, np.float32).reshape(self.per))
        self.nvalid = np.zeros((self.N,), np.int64)
        self.npairs = np.zeros((self.N, L), np.int64)
        self.vsums = np.zeros((self.N, L, 3), np.float64)

    def _launch(self, stack_ptr, stride, obs_ptr, first, b):
        d = self.dev
        w = d['weight'].ptr if 'weight' in d else None
        _lib.check(self.lib.dl4ds_ensemble_energy(stack_ptr, self.K, b * self.per, stride, obs_ptr, b, w, d['sample'].ptr,
                                                  d['nvalid'].ptr))
        _lib.check(self.lib.dl4ds_ensemble_variogram(stack_ptr, self.K, b * self.per, stride, obs_ptr, b, w, self.planes, self.H,
                                                     self.W, self.C, self.max_lag, self.order_code, d['npairs'].ptr, d['vsums'].ptr))
        d['nvalid'].download(self.nvalid[first:first + b])
        d['npairs'].download(self.npairs[first:first + b])
        d['vsums'].download(self.vsums[first:first + b])

    def result(self):
        res = multivariate_from_sums(self.sample_sums, self.nvalid, self.npairs, self.vsums, self.K, self.lags, self.lag_weights,
                                     self.fair)
        res['order'] = self.order
        return res
