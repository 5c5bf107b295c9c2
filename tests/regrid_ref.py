"""Restatement of the regridding of dl4ds_amd/regrid.py and dl4ds_amd/csrc/regrid.hip in numpy: the axis
tables, built here from a DENSE overlap matrix (every source against every destination, every shift of a periodic source), the
value of every output element with the kernel's operations in the kernel's order, and the consistency sums in their one
summation order (a lane's cells ascending, the tree over 256 lanes, the rows ascending).  Sequential and slow: for the small cases
of tests/regrid_cases.py."""
import math

import numpy as np

THREADS = 256
NAN32 = np.float32(np.nan)


# ---- tables
def bounds_from_centres(c, spherical):
    c = np.asarray(c, np.float64)
    b = np.empty(c.size + 1)
    for k in range(1, c.size):
        b[k] = (c[k - 1] + c[k]) / 2
    b[0] = c[0] - (c[1] - c[0]) / 2
    b[-1] = c[-1] + (c[-1] - c[-2]) / 2
    return np.clip(b, -90.0, 90.0) if spherical else b


def cell_ranges(b, spherical):
    g = [math.sin(float(v) * math.pi / 180.0) if spherical else float(v) for v in b]
    lo = np.array([min(g[k], g[k + 1]) for k in range(len(g) - 1)])
    hi = np.array([max(g[k], g[k + 1]) for k in range(len(g) - 1)])
    return lo, hi


def dense_conservative(sb, db, spherical=False, periodic=False, period=360.0):
    """-> (M[shift][d][s]: the overlap of destination d with source s moved by shift * period, the shifts, lower source bounds)"""
    slo, shi = cell_ranges(sb, spherical)
    dlo, dhi = cell_ranges(db, spherical)
    if periodic:
        shifts = list(range(int(math.floor((dlo.min() - shi.max()) / period)) - 1, int(math.ceil((dhi.max() - slo.min()) / period)) + 2))
    else:
        shifts = [0]
    M = np.zeros((len(shifts), dlo.size, slo.size))
    for q, k in enumerate(shifts):
        lo = slo + float(k) * period if periodic else slo
        hi = shi + float(k) * period if periodic else shi
        M[q] = np.maximum(0.0, np.minimum(hi[None, :], dhi[:, None]) - np.maximum(lo[None, :], dlo[:, None]))
    return M, shifts, slo


def table_from_dense(M, shifts, slo, periodic, period=360.0):
    rows = []
    for d in range(M.shape[1]):
        taps = [(slo[s] + float(shifts[q]) * period if periodic else float(s), s, M[q, d, s])
                for q in range(M.shape[0]) for s in range(M.shape[2]) if M[q, d, s] > 0]
        taps.sort(key=lambda t: t[0])                 # ascending unwrapped position / ascending source index
        rows.append([(s, w) for _, s, w in taps])
    return rows


def dense_points(sc, dc, method, periodic=False, period=360.0, extrapolate='nearest'):
    sc, dc = np.asarray(sc, np.float64), np.asarray(dc, np.float64)
    order = np.argsort(sc)                            # position in ascending order -> source index
    pts = [(float(sc[s]), int(s)) for s in order]
    if periodic:
        pts.append((pts[0][0] + period, pts[0][1]))
    rows = []
    for v in dc:
        v = float(v)
        if periodic:
            c0 = pts[0][0]
            v = v - math.floor((v - c0) / period) * period
            v = min(max(v, c0), c0 + period)
        if method == 'nearest':
            dist = [abs(p - v) for p, _ in pts]
            best = min(dist)
            rows.append([(min(s for (p, s), dd in zip(pts, dist) if dd == best), 1.0)])
            continue
        if v < pts[0][0] or v > pts[-1][0]:
            rows.append([(pts[0][1] if v < pts[0][0] else pts[-1][1], 1.0)] if extrapolate == 'nearest' else [])
            continue
        if len(pts) == 1 or v == pts[-1][0]:
            rows.append([(pts[-1][1], 1.0)])
            continue
        for k in range(len(pts) - 1):
            if pts[k][0] <= v < pts[k + 1][0]:
                t = (v - pts[k][0]) / (pts[k + 1][0] - pts[k][0])
                taps = [(pts[k][1], 1.0 - t), (pts[k + 1][1], t)]
                taps = [(s, w) for s, w in taps if w > 0]
                rows.append(taps if periodic else sorted(taps, key=lambda q: q[0]))
                break
    return rows


def axis_rows(src, dst, method='conservative', spherical=False, periodic=False, period=360.0, src_bounds=None, dst_bounds=None,
              extrapolate='nearest'):
    """-> the taps of every destination as a list of (source index, weight)"""
    if method == 'conservative':
        sb = np.asarray(src_bounds, np.float64) if src_bounds is not None else bounds_from_centres(src, spherical)
        db = np.asarray(dst_bounds, np.float64) if dst_bounds is not None else bounds_from_centres(dst, spherical)
        M, shifts, slo = dense_conservative(sb, db, spherical, periodic, period)
        return table_from_dense(M, shifts, slo, periodic, period)
    return dense_points(src, dst, method, periodic, period, extrapolate)


def csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([s for r in rows for s, _ in r], np.int32).reshape(-1), np.array([w for r in rows for _, w in r],
                                                                                          np.float64).reshape(-1)


def triples(ptr, idx, w):
    """a CSR table as a sorted list of (destination, source, the weight's bits)"""
    return sorted((d, int(idx[t]), np.float64(w[t]).tobytes()) for d in range(len(ptr) - 1) for t in range(ptr[d], ptr[d + 1]))


def dense_matrix(ptr, idx, w, n_src):
    M = np.zeros((len(ptr) - 1, n_src))
    for d in range(len(ptr) - 1):
        for t in range(ptr[d], ptr[d + 1]):
            M[d, idx[t]] += w[t]
    return M


# ---- apply
def apply(x, ty, tx, skipna=False, min_valid=0.5):
    """x (N, H, W, C) float32, ty / tx = (ptr, idx, w) -> (N, H', W', C) float32: per output the y-taps in table order, inside each
    the x-taps in table order; w = wy * wx; tot += w; [skipna: non-finite x skipped]; num += w * x; den += w; the elementwise numpy
    operations over (N, C) round as the scalar ones do"""
    x = np.asarray(x, np.float32)
    N, H, W, C = x.shape
    (yp, yi, yw), (xp, xi, xw) = ty, tx
    Ho, Wo = len(yp) - 1, len(xp) - 1
    out = np.empty((N, Ho, Wo, C), np.float32)
    mv = np.float64(min_valid)
    with np.errstate(all='ignore'):
        for i in range(Ho):
            for j in range(Wo):
                num, den, tot = np.zeros((N, C)), np.zeros((N, C)), np.zeros((N, C))
                for a in range(yp[i], yp[i + 1]):
                    for b in range(xp[j], xp[j + 1]):
                        w = np.float64(yw[a]) * np.float64(xw[b])
                        tot = tot + w
                        v = x[:, yi[a], xi[b], :]
                        p = w * v.astype(np.float64)
                        if skipna:
                            fin = np.isfinite(v)
                            num = np.where(fin, num + p, num)
                            den = np.where(fin, den + w, den)
                        else:
                            num = num + p
                            den = den + w
                ok = (den > 0) & (den >= mv * tot)
                q = (num / np.where(ok, den, 1.0)).astype(np.float32)
                out[:, i, j, :] = np.where(ok & ~np.isnan(q), q, NAN32)
    return out


def dense_apply(x, ty, tx, n_src):
    """the independent evaluation of finite data without skipna: einsum in fp64 with the dense matrices -> (want fp64, sum |w x| / den,
    taps per output)"""
    My, Mx = dense_matrix(*ty, n_src[0]), dense_matrix(*tx, n_src[1])
    x64 = np.asarray(x, np.float64)
    num = np.einsum('ih,jw,nhwc->nijc', My, Mx, x64)
    mag = np.einsum('ih,jw,nhwc->nijc', My, Mx, np.abs(x64))
    den = np.outer(My.sum(1), Mx.sum(1))[None, :, :, None]
    taps = np.outer(np.diff(ty[0]), np.diff(tx[0]))[None, :, :, None]
    with np.errstate(all='ignore'):
        return num / den, mag / den, taps


# ---- consistency
def _cell(acc, r, y, A):
    fr, fy = bool(np.isfinite(r)), bool(np.isfinite(y))
    if not (fr and fy):
        if fr != fy:
            acc[7] += 1
        return NAN32
    rd, yd = float(r), float(y)
    d = rd - yd
    acc[0] = acc[0] + A
    acc[1] = acc[1] + A * d
    acc[2] = acc[2] + A * (d * d)
    acc[3] = acc[3] + A * yd
    acc[4] = acc[4] + A * rd
    acc[5] = abs(d) if abs(d) > acc[5] else acc[5]
    acc[6] += 1
    return np.float32(r) - np.float32(y)


def _join(acc, t):
    for k in range(5):
        acc[k] = acc[k] + t[k]
    acc[5] = t[5] if t[5] > acc[5] else acc[5]
    acc[6] += t[6]
    acc[7] += t[7]


def _zero():
    return [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0]


def consistency(x, ref, ty, tx, ay, ax, skipna=False, min_valid=0.5):
    """-> dict(out: the regridded x, sums (N, C, 6) fp64, counts (N, C, 2) int64, resid (N, H', W', C) float32)"""
    r = apply(x, ty, tx, skipna, min_valid)
    ref = np.asarray(ref, np.float32)
    N, Ho, Wo, C = r.shape
    sums, counts = np.zeros((N, C, 6)), np.zeros((N, C, 2), np.int64)
    resid = np.empty(r.shape, np.float32)
    with np.errstate(all='ignore'):
        for n in range(N):
            for c in range(C):
                total = _zero()
                for i in range(Ho):
                    lanes = [_zero() for _ in range(THREADS)]
                    for t in range(THREADS):
                        for j in range(t, Wo, THREADS):
                            resid[n, i, j, c] = _cell(lanes[t], r[n, i, j, c], ref[n, i, j, c], float(ay[i]) * float(ax[j]))
                    o = THREADS // 2
                    while o > 0:
                        for t in range(o):
                            _join(lanes[t], lanes[t + o])
                        o //= 2
                    _join(total, lanes[0])
                sums[n, c] = total[:6]
                counts[n, c] = total[6:]
    return dict(out=r, sums=sums, counts=counts, resid=resid)


def same_bits(got, want, what=''):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.argwhere(got.view(view) != want.view(view))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
