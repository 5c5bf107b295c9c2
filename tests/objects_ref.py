"""Numpy / pure-Python restatement of the object labelling defined in DESIGN.md section 27: a sequential flood fill in
raster order, which numbers the objects by their first cell as it goes, Python integers for the integer attributes, math.fsum for
the masses, and per fp64 sum the summation bound gamma_(n-1) * sum |term| that any order of n exact terms satisfies."""
import math

import numpy as np

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U) if k > 0 else 0.0


def ordered_key(v):
    """total order of float32 values as integers, +0.0 above -0.0"""
    b = int(np.float32(v).view(np.uint32))
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def neighbours(connectivity):
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 2:
        nb += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    return nb


def label_field(event, connectivity):
    """event: (H, W) bool -> (labels int32, count): flood fill from every unlabelled event cell in raster order"""
    H, W = event.shape
    lab = np.zeros((H, W), np.int32)
    ev = event.tolist()
    nb = neighbours(connectivity)
    n = 0
    for i0 in range(H):
        row = ev[i0]
        for j0 in range(W):
            if not row[j0] or lab[i0, j0]:
                continue
            n += 1
            lab[i0, j0] = n
            stack = [(i0, j0)]
            while stack:
                i, j = stack.pop()
                for di, dj in nb:
                    a, b = i + di, j + dj
                    if 0 <= a < H and 0 <= b < W and ev[a][b] and not lab[a, b]:
                        lab[a, b] = n
                        stack.append((a, b))
    return lab, n


def _bounded_sum(terms):
    """-> (math.fsum of the exact terms, the bound any summation order keeps)"""
    return math.fsum(terms), gamma(len(terms) - 1) * math.fsum(abs(t) for t in terms)


def objects(x, thr, connectivity, cap=None):
    """x: (N, H, W, C), thr: one value per field (N*C,) -> dict with the fields on the leading axis (f = n*C + c): labels (F, H, W),
    count, nvalid, field_sums (F, 3) with field_bound, and tables of `cap` rows (default: the largest count): sums (F, cap, 6),
    bbox, first, vmax, mass (F, cap, 3) with mass_bound.  Rows beyond a field's count are zero; objects beyond cap are left out."""
    x = np.asarray(x, np.float32)
    N, H, W, C = x.shape
    F = N * C
    thr = np.broadcast_to(np.asarray(thr, np.float32).reshape(-1), (F,))
    labels = np.zeros((F, H, W), np.int32)
    count, nvalid = np.zeros(F, np.int32), np.zeros(F, np.int64)
    fsum, fbound = np.zeros((F, 3)), np.zeros((F, 3))
    per = []
    for f in range(F):
        v = x[f // C, :, :, f % C]
        valid = np.isfinite(v)
        with np.errstate(invalid='ignore'):
            event = valid & (v >= thr[f])
        labels[f], count[f] = label_field(event, connectivity)
        nvalid[f] = int(valid.sum())
        ii, jj = np.nonzero(valid)
        vals = [float(t) for t in v[ii, jj]]
        for q, w in enumerate((None, ii, jj)):
            fsum[f, q], fbound[f, q] = _bounded_sum(vals if w is None else [a * int(b) for a, b in zip(vals, w)])
        rows = []
        ii, jj = np.nonzero(labels[f])
        order = np.argsort(labels[f][ii, jj], kind='stable')
        ii, jj = ii[order], jj[order]
        ends = np.cumsum(np.bincount(labels[f][ii, jj], minlength=count[f] + 1))
        for n in range(1, count[f] + 1):
            ci = [int(a) for a in ii[ends[n - 1]:ends[n]]]
            cj = [int(a) for a in jj[ends[n - 1]:ends[n]]]
            cv = [float(v[a, b]) for a, b in zip(ci, cj)]
            best = max((np.float32(t) for t in cv), key=ordered_key)
            rows.append(dict(
                sums=[len(ci), sum(ci), sum(cj), sum(a * a for a in ci), sum(b * b for b in cj), sum(a * b for a, b in zip(ci, cj))],
                bbox=[min(ci), max(ci), min(cj), max(cj)], first=min(a * W + b for a, b in zip(ci, cj)), vmax=best,
                mass=[_bounded_sum(cv), _bounded_sum([t * a for t, a in zip(cv, ci)]), _bounded_sum([t * b for t, b in zip(cv, cj)])]))
        per.append(rows)
    if cap is None:
        cap = int(count.max()) if F else 0
    out = dict(labels=labels, count=count, nvalid=nvalid, field_sums=fsum, field_bound=fbound,
               sums=np.zeros((F, cap, 6), np.int64), bbox=np.zeros((F, cap, 4), np.int32), first=np.zeros((F, cap), np.int32),
               vmax=np.zeros((F, cap), np.float32), mass=np.zeros((F, cap, 3)), mass_bound=np.zeros((F, cap, 3)))
    for f, rows in enumerate(per):
        for r, row in enumerate(rows[:cap]):
            out['sums'][f, r], out['bbox'][f, r], out['first'][f, r], out['vmax'][f, r] = row['sums'], row['bbox'], row['first'], row['vmax']
            out['mass'][f, r] = [m[0] for m in row['mass']]
            out['mass_bound'][f, r] = [m[1] for m in row['mass']]
    return out


def factor_thresholds(x, factor):
    """factor * the largest finite float32 value of every field, as float32 (N*C,); 0 without a finite cell"""
    x = np.asarray(x, np.float32)
    N, H, W, C = x.shape
    thr = np.zeros(N * C, np.float32)
    for f in range(N * C):
        v = x[f // C, :, :, f % C]
        v = v[np.isfinite(v)]
        if v.size:
            t = np.float32(float(factor) * float(v.max()))
            thr[f] = t if np.isfinite(t) else 0.0
    return thr
