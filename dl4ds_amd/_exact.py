"""Exact host arithmetic the verification scores share (metrics.py, ensemble_score.py): thresholds and bin edges as the float32
values the device compares with, and quotients of integer sums, each rounded to float64 once, NaN on a zero denominator.  A leaf
module: numpy only, nothing from the package."""
import numpy as np


def finite_float32(values, name, least=1, increasing=False):
    """A 1-D sequence of at least ``least`` numbers -> float32 array.  Refuses values that are not finite, as given or once cast to
    float32, and with ``increasing`` values that do not strictly increase as float32.  ``name`` is how the messages call them."""
    v64 = np.asarray(values, np.float64)
    if v64.ndim != 1 or v64.size < least:
        raise ValueError(f'{name} must be a 1-D sequence of at least {least} value(s)')
    with np.errstate(over='ignore'):
        v32 = v64.astype(np.float32)
    if not np.isfinite(v64).all() or not np.isfinite(v32).all():
        raise ValueError(f'{name} must be finite (as float32)')
    if increasing and not (np.diff(v32) > 0).all():
        raise ValueError(f'{name} must be strictly increasing as float32 values')
    return v32


def ratio(num, den):
    """num / den in fp64, NaN where den == 0 (arrays of integers, or Python integers)."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den == 0, np.nan, num / np.where(den == 0, 1.0, den))


def int_ratio(num, den):
    """num / den of two Python integers, correctly rounded to fp64; NaN when den == 0."""
    return num / den if den else float('nan')


def ratio_exact(num, den):
    """Element-wise num / den of object arrays of Python integers, each quotient correctly rounded to fp64; NaN where den == 0."""
    num, den = np.asarray(num, object), np.asarray(den, object)
    out = np.full(num.shape, np.nan)
    for idx in np.ndindex(num.shape):
        out[idx] = int_ratio(int(num[idx]), int(den[idx]))
    return out


def quotient(num, den):
    """num / den element-wise for integer arrays (int64, or object arrays of Python integers), each quotient correctly rounded to
    fp64, NaN where den == 0.  Operands below 2^53 are exact in fp64, where one IEEE division is the correctly rounded quotient
    (``ratio``); anything larger goes through Python integers (``ratio_exact``)."""
    num, den = np.broadcast_arrays(np.asarray(num), np.asarray(den))
    if num.dtype != object and den.dtype != object and (num.size == 0 or (max(int(np.abs(num).max()), int(np.abs(den).max())) < 1 << 53)):
        return ratio(num, den)
    return ratio_exact(num.astype(object), den.astype(object))


def pysum(a, axis):
    """Sum of an int64 array over `axis` as Python integers (object array): cannot overflow."""
    return np.sum(a.astype(object), axis=axis)


def wide(a, bound):
    """int64 array ``a`` as it is when products up to ``bound`` fit into int64, else as Python integers"""
    return a if bound < 1 << 62 else a.astype(object)
