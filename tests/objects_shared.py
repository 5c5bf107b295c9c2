"""What the CPU and GPU tests of the device object labelling share: the restatement of every case, computed once per process, and
its tables cut or padded to a `cap`."""
import functools

import numpy as np

from tests import objects_ref
from tests.objects_cases import CASES, field_thresholds

TABLES = ('sums', 'bbox', 'first', 'vmax', 'mass', 'mass_bound')


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    """-> (x, float32 thresholds per field, objects_ref.objects at the largest count); read-only"""
    c = CASES[name]()
    x, thr = c['x'], field_thresholds(c)
    ref = objects_ref.objects(x, thr, connectivity)
    for a in (x, thr) + tuple(ref.values()):
        a.setflags(write=False)
    return x, thr, ref


def capped(ref, cap):
    """the restatement with tables of `cap` rows (None: as they are): objects beyond cap left out, rows beyond the largest count zero"""
    if cap is None:
        return ref
    out = dict(ref)
    for k in TABLES:
        a = ref[k][:, :cap]
        pad = np.zeros((a.shape[0], cap - a.shape[1]) + a.shape[2:], a.dtype)
        out[k] = np.concatenate([a, pad], axis=1)
    return out


def same_objects(got, want):
    """integers, labels and vmax equal (the sign of a zero too); the fp64 sums within the bound any summation order keeps"""
    for k in ('labels', 'count', 'nvalid', 'sums', 'bbox', 'first', 'vmax'):
        if k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert np.asarray(got['vmax'], np.float32).tobytes() == want['vmax'].tobytes()
    assert (np.abs(got['mass'] - want['mass']) <= want['mass_bound']).all()
    assert (np.abs(got['field_sums'] - want['field_sums']) <= want['field_bound']).all()
