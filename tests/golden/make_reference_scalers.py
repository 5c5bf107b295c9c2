"""Regenerate the recorded behaviour of the reference's MinMaxScaler / StandardScaler:

* tests/golden/reference_scalers.npz: for every case of cases() the input, every fitted attribute, the transform and
  inverse_transform outputs and the names of the exception types raised;
* tests/golden/reference_preprocessing_api.json: the constructor and method signatures, read by AST.

The reference's preprocessing.py is loaded by file path (its package __init__ imports TensorFlow) with an empty stub module named
``xarray`` (one class ``DataArray``) registered first; scikit-learn and scipy must be installed (the stored fixtures were made with
scikit-learn 1.7).  Nothing of the reference's text is carried here; both outputs are recorded data.

    python tests/golden/make_reference_scalers.py PATH/TO/dl4ds              # compare with the stored files; exit 1 if they differ
    python tests/golden/make_reference_scalers.py PATH/TO/dl4ds --write      # or replace them
"""
import ast
import importlib.util
import io
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_api import _spec  # noqa: E402

NPZ = os.path.join(HERE, 'reference_scalers.npz')
API = os.path.join(HERE, 'reference_preprocessing_api.json')
CLASSES = ('MinMaxScaler', 'StandardScaler')
METHODS = ('__init__', 'fit', 'partial_fit', 'transform', 'inverse_transform')
ATTRS = ('scale_', 'min_', 'data_min_', 'data_max_', 'data_range_', 'mean_', 'std_', 'nan_mask')


def load_reference(ref):
    stub = types.ModuleType('xarray')
    stub.DataArray = type('DataArray', (), {})
    sys.modules.setdefault('xarray', stub)
    spec = importlib.util.spec_from_file_location('_reference_preprocessing', os.path.join(ref, 'preprocessing.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def signatures(ref):
    with open(os.path.join(ref, 'preprocessing.py')) as f:
        tree = ast.parse(f.read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in CLASSES:
            fns = {n.name: n.args for n in node.body if isinstance(n, ast.FunctionDef)}
            out[node.name] = {m: _spec(fns[m]) for m in METHODS}
    return {'preprocessing.py': out}


def field(rng, shape, dtype, nan):
    """temperature-like values (mean 281, std 12: |mean| / std = 23); nan: scattered NaNs plus all-NaN blocks that empty cells"""
    x = (281.0 + 12.0 * rng.standard_normal(shape)).astype(dtype)
    if nan:
        x[rng.random(shape) < 0.05] = np.nan
        x[:, :2, :3] = np.nan               # empties cells of the axis=0 and axis=(0,2) reductions
        x[1] = np.nan                       # ... and of axis=(1,2)
    return x


def axis_tag(axis):
    return 'None' if axis is None else ''.join(str(a) for a in np.atleast_1d(axis))


def cases():
    """-> list of (name, class name, constructor kwargs, fit array, transform array or None (= the fit array))"""
    rng = np.random.default_rng(20261016)
    out = []
    for dtype in (np.float32, np.float64):
        for nan in (False, True):
            x3 = field(rng, (6, 5, 8), dtype, nan)
            x4 = field(rng, (5, 3, 4, 3), dtype, nan)
            for axis, x in ((None, x3), (0, x3), ((1, 2), x3), ((0, 2), x3), ((0, 1, 2), x4)):
                tag = f"{np.dtype(dtype).name}_{'nan' if nan else 'clean'}_axis{axis_tag(axis)}"
                for cls in CLASSES:
                    out.append((f'{cls}_{tag}', cls, dict(axis=axis), x, None))
    x = field(rng, (6, 5, 8), np.float32, True)
    out.append(('MinMaxScaler_range_m1_1', 'MinMaxScaler', dict(value_range=(-1, 1), axis=0), x, None))
    const = np.full((6, 5, 7), 3.5, np.float32)
    out.append(('MinMaxScaler_constant', 'MinMaxScaler', dict(axis=None), const, None))
    out.append(('StandardScaler_constant', 'StandardScaler', dict(axis=0), const, None))
    for wm in (True, False):
        for ws in (True, False):
            out.append((f'StandardScaler_mean{int(wm)}_std{int(ws)}', 'StandardScaler',
                        dict(with_mean=wm, with_std=ws, axis=(1, 2)), x, None))
    out.append(('MinMaxScaler_shape_mismatch', 'MinMaxScaler', dict(axis=None), x, x[:4]))
    out.append(('StandardScaler_shape_mismatch', 'StandardScaler', dict(axis=None), x, x[:4]))
    out.append(('StandardScaler_other_shape_no_mask', 'StandardScaler', dict(axis=0), field(rng, (6, 5, 8), np.float32, False),
                field(rng, (4, 5, 8), np.float32, False)))
    out.append(('MinMaxScaler_nhw1', 'MinMaxScaler', dict(axis=None), field(rng, (6, 8, 9, 1), np.float32, False), None))
    # exact: small integers 0..15 with 10 % NaNs -> every fp32 sum is exact, so the reference's fp32 mean / min / max are the
    # correctly rounded true values
    xe3 = rng.integers(0, 16, (12, 8, 16)).astype(np.float32)
    xe3[rng.random(xe3.shape) < 0.1] = np.nan
    xe4 = rng.integers(0, 16, (8, 6, 8, 3)).astype(np.float32)
    xe4[rng.random(xe4.shape) < 0.1] = np.nan
    for axis, xe in ((None, xe3), (0, xe3), ((1, 2), xe3), ((0, 1, 2), xe4)):
        for cls in CLASSES:
            out.append((f'{cls}_exact_axis{axis_tag(axis)}', cls, dict(axis=axis), xe, None))
    return out


def run(mod):
    rec = {}
    meta = {}            # every string of the record: one JSON entry instead of hundreds of tiny archive members
    names = []
    stored = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, cls, kw, x, xt in cases():
            names.append(name)
            meta[f'{name}/class'] = cls
            meta[f'{name}/kwargs'] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
            for key, arr in (('x', x), ('xt', xt)):          # inputs shared by several cases are stored once
                if arr is not None:
                    if id(arr) not in stored:
                        stored[id(arr)] = f'input{len(stored)}'
                        rec[stored[id(arr)]] = arr
                    meta[f'{name}/{key}'] = stored[id(arr)]
            sc = getattr(mod, cls)(**kw)
            sc.fit(x.copy())
            for attr in ATTRS:
                if hasattr(sc, attr):
                    rec[f'{name}/{attr}'] = np.asarray(getattr(sc, attr))
            for meth in ('transform', 'inverse_transform'):
                try:
                    rec[f'{name}/{meth}'] = np.asarray(getattr(sc, meth)((x if xt is None else xt).copy()))
                except Exception as e:          # recorded, not judged
                    meta[f'{name}/{meth}_raises'] = type(e).__name__
        for cls in CLASSES:
            for meth in ('transform', 'inverse_transform'):
                try:
                    getattr(getattr(mod, cls)(), meth)(np.zeros((2, 3), np.float32))
                except Exception as e:
                    meta[f'not_fitted/{cls}/{meth}_raises'] = type(e).__name__
                    meta[f'not_fitted/{cls}/{meth}_bases'] = [b.__name__ for b in type(e).__mro__]
        try:
            mod.MinMaxScaler(value_range=(1, 1)).fit(np.zeros((2, 3), np.float32))
        except Exception as e:
            meta['bad_range/raises'] = type(e).__name__
    meta['case_names'] = names
    rec['meta'] = np.array(json.dumps(meta, sort_keys=True))
    return rec


def same(a, b):
    if sorted(a) != sorted(b):
        return False
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
               (np.array_equal(a[k], b[k], equal_nan=True) if a[k].dtype.kind == 'f' else np.array_equal(a[k], b[k])) for k in a)


def main(argv):
    if not argv or argv[0].startswith('-'):
        raise SystemExit(__doc__)
    ref = argv[0]
    api = json.loads(json.dumps(signatures(ref), sort_keys=True))
    rec = run(load_reference(ref))
    if '--write' in argv:
        with open(API, 'w') as f:
            json.dump(api, f, indent=1, sort_keys=True)
            f.write('\n')
        buf = io.BytesIO()
        np.savez_compressed(buf, **rec)
        with open(NPZ, 'wb') as f:
            f.write(buf.getvalue())
        print(f'wrote {API}\nwrote {NPZ} ({os.path.getsize(NPZ)} bytes, {len(json.loads(str(rec["meta"]))["case_names"])} cases)')
        return 0
    with open(API) as f:
        ok_api = api == json.load(f)
    with np.load(NPZ) as z:
        ok_npz = same(rec, {k: z[k] for k in z.files})
    print('reference_preprocessing_api.json ' + ('matches' if ok_api else 'differs from') + ' the reference')
    print('reference_scalers.npz ' + ('matches' if ok_npz else 'differs from') + ' the reference')
    return 0 if ok_api and ok_npz else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
