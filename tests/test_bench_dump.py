"""bench.py --dump-outputs, host side: file names, dtypes, and the fixed seeded sample that stands for a large array."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_names_dtypes_and_sampling(tmp_path):
    import bench
    big = np.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=np.float32).reshape(-1, 8)
    arrays = {'loss': np.asarray([1.25], np.float32), 'weights/Block1/conv/kernel': np.ones((3, 3, 2, 4), np.float16),
              'f64': np.linspace(0, 1, 5), 'pred': big}
    got = bench.dump_outputs(str(tmp_path / 'a'), arrays)
    assert sorted(got) == ['f64.npy', 'loss.npy', 'pred.npy', 'weights.Block1.conv.kernel.npy']
    assert np.load(tmp_path / 'a' / 'loss.npy').tolist() == [1.25]
    k = np.load(tmp_path / 'a' / 'weights.Block1.conv.kernel.npy')
    assert k.dtype == np.float32 and k.shape == (3, 3, 2, 4)
    assert np.load(tmp_path / 'a' / 'f64.npy').dtype == np.float64
    p = np.load(tmp_path / 'a' / 'pred.npy')
    assert p.dtype == np.float32 and p.shape == (bench.DUMP_MAX_ELEMS,) and got['pred.npy']['shape'] == list(big.shape)
    # the sample: distinct elements in increasing flat order, the same ones in every run
    assert (np.diff(p) > 0).all()
    bench.dump_outputs(str(tmp_path / 'b'), {'pred': big})
    assert np.array_equal(np.load(tmp_path / 'b' / 'pred.npy'), p)
