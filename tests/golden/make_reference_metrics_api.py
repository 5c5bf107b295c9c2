"""Regenerate tests/golden/reference_metrics_api.json: the parameter names, order and defaults of the public functions of the
reference's metrics.py (compute_rmse, compute_correlation, compute_metrics), read by AST without importing the reference, in
the format of make_reference_api.py.  tests/test_metrics_api.py checks dl4ds_amd.metrics against it.

    python tests/golden/make_reference_metrics_api.py PATH/TO/dl4ds              # compare with the stored file; exit 1 if it differs
    python tests/golden/make_reference_metrics_api.py PATH/TO/dl4ds --write      # or replace it
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_api import _functions, _spec  # noqa: E402

OUT = os.path.join(HERE, 'reference_metrics_api.json')
FUNCTIONS = ('compute_rmse', 'compute_correlation', 'compute_metrics')


def extract(ref):
    with open(os.path.join(ref, 'metrics.py')) as f:
        fns = _functions(ast.parse(f.read()))
    return {'metrics.py': {name: _spec(fns[name]) for name in FUNCTIONS}}


def main(argv):
    if not argv or argv[0].startswith('-'):
        raise SystemExit(__doc__)
    got = json.loads(json.dumps(extract(argv[0]), sort_keys=True))
    if '--write' in argv:
        with open(OUT, 'w') as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write('\n')
        print(f'wrote {OUT}')
        return 0
    with open(OUT) as f:
        same = got == json.load(f)
    print('reference_metrics_api.json matches the reference' if same else 'reference_metrics_api.json differs from the reference')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
