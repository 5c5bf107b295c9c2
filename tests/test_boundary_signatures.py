"""The drop-in boundary keeps the reference's call signatures: every builder, trainer and Predictor entry point is
compared with the reference's own signatures for parameter names, POSITIONAL ORDER and default values.  Those are stored in
tests/golden/reference_api.json, read from the reference's source by tests/golden/make_reference_api.py (AST, no import -- the
reference needs TensorFlow).

Arguments the build adds (``seed``, the static-graph sizes ``hr_size`` / ``time_window`` of the discriminator,
``checkpoint`` / ``device_data``) must come AFTER every reference parameter, so positional callers are unaffected."""
import importlib
import inspect
import json
import os

import pytest

REF_API = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_api.json')

PAIRS = [
    ('models/sp_postups.py', 'net_postupsampling', 'dl4ds_amd.models', 'net_postupsampling'),
    ('models/sp_preups.py', 'net_pin', 'dl4ds_amd.models', 'net_pin'),
    ('models/sp_preups.py', 'unet_pin', 'dl4ds_amd.models', 'unet_pin'),
    ('models/spt_postups.py', 'recnet_postupsampling', 'dl4ds_amd.models', 'recnet_postupsampling'),
    ('models/spt_preups.py', 'recnet_pin', 'dl4ds_amd.models', 'recnet_pin'),
    ('models/discriminator.py', 'residual_discriminator', 'dl4ds_amd.models', 'residual_discriminator'),
    ('training/base.py', 'Trainer.__init__', 'dl4ds_amd.training.base', 'Trainer.__init__'),
    ('training/base.py', 'Trainer.save_results', 'dl4ds_amd.training.base', 'Trainer.save_results'),
    ('training/supervised.py', 'SupervisedTrainer.__init__', 'dl4ds_amd.training', 'SupervisedTrainer.__init__'),
    ('training/supervised.py', 'SupervisedTrainer.run', 'dl4ds_amd.training', 'SupervisedTrainer.run'),
    ('training/cgan.py', 'CGANTrainer.__init__', 'dl4ds_amd.training', 'CGANTrainer.__init__'),
    ('training/cgan.py', 'CGANTrainer.run', 'dl4ds_amd.training', 'CGANTrainer.run'),
    ('inference.py', 'Predictor.__init__', 'dl4ds_amd.inference', 'Predictor.__init__'),
    ('inference.py', 'Predictor.run', 'dl4ds_amd.inference', 'Predictor.run'),
]

# defaults that differ on purpose: (function, parameter) -> why
DEFAULT_EXCEPTIONS = {
    # cgan.py:45 defaults time_window to True, which makes the reference reject its own 'unet' backbone unless the caller
    # passes time_window=None (utils.py:76-79); None is what every working call passes
    ('CGANTrainer.__init__', 'time_window'),
}


def _ref_spec(path, name):
    with open(REF_API) as f:
        spec = json.load(f)['signatures'][path][name]
    return spec['positional'], spec['defaults'], spec['kwarg']


@pytest.mark.parametrize('ref_path,ref_name,mod,name', PAIRS)
def test_signature_matches_the_reference(ref_path, ref_name, mod, name):
    pos, dfl, kwarg = _ref_spec(ref_path, ref_name)
    obj = importlib.import_module(mod)
    for part in name.split('.'):
        obj = getattr(obj, part)
    params = inspect.signature(obj).parameters
    mine = [p for p, v in params.items() if v.kind in (v.POSITIONAL_OR_KEYWORD, v.POSITIONAL_ONLY)]
    # every reference parameter, in the reference's positional order, BEFORE anything the build adds
    assert mine[:len(pos)] == pos, f'{ref_name}: positional order differs\n ref : {pos}\n mine: {mine}'
    for extra in mine[len(pos):]:
        assert params[extra].default is not inspect.Parameter.empty, f'{ref_name}: added parameter {extra} needs a default'
    if kwarg:
        assert any(v.kind == v.VAR_KEYWORD for v in params.values()), f'{ref_name}: **{kwarg} missing'
    for k in pos:
        if k in dfl:
            assert params[k].default is not inspect.Parameter.empty, f'{ref_name}: {k} lost its default'
            if (ref_name, k) in DEFAULT_EXCEPTIONS:
                continue
            mine_d = params[k].default
            ref_d = dfl[k]
            if isinstance(ref_d, (list, tuple)):
                mine_d, ref_d = tuple(mine_d), tuple(ref_d)
            assert mine_d == ref_d, f'{ref_name}: default of {k}: reference {ref_d!r}, here {mine_d!r}'
        else:
            assert params[k].default is inspect.Parameter.empty, f'{ref_name}: {k} is required in the reference'
