"""Regenerate tests/golden/reference_api.json: the facts about the reference's public API that
tests/test_boundary_signatures.py and tests/test_name_map.py check this package against, read from a checkout of the
reference (AST only, no import -- the reference needs TensorFlow).

    python tests/golden/make_reference_api.py PATH/TO/dl4ds              # compare with the stored file; exit 1 if it differs
    python tests/golden/make_reference_api.py PATH/TO/dl4ds --write      # or replace it

PATH/TO/dl4ds is the package directory of the reference (the one holding models/, training/, inference.py).  Stored:
* ``signatures``: for every entry point the drop-in boundary mirrors, the positional parameter names in order, the
  defaults (``ast.literal_eval`` where the default is a literal, else its source form) and the name of ``**kwargs``;
* ``classes``: for every class of models/blocks.py, its base classes and the attributes its methods assign on ``self``;
* ``layer_names``: which of LAYER_NAME_SNIPPETS (the layer-name expressions the Keras name map relies on) occur in the
  builder modules.
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'reference_api.json')

# (reference module, function or Class.method) of every entry point whose signature the package keeps
ENTRY_POINTS = [
    ('models/sp_postups.py', 'net_postupsampling'),
    ('models/sp_preups.py', 'net_pin'),
    ('models/sp_preups.py', 'unet_pin'),
    ('models/spt_postups.py', 'recnet_postupsampling'),
    ('models/spt_preups.py', 'recnet_pin'),
    ('models/discriminator.py', 'residual_discriminator'),
    ('training/base.py', 'Trainer.__init__'),
    ('training/base.py', 'Trainer.save_results'),
    ('training/supervised.py', 'SupervisedTrainer.__init__'),
    ('training/supervised.py', 'SupervisedTrainer.run'),
    ('training/cgan.py', 'CGANTrainer.__init__'),
    ('training/cgan.py', 'CGANTrainer.run'),
    ('inference.py', 'Predictor.__init__'),
    ('inference.py', 'Predictor.run'),
]

BUILDER_MODULES = ('sp_postups.py', 'sp_preups.py', 'spt_postups.py', 'spt_preups.py', 'discriminator.py', 'blocks.py')

LAYER_NAME_SNIPPETS = (
    "'ResidualBlock' + str(i+1)", "'ConvBlock' + str(i+1)", "'DenseBlock' + str(i+1)", "'Transition' + str(i+1)",
    "'ConvNextBlock' + str(i+1)", "name='TransitionLast'", "name='ConvBlock_aux'", "name='TransitionBackboneLast'",
    "name='TransitionDC'", "name='Bottleneck'", "'DecoderConvBlock' + str(j+1)", "name='EncoderBlock' + name_suffix",
    "name='SubpixelConvolution' + name_suffix", "name='ResizeConvolution' + name_suffix",
    "name='Deconvolution' + name_suffix", "name='upsampling_' + upsampling", "name='localized_conv_block'",
    "_branch1'", "_branch2'", "name='deconv_1of2_scale_x2'", "name='deconv_2of2_scale_x2'",
    "name='deconv_scale_x' + str(self.scale)",
)


def _functions(tree):
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            out[node.name] = node.args
        elif isinstance(node, ast.ClassDef):
            for n in node.body:
                if isinstance(n, ast.FunctionDef):
                    out[node.name + '.' + n.name] = n.args
    return out


def _spec(a):
    pos = [x.arg for x in a.args]
    defaults = {}
    for x, d in zip(pos[len(pos) - len(a.defaults):], a.defaults):
        try:
            defaults[x] = ast.literal_eval(d)
        except Exception:
            defaults[x] = ast.unparse(d)
    return {'positional': pos, 'defaults': defaults, 'kwarg': a.kwarg.arg if a.kwarg else None}


def _classes(tree):
    out = {}
    for node in tree.body:
        if isinstance(node, ast.ClassDef):
            attrs = set()
            for sub in ast.walk(node):
                if isinstance(sub, ast.Assign):
                    for t in sub.targets:
                        if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == 'self':
                            attrs.add(t.attr)
            out[node.name] = {'bases': [b.id for b in node.bases if isinstance(b, ast.Name)], 'attrs': sorted(attrs)}
    return out


def extract(ref):
    def read(path):
        with open(os.path.join(ref, path)) as f:
            return f.read()
    sigs = {}
    for path, name in ENTRY_POINTS:
        sigs.setdefault(path, {})[name] = _spec(_functions(ast.parse(read(path)))[name])
    src = ''.join(read(os.path.join('models', f)) for f in BUILDER_MODULES)
    return {'signatures': sigs,
            'classes': _classes(ast.parse(read(os.path.join('models', 'blocks.py')))),
            'layer_names': [s for s in LAYER_NAME_SNIPPETS if s in src]}


def load():
    with open(OUT) as f:
        return json.load(f)


def main(argv):
    if not argv or argv[0].startswith('-'):
        raise SystemExit(__doc__)
    # (a JSON round trip: tuples become lists, as in the stored file)
    got = json.loads(json.dumps(extract(argv[0]), sort_keys=True))
    if '--write' in argv:
        with open(OUT, 'w') as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write('\n')
        print(f'wrote {OUT}')
        return 0
    same = got == load()
    print('reference_api.json matches the reference' if same else 'reference_api.json differs from the reference')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
