"""The one-op ConvLSTM2D graph of tests/test_gpu_ops.py::test_conv_lstm2d and tests/test_gpu_convlstm.py (not a test module)."""
import ctypes

import numpy as np
import pytest


class OneOp:
    """ConvLSTM2D(F, KS, 'same', return_sequences=True) [+ ReLU] on an input that asks for its gradient, with an MSE engine."""

    def __init__(self, Tn, H, W, C, F, KS, relu):
        from dl4ds_amd.graph import GraphBuilder, Model
        self.gb = GraphBuilder()
        self.xin = self.gb.input(H, W, C, nmul=Tn, requires_grad=True)
        out = self.gb.convlstm(self.xin, 'lstm', F, KS, Tn, activation='relu' if relu else None)
        self.gb.finalize(out, seed=1)
        self.model = Model(self.gb, 'convlstm_only', [(Tn, H, W, C)])
        self.engine = None

    def run(self, x, y):
        """Forward, then loss and gradients -> (output, loss, {name: gradient}) with dX under 'x', read from the input's gradient
        buffer."""
        from dl4ds_amd import _lib
        from dl4ds_amd.training import SupervisedEngine
        shape = y.shape             # (a one-step model reports its output without the time axis)
        y = np.ascontiguousarray(y).reshape((len(x),) + tuple(self.model.output_shape))
        got = self.model([x]).reshape(shape)
        if self.engine is None:
            self.engine = SupervisedEngine(self.model, loss='mse', learning_rate=1e-3)
        l_hip, g_hip = self.engine.loss_and_grads([x], y)
        p = ctypes.c_void_p()
        _lib.check(_lib.lib().dl4ds_graph_tensor_ptr(self.gb.h, self.xin.id, 1, ctypes.byref(p)))
        dx = np.empty(x.shape, np.float32)
        _lib.check(_lib.lib().dl4ds_memcpy_d2h(dx.ctypes.data, p, dx.nbytes))
        return got, l_hip, dict(g_hip, x=dx)


def assert_against_fp64(got, l_hip, grads, ref, what):
    """Output, loss and the four gradients against ``ref`` = tests.parity.banded_reference of the oracle: what test_conv_lstm2d asserts."""
    from tests.parity import assert_matches_reference
    from tests.test_gpu_ops import close
    close(got, ref['pred'])
    assert l_hip == pytest.approx(ref['loss'], rel=1e-4)
    assert_matches_reference(grads, ref, what=what)
