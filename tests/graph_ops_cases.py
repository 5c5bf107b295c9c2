"""Inputs, size rules, dispatch restatements and references of tests/test_gpu_graph_ops.py (not a test module; needs no GPU).

The graph's copy / concat / add ops are pure selections of their inputs (or one IEEE add), so the GPU tests compare bitwise.  To
make that possible through the MAE loss (dY = g * sign(pred - target), g = 1 / size): inputs are integer-valued float32 from a hash
of the flat index (a misplaced element is a visible mismatch), and targets are ``forward - s`` with ``s`` a +-1 pattern from the same
hash, so every entry of dY is exactly ``g * s``."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ew_blocks (csrc/elementwise.hip): at most 8192 blocks of 256 threads per element-wise launch; a launch with more vector elements
# than this runs the grid-stride loop a second time.  tests/test_graph_ops_oracle.py checks the figure against the source.
EW_GRID_THREADS = 8192 * 256


def ew_grid_threads_in_source():
    src = open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'elementwise.hip')).read()
    m = re.search(r'inline int ew_blocks\(size_t n\) \{[^}]*cdivz\(n, (\d+)\), (\d+)\)', src)
    return int(m.group(1)) * int(m.group(2))


# ---------------------------------------------------------------------------------------------------------------- inputs
def _mix(n, seed):
    """murmur3's 32-bit finaliser of (flat index + seed): uint32 array of n hashes."""
    h = np.arange(n, dtype=np.uint32) + np.uint32((seed * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def hashed_ints(shape, seed, zeros=False):
    """Integer-valued float32 in [-64, 64] without zeros (``zeros``: a fifth of the entries exactly 0)."""
    h = _mix(int(np.prod(shape)), seed)
    v = ((h & np.uint32(63)) + np.uint32(1)).astype(np.float32)
    v *= (1.0 - 2.0 * ((h >> np.uint32(6)) & np.uint32(1)).astype(np.float32))
    if zeros:
        v[((h >> np.uint32(7)) % np.uint32(5)) == 0] = 0.0
    return v.reshape(shape)


def signs(shape, seed):
    """+-1 pattern (float32)."""
    h = _mix(int(np.prod(shape)), seed ^ 0x5BD1E995)
    return (1.0 - 2.0 * ((h >> np.uint32(9)) & np.uint32(1)).astype(np.float32)).reshape(shape)


def hashed_small_ints(shape, seed, zeros=False):
    """Integer-valued float32 in {-2, -1, 1, 2} (``zeros``: a fifth of the entries exactly 0) from the same hash: so few values that
    a 2x2 window often holds its maximum more than once."""
    h = _mix(int(np.prod(shape)), seed)
    v = ((h & np.uint32(1)) + np.uint32(1)).astype(np.float32)
    v *= (1.0 - 2.0 * ((h >> np.uint32(6)) & np.uint32(1)).astype(np.float32))
    if zeros:
        v[((h >> np.uint32(7)) % np.uint32(5)) == 0] = 0.0
    return v.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- size rule
def is_large(totalv):
    """The second-iteration rule: between 1.25x and 1.5x the grid cap in vector elements, so at least a quarter of the threads
    run the grid-stride loop (and its (pix, cv) stepping) a second time."""
    return 1.25 * EW_GRID_THREADS <= totalv <= 1.5 * EW_GRID_THREADS


def large_grid(cvn, width=61):
    """(N, H, W) = (1, H, width) whose pixel count times ``cvn`` vector elements per pixel sits mid-way in the rule."""
    npix = int(np.ceil(1.375 * EW_GRID_THREADS / cvn))
    h = -(-npix // width)
    assert is_large(h * width * cvn)
    return (1, h, width)


# ---------------------------------------------------------------------------------------------------------------- dispatch
# Restatements of the host-side dispatch of csrc/elementwise.hip for dense tensors and channel slices of dense tensors whose buffers
# are at least 16-byte aligned (Graph::prepare aligns every buffer to 256 bytes).  `off`: channel offset of the slice in its buffer.
def concat_onepass_vec(chans):
    """concat_join / concat_split: V = 2 when the pitch and every slice offset and width are even, else 1 -> (V, cvn)."""
    ld, off, even = sum(chans), 0, sum(chans) % 2 == 0
    for c in chans:
        even = even and off % 2 == 0 and c % 2 == 0
        off += c
    v = 2 if even else 1
    return v, ld // v


def view_axpy_variant(c, ld_a, off_a, ld_b, off_b, npix):
    """view_axpy between (a dense tensor or a slice of one) and another -> ('flat4' | 'strided4' | 'small2' | 'small1', V)."""
    if ld_a == c and ld_b == c and (npix * c) % 4 == 0:
        return 'flat4', 4
    if c % 4 == 0 and ld_a % 4 == 0 and ld_b % 4 == 0 and off_a % 4 == 0 and off_b % 4 == 0:
        return 'strided4', 4
    if (c | ld_a | ld_b | off_a | off_b) % 2 == 0:
        return 'small2', 2
    return 'small1', 1


def view_axpy_masked_variant(c, ld_wide, off):
    """view_axpy_masked out of a slice (pitch ld_wide, offset off) into a dense tensor with a dense mask -> 'masked4' | 'generic'."""
    return 'masked4' if c % 4 == 0 and ld_wide % 4 == 0 and off % 4 == 0 else 'generic'


# ---------------------------------------------------------------------------------------------------------------- activations
ACT_KINDS = ('relu', 'sigmoid', 'tanh', 'elu', 'leaky_relu', 'selu', 'gelu')
ACT_SMOOTH = ('sigmoid', 'tanh', 'elu', 'selu', 'gelu')
ACT_SPECIALS = np.array([0.0] + [sg * v for v in (1e-30, 1e-6, 0.5, 3.0, 30.0, 88.0, 104.0) for sg in (1.0, -1.0)], np.float32)
ACT_FLOOR = 2.0 ** -22        # two ulp of 1.0
ACT_CPU_CAP = 2.0 ** -20      # what the float32 CPU oracle itself must stay within of the float64 one


def act_inputs(shape, seed):
    """A seeded dense sample of [-20, 20] with the special values in front."""
    n = int(np.prod(shape))
    x = np.random.default_rng(seed).uniform(-20.0, 20.0, n).astype(np.float32)
    x[:ACT_SPECIALS.size] = ACT_SPECIALS
    return x.reshape(shape)


def act_oracle(kind, x, dy, dtype, residual=False):
    """oracle.torch_ops.activation at ``dtype`` on the CPU: (y, dx) for the upstream gradient dy; ``residual``: y = act(x) + x
    (the activation's gradient accumulates onto the Add's)."""
    import torch
    from oracle import torch_ops as T
    tx = torch.tensor(np.asarray(x, np.float64), dtype=dtype, requires_grad=True)
    y = T.activation(tx, kind)
    if residual:
        y = y + tx
    y.backward(torch.tensor(np.asarray(dy, np.float64), dtype=dtype))
    return y.detach().numpy().astype(np.float64), tx.grad.numpy().astype(np.float64)


def act_error(got, ref, x, scale=1.0):
    """E = max_i |got_i - ref_i| / max(1, |x_i|) (``scale``: the magnitude of the upstream gradient, for the backward direction)."""
    d = np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(np.asarray(x, np.float64)))
    return float(d.max() / scale)


def act_bound(e_cpu):
    return max(4.0 * e_cpu, ACT_FLOOR)


# ---------------------------------------------------------------------------------------------------------------- max-pool 2x2
POOL_QUAD_CHANS, POOL_SCALAR_CHANS = (4, 8), (3, 6)
POOL_GRIDS = ((2, 8, 12), (1, 7, 9), (1, 3, 2), (1, 2, 2))
POOL_ODD_GRIDS = tuple(g for g in POOL_GRIDS if (g[1] | g[2]) & 1)
POOL_WINDOW = ((0, 0), (0, 1), (1, 0), (1, 1))       # the order in which the backward kernels look for the maximum


def pool_quad(c):
    """pool_quad_ok for every view of a dense tensor in a 16-byte-aligned buffer (make_view sets vec = C % 4 == 0 and aligned; no
    depth_to_space layout, no channel affine): the four-channel kernels run iff C % 4 == 0."""
    return c % 4 == 0


def pool_quad_ok_in_source():
    """The conjuncts of pool_quad_ok (csrc/elementwise.hip) and make_view's rule for TView::vec (csrc/common.h), as written."""
    src = open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'elementwise.hip')).read()
    m = re.search(r'static bool pool_quad_ok\(const TView& v\) \{ return ([^;]*); \}', src)
    hdr = open(os.path.join(ROOT, 'dl4ds_amd', 'csrc', 'common.h')).read()
    v = re.search(r'inline TView make_view\(float\* p, int N, int H, int W, int C\) \{.*?v\.vec = ([^;]*);', hdr, re.S)
    return sorted(t.strip() for t in m.group(1).split('&&')), re.sub(r'\s+', '', v.group(1))


def pool_windows(x):
    """(4, N, H // 2, W // 2, C): the entries of every 2x2 window in POOL_WINDOW order."""
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    return np.stack([x[:, dy:2 * ho:2, dx:2 * wo:2, :] for dy, dx in POOL_WINDOW])


def maxpool2_ref(x):
    return pool_windows(x).max(axis=0)


def maxpool2_bwd_ref(x, dy):
    """dx: dy at the first maximum of each window in POOL_WINDOW order, 0 at the other three and in the row / column that VALID
    pooling drops."""
    win = pool_windows(x)
    first = np.argmax(win == win.max(axis=0), axis=0)          # (argmax returns the first True)
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    dx = np.zeros_like(x)
    for k, (oy, ox) in enumerate(POOL_WINDOW):
        dx[:, oy:2 * ho:2, ox:2 * wo:2, :] = np.where(first == k, dy, 0)
    return dx


def pool_tie_share(x):
    win = pool_windows(x)
    return float(((win == win.max(axis=0)).sum(axis=0) > 1).mean())


def pool_has_dead_window(x):
    """A window whose four entries are all <= 0."""
    return bool((pool_windows(x).max(axis=0) <= 0).any())


def pool_input(shape, relu):
    """hashed_small_ints with the first seed >= 1 at which the case has what it is there for: at least a quarter of the windows of
    the tensor the pooling reads (``relu``: max(x, 0)) hold their maximum more than once, and with ``relu`` at least one window of x
    is all <= 0.  tests/test_graph_ops_oracle.py checks both on every named case."""
    for seed in range(1, 1000):
        x = hashed_small_ints(shape, seed, zeros=relu)
        if pool_tie_share(np.maximum(x, 0) if relu else x) >= 0.25 and (not relu or pool_has_dead_window(x)):
            return x
    raise AssertionError(shape)
