"""GPU: the trainer's MLP forward and backward paths on integer nets (tests/exact_nets.py), where the answer is exact.

pnrf_trainer_net_fwd_bwd runs one net's forward and its backward from a chosen output gradient dy through the iterations' own dispatch
(preparation launch, product kind, engine / chain / per-layer path by row count, grouped weight gradients).  The iteration tests compare
against fp64 autograd within a noise factor, or against another kernel path of the library; a weight gradient that drops or doubles a
ragged row, a split-K partial summed twice or a skip-layer column shifted by one hides under those bounds.  Here it cannot.

Exactness (certified on the CPU by tests/test_exact_train_cpu.py for every input set used here; exact_nets.certify_*_train):
  * weights, biases, inputs and dy are integers; every forward activation and every backward dZ, dX = dZ W, dW = dZ^T X and db = sum dZ is
    an integer, and every dot product's sum of |terms| — forward, input gradient, and the weight-gradient reductions over ALL R rows — is below
    2^24, so fp32 accumulation is exact in any order and any split-K;
  * every operand the kernels split into fp16 hi + 2^-11 lo survives the split exactly at every power-of-two scale the kernel can choose
    (hg_scale_for of the tensor maximum, a row block's own maximum, the engine backward's per-row scale and the smallest per-layer factor its
    norm bound allows);
  * ReLU pre-activations that are exactly 0 occur (asserted on the CPU) and get derivative 0, torch's convention and the kernels' v > 0 masks;
    the ELU nets' pre-activations are >= 0, where ELU is the identity and ELU' = 1 (the kernels' act' from the saved output: 1 at 0).
So y, every dW / db of the net and d_pts are compared with assert_array_equal against torch autograd in float64 — except:

Weight-gradient columns that meet sin / cos of a non-zero coordinate (pts_linears.0 and the embedding columns of pts_linears.5: sin / cos of
the two non-live coordinates; views_linears.0: of the view directions' non-live components; exact_nets.NerfTrainRef.exact_cols).  There
dW[o, j] = sum_r dZ_r X_r with exact integer dZ_r and X_r = sinf / cosf of the kernel.  Componentwise (exact_nets.dw_inexact_bound):
  |got - ref| <= sum_r |dZ_r| e + (nnz + 132) 2^-24 sum_r |dZ_r| (|X_r| + e),   e = E_SIN + 2^-23,
with E_SIN = 2^-22 (sinf / cosf: <= 2 ulp of a value <= 1, a factor 2 kept) and 2^-23 the relative loss of the 22-bit hi / lo split of a value
<= 1; every fp32 addition of the reduction rounds by <= 2^-24 of a partial sum bounded by sum |terms|, and a reduction over R rows has at most
one rounding per nonzero term (nnz = rows where dZ != 0: zero terms add exactly) plus one per split-K partial (<= 128) and four in the
epilogues (hi / lo combine, unscale, the partials' sum, the store).  d_pts: the non-live coordinates' sin / cos columns carry zero weight in
pts0 and in the skip layer, so posenc_bwd adds cos(.) 0 - sin(.) 0 = 0 there; on the live coordinate cos 0 = 1 and sin 0 = 0, and the 2^k of
the chain rule are exact (exact_nets.nerf_dpts_exact_cols).  posenc_bwd then sums e_c + sum_k 2^k e_k over both embedding gradients in fp32:
exact where that sum of |terms| T (exact_nets.dpts_sums) is below 2^24; where the 2^9 of the top frequency lifts T past it, each of the 2 x 21
terms rounds at most three times and each of 42 additions once, all by <= 2^-24 T: |got - ref| <= 48 2^-24 T (exact_nets.dpts_bound).

Covered: products f16x2 (engine from 8192 rows), f16x2_unchained, f16x2_wchain, f32; dW tile 0, 64, 128, 256 from row 0 (wide grouped tiles,
dw_group_info asserted), 255 (wide off); row counts around 8192, ragged 128-row tails, 32 768, 65 536 and past the CU count; ELU nets across
the 16-row and 8192-row chain switches; d_pts given and NULL; one-hot and all-zero dy; state (a second call after a call with a huge dy, other
nets untouched, parameters rewritten); mutations of a hidden layer, the skip layer, a head and of dy, each asserted to fail.
"""
import numpy as np
import pytest
import torch

import exact_nets as E

pytestmark = pytest.mark.gpu

# (products, dW tile): set_dw_kernel(tile, 0) — 0 / 64 / 128: that weight-gradient kernel; 256: wide grouped tiles from the first row; 255: off
CONFIGS = [('f16x2', 0), ('f16x2', 256), ('f16x2', 255), ('f16x2', 64), ('f16x2', 128), ('f32', 0), ('f16x2_unchained', 0), ('f16x2_wchain', 0)]
L_S, L_R, L_N = 0, 7, 14
WIDE_JOBS = 0b0111111110           # engine backward's grouped jobs: views, feature, pts7 .. pts0; 256 x 128 tiles for those 256 wide with >= 128 inputs


@pytest.fixture(scope='module')
def dev():
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope='module')
def nets():
    return E.train_nets()


def _trainer(nets, max_rays, max_samples):
    from pronerf_amd import ops
    W, b = nets
    return ops.Trainer([np.float32(w) for w in W], [np.float32(v) for v in b], max_rays, max_samples=max_samples)


@pytest.fixture(scope='module')
def tr8(dev, nets):
    return _trainer(nets, E.TRAIN_MAX_RAYS, 8)


@pytest.fixture(scope='module')
def trbig(dev, nets):
    return _trainer(nets, *E.TRAIN_BIG)


def _g(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _configure(tr, products, tile):
    tr.set_products(products)
    if tile in (255, 256):
        tr.set_dw_kernel(0, 0)
        tr.set_dw_kernel(tile, 0)
    else:
        tr.set_dw_kernel(tile, 0)
        tr.set_dw_kernel(256, 32768)                   # the wide tiles' default threshold


def _grads(tr, layers):
    return [tuple(t.cpu().numpy() for t in tr.read('grad', li)) for li in layers]


# ----------------------------------------------------------------------------------------------- ELU nets
class _Elu:
    def __init__(self, nets, net, dev):
        W, b = nets
        self.first = L_S if net == 'sampler' else L_R
        self.W, self.b = W[self.first:self.first + 7], b[self.first:self.first + 7]
        self.net = net
        self.x = E.elu_inputs(max(E.ELU_COUNTS), self.W[0].shape[1])
        self.xg = _g(self.x, dev)
        self.cache = {}

    def case(self, n, dev, dy=None):
        key = (n, None if dy is None else dy.tobytes())
        if key not in self.cache:
            d = E.train_dy(n, self.W[-1].shape[0], seed=n) if dy is None else dy
            y, grads, _, _ = E.elu_train_reference(self.W, self.b, self.x[:n], d)
            self.cache[key] = (d, _g(d, dev), y, grads)
        return self.cache[key]


def _check_elu(tr, elu, n, dev, what, dy=None):
    d, dg, y, grads = elu.case(n, dev, dy)
    got, _ = tr.net_fwd_bwd(elu.net, elu.xg[:n], dg)
    np.testing.assert_array_equal(got.cpu().numpy(), y, err_msg=f'{what}: y')
    for l, (gW, gb) in enumerate(_grads(tr, range(elu.first, elu.first + 7))):
        np.testing.assert_array_equal(gW, grads[l][0], err_msg=f'{what}: dW of layer {l}')
        np.testing.assert_array_equal(gb, grads[l][1], err_msg=f'{what}: db of layer {l}')


@pytest.mark.parametrize('net', ['sampler', 'refine'])
def test_elu_net_exact(tr8, dev, nets, net):
    """Every product kind and dW kernel at N across the 16-row tiles, the 4096-row tile switch and the 8192 / 8193 chain switch."""
    elu = _Elu(nets, net, dev)
    try:
        for products, tile in CONFIGS:
            _configure(tr8, products, tile)
            for n in E.ELU_COUNTS:
                _check_elu(tr8, elu, n, dev, f'{net} {products} tile {tile} N={n}')
    finally:
        _configure(tr8, 'f16x2', 0)


# ----------------------------------------------------------------------------------------------- the fine net
class _Nerf:
    """One input set (S samples per ray, n rays) on the device, its float64 reference and the comparisons."""

    def __init__(self, nets, n, S, dev, certify=False):
        W, b = nets
        self.W = [np.asarray(w) for w in W[L_N:]]
        self.inp = E.nerf_inputs(n, live=E.TRAIN_LIVE, n_samples=S)
        self.ref = E.NerfTrainRef(W[L_N:], b[L_N:], self.inp)
        self.n, self.S, self.R = n, S, n * S
        self.pts = _g(self.inp['pts'].reshape(-1, 3), dev)
        self.rays = _g(self.inp['rays'], dev)
        self.dev = dev
        self.certify = certify
        self.cache = {}

    def expect(self, dy):
        key = dy.tobytes()
        if key not in self.cache:
            if self.certify:
                E.certify_nerf_train(self.ref, dy, f'R={self.R}')
            grads, dpts = self.ref.grads(dy)
            bounds = {l: E.dw_inexact_bound(self.ref, l, dy) for l in range(12) if not self.ref.exact_cols(l).all()}
            self.cache[key] = (_g(dy, self.dev), grads, dpts, bounds, E.dpts_sums(self.ref, dy))
        return self.cache[key]

    def check(self, tr, dy, what, want_dpts=False):
        dg, grads, dpts, bounds, T = self.expect(dy)
        y, dp = tr.net_fwd_bwd('nerf', self.pts, dg, rays=self.rays, S=self.S, want_dpts=want_dpts)
        np.testing.assert_array_equal(y.cpu().numpy(), self.ref.raw(), err_msg=f'{what}: raw')
        for l, (gW, gb) in enumerate(_grads(tr, range(L_N, L_N + 12))):
            ex = self.ref.exact_cols(l)
            np.testing.assert_array_equal(gW[:, ex], grads[l][0][:, ex], err_msg=f'{what}: dW of fine-net layer {l}')
            np.testing.assert_array_equal(gb, grads[l][1], err_msg=f'{what}: db of fine-net layer {l}')
            if not ex.all():
                assert np.all(np.isfinite(gW))
                err = np.abs(gW[:, ~ex].astype(np.float64) - grads[l][0][:, ~ex])
                bad = err > bounds[l][:, ~ex]
                assert not bad.any(), f'{what}: dW of fine-net layer {l}, sin / cos columns: {bad.sum()} entries over the bound (max err {err.max():.3g})'
        if want_dpts:
            got = dp.cpu().numpy()
            ex = E.nerf_dpts_exact_cols(self.W, self.ref)[None, :] & (T < E.ACC_MAX)
            np.testing.assert_array_equal(got[ex], dpts[ex], err_msg=f'{what}: d_pts')
            err = np.abs(got.astype(np.float64) - dpts)
            assert np.all(err <= E.dpts_bound(T)), f'{what}: d_pts off by {err.max():.3g} where its sums pass 2^24'


def _expect_wide(tr, products, tile, R):
    n_jobs, mask = tr.dw_group_info()
    assert n_jobs == 10, f'engine backward: {n_jobs} grouped weight gradients'
    wide = tile == 256 or (tile == 0 and R >= 32768)
    assert mask == (WIDE_JOBS if wide else 0), f'{products} tile {tile} R={R}: wide mask {mask:#x}'


def _run_nerf(tr, case, dy_seed, what, want_dpts):
    for products, tile in CONFIGS:
        _configure(tr, products, tile)
        dy = E.train_dy(case.R, 4, seed=dy_seed)
        case.check(tr, dy, f'{what} {products} tile {tile}', want_dpts=want_dpts)
        if products == 'f16x2' and tile in (0, 255, 256) and case.R >= 8192:
            _expect_wide(tr, products, tile, case.R)


@pytest.mark.parametrize('n', E.NERF_S8)
def test_nerf_exact_s8(tr8, dev, nets, n):
    """S = 8 (stage 2): below / at / above the 8192-row engine switch, ragged 128-row tails, 32 768 (wide tiles), 65 536 (wgs); d_pts given
    for most counts, NULL for the others."""
    case = _Nerf(nets, n, 8, dev)
    try:
        _run_nerf(tr8, case, n, f'S=8 n={n}', want_dpts=n % 2 == 1)
    finally:
        _configure(tr8, 'f16x2', 0)


@pytest.mark.parametrize('S,n', E.NERF_BIG)
def test_nerf_exact_many_samples(trbig, dev, nets, S, n):
    """S = 64 / 256 (stage-1 exploration: no position gradient): 8128 .. 65 792 rows."""
    case = _Nerf(nets, n, S, dev)
    try:
        _run_nerf(trbig, case, S + n, f'S={S} n={n}', want_dpts=False)
    finally:
        _configure(trbig, 'f16x2', 0)


def test_nerf_exact_past_cu_count(tr8, dev, nets, cus):
    """More 128-row batches than CUs (persistent engine workgroups take several), ragged last batch; certified here for this device."""
    n = E.nerf_cu_rays(cus)
    assert n * 8 > 128 * cus and n <= E.TRAIN_MAX_RAYS
    case = _Nerf(nets, n, 8, dev, certify=True)
    try:
        for products, tile in [('f16x2', 0), ('f16x2', 64), ('f16x2_wchain', 0)]:
            _configure(tr8, products, tile)
            case.check(tr8, E.train_dy(case.R, 4, seed=3), f'cus={cus} n={n} {products} tile {tile}', want_dpts=True)
    finally:
        _configure(tr8, 'f16x2', 0)


def test_nerf_onehot_rows(tr8, dev, nets):
    """dy zero except the first, the last and the rows on each side of a 128-row and a 32 768-row boundary: a dropped row leaves an exact
    zero, a doubled row twice the gradient."""
    S, n = E.NERF_ONEHOT
    case = _Nerf(nets, n, S, dev)
    rows = E.onehot_rows(case.R)
    assert {0, 127, 128, 32767, 32768, case.R - 1} <= set(rows)
    try:
        for products, tile in [('f16x2', 0), ('f16x2', 255), ('f16x2', 64), ('f32', 0), ('f16x2_unchained', 0)]:
            _configure(tr8, products, tile)
            for r in rows:
                dy = np.zeros((case.R, 4), np.float32)
                dy[r] = (1, -2, 3, 1)
                case.check(tr8, dy, f'one-hot row {r} {products} tile {tile}', want_dpts=True)
    finally:
        _configure(tr8, 'f16x2', 0)


def test_all_zero_dy(tr8, dev, nets):
    """dy = 0: every gradient exactly 0.0 and finite (hg_scale_for(0) = 1; the engine's row scale of a zero row stays 1)."""
    elu = _Elu(nets, 'refine', dev)
    for n in (8184, 8200):
        case = _Nerf(nets, n // 8, 8, dev)
        for products, tile in [('f16x2', 0), ('f16x2', 64), ('f32', 0)]:
            _configure(tr8, products, tile)
            case.check(tr8, np.zeros((case.R, 4), np.float32), f'zero dy R={n} {products}', want_dpts=True)
            for gW, gb in _grads(tr8, range(L_N, L_N + 12)):
                assert np.all(gW == 0) and np.all(gb == 0)
    _configure(tr8, 'f16x2', 0)
    for n in (16, 8193):
        _check_elu(tr8, elu, n, dev, f'refine zero dy N={n}', dy=np.zeros((n, 35), np.float32))


# ----------------------------------------------------------------------------------------------- state
def test_second_call_after_a_huge_gradient(tr8, dev, nets):
    """A call whose dy is ~2^60 leaves max-|gradient| values ~2^70 in the amax slots; were they not cleared, the next call would scale its
    integer gradients down by ~2^-58 and lose them in the fp16 planes.  The next call's answer is the exact one (= a fresh trainer's)."""
    elu = _Elu(nets, 'sampler', dev)
    for n in (1023, 1025):
        case = _Nerf(nets, n, 8, dev)
        dy = E.train_dy(case.R, 4, seed=11)
        huge = _g(np.ldexp(E.train_dy(case.R, 4, seed=12).astype(np.float64), 60), dev)
        tr8.net_fwd_bwd('nerf', case.pts, huge, rays=case.rays, S=8, want_dpts=True)
        case.check(tr8, dy, f'after a huge dy, R={case.R}', want_dpts=True)
    n = 4096
    d, dg, _, _ = elu.case(n, dev)
    tr8.net_fwd_bwd('sampler', elu.xg[:n], dg * 2.0 ** 60)
    _check_elu(tr8, elu, n, dev, 'sampler after a huge dy')
    fresh = _trainer(nets, 1025, 8)                        # the same answer from a trainer that never saw the huge call, bit for bit
    case = _Nerf(nets, 1025, 8, dev)
    dy = _g(E.train_dy(case.R, 4, seed=11), dev)
    a = fresh.net_fwd_bwd('nerf', case.pts, dy, rays=case.rays, S=8, want_dpts=True)
    ga = _grads(fresh, range(L_N, L_N + 12))
    b = tr8.net_fwd_bwd('nerf', case.pts, dy, rays=case.rays, S=8, want_dpts=True)
    gb = _grads(tr8, range(L_N, L_N + 12))
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u.cpu().numpy(), v.cpu().numpy())
    for (u1, u2), (v1, v2) in zip(ga, gb):
        np.testing.assert_array_equal(u1, v1); np.testing.assert_array_equal(u2, v2)


def test_one_net_leaves_the_others_alone(tr8, dev, nets):
    elu = _Elu(nets, 'refine', dev)
    case = _Nerf(nets, 1025, 8, dev)
    case.check(tr8, E.train_dy(case.R, 4, seed=5), 'fine net')
    _check_elu(tr8, elu, 4097, dev, 'refine')
    before = _grads(tr8, range(26))
    _check_elu(tr8, _Elu(nets, 'sampler', dev), 300, dev, 'sampler')
    after = _grads(tr8, range(26))
    for li in range(L_R, 26):
        np.testing.assert_array_equal(after[li][0], before[li][0]); np.testing.assert_array_equal(after[li][1], before[li][1])
    before = after
    case.check(tr8, E.train_dy(case.R, 4, seed=6), 'fine net again')
    after = _grads(tr8, range(26))
    for li in range(L_N):
        np.testing.assert_array_equal(after[li][0], before[li][0]); np.testing.assert_array_equal(after[li][1], before[li][1])


# ----------------------------------------------------------------------------------------------- mutations
def _mutated(W, seed=0):
    Wm = np.array(W, np.float64, copy=True)
    rs = np.random.RandomState(77 + seed)
    r, c = np.argwhere(Wm != 0)[rs.randint(np.count_nonzero(Wm))]
    Wm[r, c] += 1
    return Wm


def _visible(W, changes):
    """The first +1 mutation of W (seeds 0, 1, ...) that changes the float64 reference (an entry meeting only zero operands changes nothing)."""
    for seed in range(32):
        Wm = _mutated(W, seed)
        if changes(Wm):
            return Wm
    raise AssertionError('no visible +1 mutation')


def _same_nerf(a, b):
    return all(np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1]) for u, v in zip(a, b))


@pytest.mark.parametrize('layer,products', [(L_N + 3, 'f16x2'), (L_N + 5, 'f16x2'), (L_N + 11, 'f16x2'), (L_N + 9, 'f16x2_unchained'),
                                            (L_N + 5, 'f32'), (L_N + 10, 'f16x2_wchain')])
def test_mutation_nerf_weight(tr8, dev, nets, layer, products):
    """+1 on one weight (a hidden layer, the skip layer, the rgb / alpha heads, the view layer) through tr.write: the exact comparison fails;
    written back, it passes again (the planes / streams were refreshed both times)."""
    W, b = nets
    case = _Nerf(nets, 1025, 8, dev)
    dy = E.train_dy(case.R, 4, seed=21)
    g0, _ = case.ref.grads(dy)

    def changes(Wm):
        Ws = list(W[L_N:]); Ws[layer - L_N] = Wm
        ref = E.NerfTrainRef(Ws, b[L_N:], case.inp)
        return not np.array_equal(ref.raw(), case.ref.raw()) or not _same_nerf(ref.grads(dy)[0], g0)
    Wm = _visible(W[layer], changes)
    _configure(tr8, products, 0)
    try:
        case.check(tr8, dy, 'unmutated', want_dpts=True)
        tr8.write('param', layer, Wm.astype(np.float32), np.float32(b[layer]))
        with pytest.raises(AssertionError):
            case.check(tr8, dy, 'mutated', want_dpts=True)
    finally:
        tr8.write('param', layer, np.float32(W[layer]), np.float32(b[layer]))
        _configure(tr8, 'f16x2', 0)
    case.check(tr8, dy, 'restored', want_dpts=True)


@pytest.mark.parametrize('net,layer', [('sampler', 3), ('refine', 6)])
def test_mutation_elu_weight(tr8, dev, nets, net, layer):
    W, b = nets
    elu = _Elu(nets, net, dev)
    li = elu.first + layer
    d, _, y, grads = elu.case(4097, dev)

    def changes(Wm):
        Ws = list(elu.W); Ws[layer] = Wm
        y1, g1, _, _ = E.elu_train_reference(Ws, elu.b, elu.x[:4097], d)
        return not np.array_equal(y1, y) or not _same_nerf(g1, grads)
    Wm = _visible(W[li], changes)
    _check_elu(tr8, elu, 4097, dev, 'unmutated')
    try:
        tr8.write('param', li, Wm.astype(np.float32), np.float32(b[li]))
        with pytest.raises(AssertionError):
            _check_elu(tr8, elu, 4097, dev, 'mutated')
    finally:
        tr8.write('param', li, np.float32(W[li]), np.float32(b[li]))
    _check_elu(tr8, elu, 4097, dev, 'restored')


@pytest.mark.parametrize('n', [1025, 4101])
def test_mutation_dy_last_row(tr8, dev, nets, n):
    """+1 on one dy entry of the last row (a ragged 128-row batch): some weight gradient differs from the unmutated reference."""
    case = _Nerf(nets, n, 8, dev)
    dy = E.train_dy(case.R, 4, seed=31)
    case.check(tr8, dy, 'unmutated')
    dm = dy.copy()
    dm[-1, 1] += 1
    dg, grads, _, _, _ = case.expect(dy)
    tr8.net_fwd_bwd('nerf', case.pts, _g(dm, dev), rays=case.rays, S=8)
    got = _grads(tr8, range(L_N, L_N + 12))
    with pytest.raises(AssertionError):
        for l in range(12):
            ex = case.ref.exact_cols(l)
            np.testing.assert_array_equal(got[l][0][:, ex], grads[l][0][:, ex])
            np.testing.assert_array_equal(got[l][1], grads[l][1])


# ----------------------------------------------------------------------------------------------- arguments
def test_net_fwd_bwd_argument_errors(trbig, dev):
    from pronerf_amd import _lib
    import ctypes as C
    lib = _lib.load()
    h = trbig.handle
    x = torch.zeros(2048, 288, device=dev); dy = torch.zeros(2048, 35, device=dev); y = torch.zeros(2048, 35, device=dev)
    rays = torch.zeros(1024, 11, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    cases = [
        (3, p(x), None, 1, 1, p(dy), p(y), None, b'net must be'),
        (1, p(x), None, 1025, 0, p(dy), p(y), None, b'max_rays'),
        (1, p(x), None, 0, 0, p(dy), p(y), None, b'max_rays'),
        (1, None, None, 1, 0, p(dy), p(y), None, b'null pointer'),
        (1, p(x), None, 1, 0, None, p(y), None, b'null pointer'),
        (0, p(x), None, 1, 0, p(dy), p(y), p(x), b'd_pts belongs'),
        (2, p(x), None, 1, 8, p(dy), p(y), None, b'needs rays'),
        (2, p(x), p(rays), 1, 0, p(dy), p(y), None, b'outside [1, max_samples'),
        (2, p(x), p(rays), 1, 257, p(dy), p(y), None, b'outside [1, max_samples'),
        (2, p(x), p(rays), 1024, 16, p(dy), p(y), p(x), b'd_pts needs'),
    ]
    for net, xp, rp, n, S, dp, yp, dpts, msg in cases:
        assert lib.pnrf_trainer_net_fwd_bwd(h, net, xp, rp, n, S, dp, yp, dpts, None) == -1, msg
        assert msg in lib.pnrf_last_error(), (msg, lib.pnrf_last_error())
