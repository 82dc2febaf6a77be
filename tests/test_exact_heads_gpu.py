"""GPU: the trainer's head and positional-encoding kernels — sampler_head_fwd / bwd, refine_head_fwd / bwd, posenc_kernel, posenc_bwd —
against answers that are exact, and within a derived per-element bound of the float64 oracle elsewhere (tests/exact_heads.py).

Exact assertions (``assert_array_equal``):
  * all four head kernels on the dyadic exact set, whose replay tests/test_exact_heads_cpu.py certifies, in every option set (jitter
    absent / toward the next / toward the previous sample; d_z, d_rgb0, d_mm_rgb given or NULL), at 1 / 63 / 64 / 65 / 257 rays;
  * the forward heads on general origins, directions, depths and jitter around saturated y, against the float32 replay (ieee_* operations);
  * past the 4096-block cap (262 209 rays; 349 526 posenc rows) against the tiling of the small result;
  * posenc forward and backward at every x == 0, the copied x columns, the sampler's indices / add / mul, absent gradients' zero columns;
  * rays next to a NaN / Inf ray, and three runs of everything.
Bounded assertions: every output element of every kernel on general inputs, |got - ref| <= bound (exact_heads' docstring derives it).
"""
import functools

import numpy as np
import pytest
import torch

import exact_heads as H

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module')
def dev():
    from pronerf_amd import _lib
    _lib.load()
    yield torch.device('cuda:0')
    if WORST:
        print('\n[exact_heads] worst error / bound: ' + '   '.join(f'{k} {v:.3f}' for k, v in sorted(WORST.items())))


def cu(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def run(kernel, inp, dev, fwd=None, **kw):
    """One kernel through pronerf_amd.ops on an input set -> dict of numpy outputs.  fwd: dict(idx=, z_pre=) for the backward kernels."""
    from pronerf_amd import ops
    t = lambda k: cu(inp[k], dev)
    if kernel == 'sampler_fwd':
        out = dict(zip(('depth', 'idx', 'add', 'mul', 'rgb'), ops.sampler_head_fwd(t('y27'), t('rays'))))
    elif kernel == 'sampler_bwd':
        out = dict(dy=ops.sampler_head_bwd(t('y27'), t('rays'), cu(fwd['idx'], dev), t('s_gd'), t('s_ga'), t('s_gm'), t('s_gr') if kw['d_rgb'] else None))
    elif kernel == 'refine_fwd':
        j = kw['jdir']
        out = dict(zip(('z_pre', 'z', 'pts', 'rgb0'), ops.refine_head_fwd(t('y35'), t('rays'), t('D'), t('jitter') if j else None, j or 1)))
    elif kernel == 'refine_bwd':
        j = kw['jdir']
        dy, dD = ops.refine_head_bwd(t('y35'), t('rays'), t('D'), cu(fwd['z_pre'], dev), t('r_gp'), t('r_gz') if kw['d_z'] else None,
                                     t('r_gr') if kw['d_rgb0'] else None, t('jitter') if j else None, j or 1)
        out = dict(dy=dy, dD=dD)
    elif kernel == 'posenc_fwd':
        out = dict(out=ops.posenc(t('x'), inp['n_freq']))
    else:
        out = dict(dx=ops.posenc_bwd(t('x'), t('dE'), inp['n_freq']))
    return {k: v.cpu().numpy() for k, v in out.items()}


def forwards(inp, dev):
    """idx and z_pre of the kernels' own forwards (what the trainer hands to the backward kernels)."""
    return dict(idx=run('sampler_fwd', inp, dev)['idx'], z_pre=run('refine_fwd', inp, dev, jdir=0)['z_pre'])


@functools.lru_cache(maxsize=None)
def exact_set():
    """The dyadic set, its certified answers per (kernel, options) — pts from the float32 replay —, and the float32 forward state."""
    inp = H.exact_inputs()
    st = H.forward_state(inp)
    exp = {}
    for kernel, kw in H.head_cases():
        kwf = dict(kw, **H.saved(kernel, st))
        exp[kernel, tuple(kw.items())] = dict(H.certify(kernel, inp, taint_ok=('pts',), **kwf)[0], **({'pts': H.emulate(kernel, inp, **kwf)['pts']}
                                                                                                     if kernel == 'refine_fwd' else {}))
    return inp, st, exp


@functools.lru_cache(maxsize=None)
def free_set():
    inp = H.exact_inputs(free=True)
    return inp, {(k, tuple(kw.items())): H.emulate(k, inp, **kw) for k, kw in H.head_cases() if k in ('sampler_fwd', 'refine_fwd')}


@functools.lru_cache(maxsize=None)
def random_set():
    """The general set, the float64 references and the magnitudes per (kernel, options)."""
    inp = H.random_inputs()
    st = H.forward_state(inp)
    ref = {}
    for kernel, kw in H.head_cases():
        ref[kernel, tuple(kw.items())] = (H.reference(kernel, inp, **kw), H.magnitudes(kernel, inp, **dict(kw, **H.saved(kernel, st)))[1])
    return inp, ref


def assert_exact(got, exp, what):
    assert set(got) == set(exp)
    for k in exp:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=f'{k} {what}')


def assert_absent_zero(kernel, kw, got):
    if kernel == 'sampler_bwd' and not kw['d_rgb']:
        np.testing.assert_array_equal(got['dy'][:, 24:27], 0.0)
    if kernel == 'refine_bwd' and not kw['d_rgb0']:
        np.testing.assert_array_equal(got['dy'][:, 32:35], 0.0)


@pytest.mark.parametrize('n', H.NS)
def test_heads_exact(dev, n):
    """Every head kernel, every option set, on the first n rays of the exact sets: bit for bit."""
    inp, st, exp = exact_set()
    sub, fwd = H.head(inp, n), H.head(st, n)
    for kernel, kw in H.head_cases():
        got = run(kernel, sub, dev, fwd=fwd, **kw)
        assert_exact(got, H.head(exp[kernel, tuple(kw.items())], n), f'{kernel} {kw} n={n}')
        assert_absent_zero(kernel, kw, got)
    got = forwards(sub, dev)                                     # the backward kernels were fed what the forward kernels give
    assert_exact(got, fwd, f'forward state n={n}')
    inp, exp = free_set()
    for (kernel, kwt), e in exp.items():
        assert_exact(run(kernel, H.head(inp, n), dev, **dict(kwt)), H.head(e, n), f'{kernel} {kwt} n={n} (free)')


@pytest.mark.parametrize('n', H.NS)
def test_heads_bounded(dev, n):
    """General inputs: every output element within the derived bound of the float64 oracle and its autograd; indices, add and mul equal."""
    inp, ref = random_set()
    sub = H.head(inp, n)
    fwd = forwards(sub, dev)
    for kernel, kw in H.head_cases():
        r, mag = ref[kernel, tuple(kw.items())]
        got = run(kernel, sub, dev, fwd=fwd, **kw)
        ratio = H.ratios(kernel, got, H.head(r, n), H.head(mag, n), sub)
        WORST[kernel] = max(WORST.get(kernel, 0.0), max(ratio.values()))
        assert max(ratio.values()) <= 1, (kernel, kw, n, ratio)
        assert_absent_zero(kernel, kw, got)
        if kernel == 'sampler_fwd':
            for k in ('idx', 'add', 'mul'):
                np.testing.assert_array_equal(got[k], r[k][:n].astype(got[k].dtype), err_msg=k)


def test_heads_past_the_block_cap(dev):
    """262 209 rays: the grid is capped at 4096 blocks of 64 threads, so every thread takes a second ray and 65 threads a third.  The
    tiled exact set must give the tiling of the 257-ray result (and so the certified answers), forward and backward."""
    inp, st, exp = exact_set()
    big, fwd_big = H.tile(inp, H.N_CAP), H.tile(st, H.N_CAP)
    cases = [('sampler_fwd', {}), ('sampler_bwd', dict(d_rgb=True)), ('sampler_bwd', dict(d_rgb=False))]
    cases += [('refine_fwd', dict(jdir=j)) for j in (0, 1, -1)]
    cases += [('refine_bwd', dict(jdir=j, d_z=dz, d_rgb0=dr)) for j, dz, dr in ((0, True, True), (1, True, True), (-1, True, True), (1, False, False))]
    for kernel, kw in cases:
        small = run(kernel, inp, dev, fwd=st, **kw)
        got = run(kernel, big, dev, fwd=fwd_big, **kw)
        assert_exact(got, H.tile(small, H.N_CAP), f'{kernel} {kw} tiled')
        assert_exact(small, exp[kernel, tuple(kw.items())], f'{kernel} {kw}')
    inp, exp = free_set()
    big = H.tile(inp, H.N_CAP)
    for (kernel, kwt), e in exp.items():
        assert_exact(run(kernel, big, dev, **dict(kwt)), H.tile(e, H.N_CAP), f'{kernel} {kwt} tiled (free)')


def _x0(inp, a):
    return np.broadcast_to((inp['x'] == 0)[:, None, :], (a.shape[0], a.shape[1] // 3, 3)).reshape(a.shape)


@pytest.mark.parametrize('n_freq', H.PE_FREQS)
def test_posenc(dev, n_freq):
    """posenc forward and backward at 1 / 85 / 86 / 1000 rows: every element within the bound of the float64 oracle on both sets; on the
    exact set every element of an x == 0 bit for bit (0, 1; dE[c] + sum 2^k dE[sin_k]); the forward's x columns are copies."""
    for exact in (True, False):
        inp = H.posenc_inputs(n_freq=n_freq, exact=exact)
        ref = H.reference_posenc(inp)
        for kernel in ('posenc_fwd', 'posenc_bwd'):
            k = H.KEYS[kernel][0]
            _, mag = H.magnitudes(kernel, inp)
            exp, bad = H.certify(kernel, inp, taint_ok=(k,)) if exact else (None, None)
            for rows in H.PE_ROWS:
                sub = H.head(inp, rows)
                got = run(kernel, sub, dev)
                ratio = H.ratios(kernel, got, H.head(ref, rows), H.head(mag, rows), sub)
                WORST[kernel] = max(WORST.get(kernel, 0.0), ratio[k])
                assert ratio[k] <= 1, (kernel, n_freq, exact, rows, ratio)
                if kernel == 'posenc_fwd':
                    np.testing.assert_array_equal(got[k][:, :3], sub['x'])
                if exact:
                    z = _x0(sub, got[k])
                    assert not bad[k][:rows][z].any()
                    np.testing.assert_array_equal(got[k][z], exp[k][:rows][z], err_msg=f'{kernel} n_freq={n_freq} rows={rows} at x == 0')


def test_posenc_past_the_block_cap(dev):
    """349 526 rows = 1 048 578 scalars at n_freq = 10: the grid is capped at 4096 blocks of 256 threads, two threads take a second
    scalar.  The tiled 1000-row set gives the tiling of the 1000-row result, forward and backward, bit for bit."""
    inp = H.posenc_inputs(n_freq=10, exact=True)
    big = H.tile(inp, H.PE_CAP_ROWS)
    assert big['x'].size > 4096 * 256
    for kernel in ('posenc_fwd', 'posenc_bwd'):
        assert_exact(run(kernel, big, dev), H.tile(run(kernel, inp, dev), H.PE_CAP_ROWS), kernel)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_heads_non_finite_inputs_stay_in_their_ray(dev):
    """A NaN depth logit in one ray, a NaN jitter in another, +-Inf gradients in a third: every other ray's outputs keep the bits of the
    clean run, the NaN ray's sort indices are still a permutation of 0..7 (where the NaN sorts is not promised), and three runs agree."""
    clean, _ = random_set()
    inp = {k: v.copy() for k, v in clean.items()}
    r1, r2, r3 = 70, 135, 200
    inp['y27'][r1, 3] = np.nan; inp['y35'][r1, 2] = np.nan
    inp['jitter'][r2, 4] = np.nan
    inp['s_gd'][r3, 1] = np.inf; inp['s_ga'][r3, 6] = -np.inf; inp['r_gp'][r3, 2, 1] = -np.inf; inp['r_gz'][r3, 5] = np.inf
    keep = np.ones(H.N_SET, bool); keep[[r1, r2, r3]] = False
    runs = []
    for rep in range(3):
        outs = {}
        for which, data in (('clean', clean), ('poisoned', inp)):
            fwd = forwards(data, dev)
            for kernel, kw in H.head_cases():
                outs[which, kernel, tuple(kw.items())] = run(kernel, data, dev, fwd=fwd, **kw)
        runs.append(outs)
    for key, got in runs[0].items():
        for k, v in got.items():
            for other in runs[1:]:
                np.testing.assert_array_equal(_bits(v), _bits(other[key][k]), err_msg=f'{key} {k}: runs differ')
            if key[0] == 'poisoned':
                np.testing.assert_array_equal(_bits(v)[keep], _bits(runs[0][('clean',) + key[1:]][k])[keep], err_msg=f'{key} {k}: another ray changed')
    idx = runs[0]['poisoned', 'sampler_fwd', ()]['idx']
    assert (np.sort(idx, 1) == np.arange(8)).all()
    assert np.isnan(runs[0]['poisoned', 'sampler_fwd', ()]['depth'][r1]).any() and np.isnan(runs[0]['poisoned', 'refine_fwd', (('jdir', 1),)]['z'][r2]).any()
