"""CPU: the generator of the device-resident training set's draws (pnrf_train_batch_fwd).  tests/batch_ref.py restates it in numpy; here that
restatement meets the published known answers, the library's own Philox code (the host entry point pnrf_philox4x32_10 runs the function the kernel
runs) meets it too, the row / quad counter rule is consistent under a row0 split, the draws have the statistics of a standard normal — and the new
unit's kernels keep to the library's rules (no scratch), the option exists in both training parsers, and argument errors are reported on the host."""
import ctypes as C

import numpy as np
import pytest

import batch_ref as R

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers_numpy_restatement(ctr, key, want):
    assert tuple(int(x) for x in R.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers_library(lib, ctr, key, want):
    out = (C.c_uint32 * 4)()
    assert lib.pnrf_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
    assert tuple(out) == want
    assert lib.pnrf_philox4x32_10(None, None, out) == -1


def test_library_philox_equals_the_restatement_on_random_counters(lib):
    rs = np.random.RandomState(0)
    ctr = rs.randint(0, 2 ** 32, (64, 4), dtype=np.uint64)
    key = rs.randint(0, 2 ** 32, 2, dtype=np.uint64)
    want = R.philox4x32_10([ctr[:, i] for i in range(4)], key)
    out = (C.c_uint32 * 4)()
    for i in range(64):
        lib.pnrf_philox4x32_10((C.c_uint32 * 4)(*[int(x) for x in ctr[i]]), (C.c_uint32 * 2)(*[int(x) for x in key]), out)
        assert tuple(out) == tuple(int(x) for x in want[i])


def test_unit_map_is_exact_in_fp32_and_strictly_inside_the_unit_interval():
    x = np.array([0, 1, 511, 512, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
    u = R.unit(x)
    assert (u.astype(np.float32).astype(np.float64) == u).all()
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24


@pytest.mark.parametrize('C_', [8, 16])
def test_row0_split_reproduces_the_unsplit_rows(C_):
    for stream in (0, 1):
        whole = R.words(100, C_, seed=5, step=3, stream=stream)
        part = R.words(40, C_, seed=5, step=3, stream=stream, row0=60)
        np.testing.assert_array_equal(whole[60:], part)
    np.testing.assert_array_equal(R.normals(100, 8, 5, 3, 1)[60:], R.normals(40, 8, 5, 3, 1, row0=60))
    assert not np.array_equal(R.words(4, 8, seed=5, step=3), R.words(4, 8, seed=5, step=4))
    assert not np.array_equal(R.words(4, 8, seed=5, step=3), R.words(4, 8, seed=6, step=3))
    assert not np.array_equal(R.words(4, 8, seed=5, step=3, stream=0), R.words(4, 8, seed=5, step=3, stream=1))
    assert not np.array_equal(R.words(4, 8, seed=5), R.words(4, 8, seed=5 + 2 ** 32))             # the seed's high word is part of the key


@pytest.mark.parametrize('seed,step', [(0, 1), (20240611, 7)])
def test_draw_statistics(seed, step):
    n, C_ = 2 ** 17, 8
    N = n * C_
    z0 = R.normals(n, C_, seed, step, R.STREAM_JITTER)
    z1 = R.normals(n, C_, seed, step, R.STREAM_NOISE)
    for z in (z0, z1):
        print(f'seed {seed} step {step}: mean {z.mean():.3e} (bound {5 / np.sqrt(N):.3e}), var - 1 {z.var() - 1:.3e} (bound {5 * np.sqrt(2 / N):.3e})')
        assert abs(z.mean()) <= 5 / np.sqrt(N)
        assert abs(z.var() - 1) <= 5 * np.sqrt(2 / N)
    j = R.jitter(n, C_, R.CAP_STAGE2, seed, step)
    assert abs(j.mean() - np.sqrt(2 / np.pi) / 5) <= 1e-3
    assert j.max() <= R.CAP_STAGE2 and j.min() >= 0
    corr = float(np.corrcoef(z0.reshape(-1), z1.reshape(-1))[0, 1])
    assert abs(corr) <= 5 / np.sqrt(N)


def test_batch_kernels_use_no_scratch_and_rank_shares_one_statement(lib):
    import os
    from pronerf_amd import build
    k = build.device_kernels()
    mine = {n: v for n, v in k.items() if any(t in n for t in ('scene_rank_table_kernel', 'train_batch_rows_kernel', 'train_batch_draws_kernel'))}
    assert len(mine) == 3, sorted(mine)
    for n, v in mine.items():
        assert v['scratch'] == 0 and v['vgpr'] <= 128 and v['mfma'] == 0, (n, v)
    assert 'pnrf_batch.hip' in build.SOURCES
    # the counting rule is written once (pnrf_scene_impl.h) and called by both ranking kernels
    csrc = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), 'csrc')
    rule = 'o == d && u < v'
    holders = sorted(f for f in os.listdir(csrc) if rule in open(os.path.join(csrc, f), encoding='utf-8').read())
    assert holders == ['pnrf_scene_impl.h'], holders
    for f in ('pnrf_scene.hip', 'pnrf_batch.hip'):
        assert 'scene_rank_views(' in open(os.path.join(csrc, f), encoding='utf-8').read(), f


def test_argument_errors_come_before_any_device_work(lib):
    """No GPU here: a call that reached the device would fail with a hipError (> 0), these return PNRF_E_ARG."""
    order = (C.c_int * 4)(0, 1, 2, 3)
    assert lib.pnrf_train_batch_fwd(None, None, None, 1, order, 0., 1., 1., 10., None, None, None, None, None, 0, 0, 0, None, 0, 0., None, 0, 0., None) == -1
    assert b'pnrf_train_batch_fwd' in lib.pnrf_last_error()
    assert lib.pnrf_scene_rank_table_fwd(None, None, None) == -1
    assert lib.pnrf_scene_arrays(None, None, None, None, None) == -1
    h = C.c_void_p()
    assert lib.pnrf_scene_create(6, 2, 2, 1, C.byref(h)) == 0                # a U8 scene is refused, an incomplete F32 scene is a state error
    assert lib.pnrf_scene_arrays(h, None, None, None, None) == -1 and b'PNRF_SCENE_F32' in lib.pnrf_last_error()
    lib.pnrf_scene_free(h)
    assert lib.pnrf_scene_create(6, 2, 2, 0, C.byref(h)) == 0
    assert lib.pnrf_scene_arrays(h, None, None, None, None) == -3
    assert lib.pnrf_scene_rank_table_fwd(h, None, None) == -3
    lib.pnrf_scene_free(h)


@pytest.mark.parametrize('variant', ['refine2', 'base'])
def test_device_batches_option(variant):
    from pronerf_amd.config import config_parser
    a = config_parser(variant).parse_args([])
    assert a.device_batches == 'off' and a.batch_seed == 0
    a = config_parser(variant).parse_args(['--device_batches', 'all', '--batch_seed', '77'])
    assert a.device_batches == 'all' and a.batch_seed == 77
    with pytest.raises(SystemExit):
        config_parser(variant).parse_args(['--device_batches', 'some'])
    assert not hasattr(config_parser('trt').parse_args([]), 'device_batches')
