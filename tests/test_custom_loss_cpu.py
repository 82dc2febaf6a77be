"""CPU: training with a caller's loss — the three new entry points are declared, bound and exported and refuse bad arguments on the host;
the closed-form folding of all of raw2outputs' cotangents into the weights' (what pnrf_composite_bwd_maps adds in front of the colour-only
backward) is float64 autograd's; ``autograd.render_train`` does its bookkeeping (absent maps, normalised cotangents, one backward)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import custom_loss_ref as R
import exact_composite as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pnrf_composite_bwd_maps', 'pnrf_train_stage2_fwd', 'pnrf_train_stage2_bwd')


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_new_entry_points_are_declared_bound_and_exported(lib):
    from pronerf_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pronerf_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(pnrf_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'pnrf_train_maps_t' in hdr and 'pnrf_train_cotangents_t' in hdr
    # the structs of the binding have the header's eight pointers each, in the header's order
    order = ('rgb_map1', 'rgb_map0', 'mm_rgb', 'depth', 'acc', 'disp', 'weights', 'z')
    assert tuple(f[0] for f in _lib.TrainMaps._fields_) == order and C.sizeof(_lib.TrainMaps) == 8 * C.sizeof(C.c_void_p)
    assert tuple(f[0] for f in _lib.TrainCotangents._fields_) == tuple('d_' + k for k in order)
    m = re.search(r'typedef struct pnrf_train_maps \{(.*?)\}', hdr, flags=re.S)
    assert tuple(re.findall(r'\*(\w+)', m.group(1))) == order
    m = re.search(r'typedef struct pnrf_train_cotangents \{(.*?)\}', hdr, flags=re.S)
    assert tuple(re.findall(r'\*(\w+)', m.group(1))) == tuple('d_' + k for k in order)
    assert lib.pnrf_abi_version() == 1                          # additions only


def test_argument_checks_run_before_any_device_work(lib):
    null = [None] * 3
    args = lambda n: null + [3] + null + [0.0, 0] + [None] * 10 + [n, 8, None]
    assert lib.pnrf_composite_bwd_maps(*args(5)) == -1
    assert b'pnrf_composite_bwd_maps' in lib.pnrf_last_error()
    assert lib.pnrf_composite_bwd_maps(*args(0)) == 0           # empty input is a no-op
    assert lib.pnrf_train_stage2_fwd(None, None, None, None) == -1 and b'pnrf_train_stage2_fwd' in lib.pnrf_last_error()
    assert lib.pnrf_train_stage2_bwd(None, None, None) == -1 and b'pnrf_train_stage2_bwd' in lib.pnrf_last_error()


@pytest.mark.parametrize('oi', range(4))
@pytest.mark.parametrize('S', [1, 2, 8, 65])
def test_closed_form_folding_is_float64_autograd(S, oi):
    """All six cotangents random.  Left: autograd of the full objective.  Right: autograd of the colour and weight outputs ALONE, with the weights'
    cotangent and the extra z term that custom_loss_ref.fold computes from depth, acc, w and z.  Equal to 1e-12 relative per output tensor; on the
    rays where depth / acc is not finite or <= 1e-10, d_disp must have contributed nothing."""
    import inspect
    from pronerf_amd import ops
    # the helper's six cotangents are the public operator's, name for name and in its order (the GPU tests pass them through by these names)
    public = [p for p in inspect.signature(ops.composite_bwd_maps).parameters if p.startswith('d_')]
    assert public == ['d_rgb', 'd_disp', 'd_acc', 'd_weights', 'd_depth', 'd_z'] and len(R.COT) == len(public)
    inp = X.random_case(S, oi)
    n = inp['z'].shape[0]
    cot = R.random_cotangents(n, S, seed=7 * S + oi)
    _, o, _ = R.forward(inp)
    fwd = {k: v.detach().numpy() for k, v in o.items()}
    ok = R.disp_ok(fwd['depth'], fwd['acc'])
    if inp['mul'] is not None and S == 8:
        assert (~ok).any()                                      # rays that composite nothing exist in these sets
    full = R.autograd_ref(inp, cot)
    g_rgb, dws_extra, dz_extra = R.fold(fwd, inp['z'], cot, inp['white'])
    folded = R.autograd_ref(inp, dict(rgb=g_rgb, w=dws_extra, z_in=dz_extra))
    for k in full:
        err = np.linalg.norm(full[k] - folded[k]) / max(np.linalg.norm(full[k]), 1e-300)
        assert np.isfinite(full[k]).all() and err < 1e-12, (k, err)
    # d_disp on the excluded rays alone changes nothing
    only = dict(cot, disp=np.where(ok, 0, cot['disp']))
    a, b = R.fold(fwd, inp['z'], only, inp['white']), R.fold(fwd, inp['z'], dict(cot, disp=None), inp['white'])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


class _StubTrainer:
    """What render_train needs of a trainer, on the CPU: MAPS, anchor, forward, backward (one per forward)."""
    MAPS = {'rgb_map1': (3,), 'rgb_map0': (3,), 'mm_rgb': (3,), 'depth': (), 'acc': (), 'disp': (), 'weights': (8,), 'z': (8,)}

    def __init__(self, n):
        self.n, self.anchor, self.calls, self.open = n, torch.zeros((), requires_grad=True), [], False

    def forward(self, *args, want=None, **kw):
        self.args, self.kw, self.open = args, kw, True
        return {k: torch.arange(self.n * int(np.prod(self.MAPS[k], dtype=int)), dtype=torch.float32).reshape((self.n,) + self.MAPS[k]) / 10 for k in want}

    def backward(self, **cot):
        from pronerf_amd._lib import PnrfError
        if not self.open:
            raise PnrfError('pnrf_train_stage2_bwd failed (rc=-3): valid only as the next trainer call after pnrf_train_stage2_fwd')
        self.open = False
        self.calls.append(cot)


def test_render_train_bookkeeping():
    from pronerf_amd import autograd
    from pronerf_amd._lib import PnrfError
    n = 5
    tr = _StubTrainer(n)
    data = [torch.zeros(n, 11, requires_grad=True), torch.zeros(n, 11), torch.zeros(2, 4, 4, 4), torch.zeros(2, 3, 4), torch.eye(3), torch.zeros(n, 4, dtype=torch.int64)]
    maps = autograd.render_train(tr, *data, jitter_dir=-1, white_bkgd=True)
    assert list(maps) == list(tr.MAPS) and tr.kw['jitter_dir'] == -1 and tr.kw['white_bkgd'] is True and len(tr.args) == 6
    assert all(m.requires_grad for m in maps.values())
    # acc through a sum (an expanded, stride-0 cotangent), depth in float64 arithmetic, weights through a transposed view: three maps used, five not
    loss = maps['acc'].sum() + (maps['depth'].double() * 2).sum().float() + (maps['weights'].t() * torch.arange(n, dtype=torch.float32)).sum()
    loss.backward(retain_graph=True)
    assert len(tr.calls) == 1 and sorted(tr.calls[0]) == ['acc', 'depth', 'weights']          # unused maps are absent, not zeros
    for k, g in tr.calls[0].items():
        assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == (n,) + tr.MAPS[k] and not g.requires_grad, k
    assert torch.equal(tr.calls[0]['acc'], torch.ones(n)) and torch.equal(tr.calls[0]['depth'], torch.full((n,), 2.0))
    assert torch.equal(tr.calls[0]['weights'], torch.arange(n, dtype=torch.float32)[:, None].expand(n, 8))
    assert data[0].grad is None and tr.anchor.grad is None                                    # no gradient for the data arguments
    with pytest.raises(PnrfError, match='pnrf_train_stage2_fwd'):                             # one forward, one backward
        loss.backward()
    # a subset of the maps
    maps = autograd.render_train(tr, *data, want=('rgb_map1', 'z'))
    assert list(maps) == ['rgb_map1', 'z']
    maps['z'].mean().backward()
    assert sorted(tr.calls[-1]) == ['z']
