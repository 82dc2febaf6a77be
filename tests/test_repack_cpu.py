"""CPU: the device repack's surface — pnrf_mlp_repack / pnrf_trainer_publish exported, declared and bound; the Python methods; the drivers' option;
and, without a device, the refusals that are decided on the host before anything is launched."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pnrf_mlp_repack', 'pnrf_trainer_publish')


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize('name', SYMBOLS)
def test_symbol_is_exported_declared_and_bound(lib, name):
    from pronerf_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pronerf_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+' + name + r'\s*\(', hdr)
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)                              # AttributeError if the library does not export it
    assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name][1])


def test_header_states_the_ordering_rule():
    hdr = open(os.path.join(ROOT, 'include', 'pronerf_hip.h')).read()
    doc = hdr[:hdr.index('int pnrf_mlp_repack(')].rsplit('/*', 1)[1]
    assert 'stream order' in doc and "caller's business" in doc and 'never synchronises' in doc


def test_python_surface():
    from pronerf_amd import ops, render
    from pronerf_amd.run_S_eS_eN_alter_base_refine2 import evaluate_views
    assert list(inspect.signature(ops.PackedMLP.repack).parameters) == ['self', 'weights', 'biases']
    assert list(inspect.signature(ops.Trainer.publish).parameters) == ['self', 'sampler', 'refine', 'fine']
    assert all(p.default is None for n, p in inspect.signature(ops.Trainer.publish).parameters.items() if n != 'self')
    assert list(inspect.signature(render.Renderer.publish_from).parameters) == ['self', 'trainer']
    assert inspect.signature(evaluate_views).parameters['path'].default == 'train'
    assert 'calibrate' in ops.Trainer.publish.__doc__ and 'calibrate' in render.Renderer.publish_from.__doc__


@pytest.mark.parametrize('variant', ['refine2', 'base'])
def test_testset_path_option(variant):
    from pronerf_amd.config import config_parser
    p = config_parser(variant)
    assert p.parse_args([]).testset_path == 'train'
    assert p.parse_args(['--testset_path', 'render']).testset_path == 'render'
    with pytest.raises(SystemExit):
        p.parse_args(['--testset_path', 'fast'])


def test_repack_sources_are_built_and_share_the_rules():
    from pronerf_amd import build
    assert 'pnrf_repack.hip' in build.SOURCES
    rules = open(os.path.join(build.CSRC, 'pnrf_pack_rules.h')).read()
    for fn in ('f2bf', 'f2h', 'wdbl', 'wval', 'split_h16', 'pack_lane', 'bias_val', 'fold6_elem', 'derive_elem', 'colnorm', 'mac_d'):
        assert re.search(r'PNRF_RULE [a-z0-9_ *]*\b' + fn + r'\(', rules), fn
    for src in ('pnrf_pack.hip', 'pnrf_repack.hip'):      # neither side states an element rule of its own
        text = open(os.path.join(build.CSRC, src)).read()
        assert 'pack_lane(' in text and not re.search(r'\b(f2bf|f2h|split_h16)\s*\([a-z]+ [a-z]', text), src


def test_new_kernels_do_not_spill(lib):
    from pronerf_amd import build
    ks = {n: v for n, v in build.device_kernels().items() if 'repack_' in n}
    assert len(ks) == 2, sorted(ks)
    assert all(v['scratch'] == 0 and v['mfma'] == 0 for v in ks.values()), ks


def test_null_arguments_are_refused_on_the_host(lib):
    assert lib.pnrf_mlp_repack(None, None, None, None, None, 0, None) == -1 and b'pnrf_mlp_repack: null argument' in lib.pnrf_last_error()
    assert lib.pnrf_trainer_publish(None, None, None, None, None) == -1 and b'pnrf_trainer_publish' in lib.pnrf_last_error()
