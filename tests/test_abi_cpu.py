"""CPU: the C-ABI library loads and exports every symbol include/pronerf_hip.h declares;
host-only helpers agree with torch; the sort network used by the sampler epilogue sorts."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from pronerf_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_header_symbols_exported(lib):
    from pronerf_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'pronerf_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(pnrf_[a-z0-9_]+)\s*\(', hdr))
    assert declared, 'no declarations parsed'
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pnrf_abi_version() == 1


def test_no_packed_fp32_instruction_in_any_kernel(lib):
    """Round 5 (NOTEBOOK §19): compiler-generated packed-fp32 arithmetic (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 / v_pk_mov_b32) returned wrong values in the
    fused refine epilogue whenever a workgroup of another fused kernel shared the CU; the library is built with that target feature off.  The guard: every
    gfx950 code object inside the built library is disassembled and must hold none of those opcodes — and the disassembly is a real one (MFMAs, LDS-DMA)."""
    from pronerf_amd import build
    assert build.NO_PACKED_FP32 == ['-Xclang', '-target-feature', '-Xclang', '-packed-fp32-ops'] and all(f in build.FLAGS for f in build.NO_PACKED_FP32)
    cos = build.device_code_objects()
    assert len(cos) >= 3, 'expected one gfx950 code object per translation unit with kernels'
    ops = build.device_opcodes()
    assert sum(ops.values()) > 100000 and ops['v_mfma_f32_16x16x32_bf16'] > 1000 and ops['global_load_lds_dwordx4'] > 100
    found = {k: ops[k] for k in build.PACKED_FP32_OPCODES if ops[k]}
    assert not found, f'packed fp32 instructions in the library: {found}'


def test_frame_path_kernels_do_not_spill_and_the_fern_instances_kept_their_size(lib):
    """Round 6 made the layer counts run-time arguments and templated the refine kernel on its views per lane half (the reference's free shape arguments).
    Guard of what that must not cost: no kernel of the inference frame path — any shape — uses scratch memory (a spill in a fused-MLP loop is a 10 % kernel),
    none exceeds the 256-register window two waves per SIMD leave, and the Fern instances still hold exactly the MFMAs of their layer bodies (a third
    layer body appeared in the dominant kernel while this was written: 594 -> 850 MFMAs, 229 -> 250 VGPRs) — and no frame kernel copies its operand
    registers around: the first run-time-count form of the NeRF stage kept the activations in one register set and moved 64 + 112 registers per pair of
    layers on the main path (1.5 % of the stage; found in the disassembly, not by a test: now there is one).  Its form today: two layer bodies + the
    output layer once per register set the activations can end in (594 + 18 MFMAs)."""
    from pronerf_amd import build
    k = build.device_kernels()
    assert len(k) > 80
    frame = {n: v for n, v in k.items() if n.startswith(('void sampler_p1_kernel', 'void sampler_h16_kernel', 'void sampler_kernel<2>', 'void nerf16_kernel', 'void refine16_kernel'))
             or ('refine_kernel<1, ' in n and ', 1, 1, PrecF16' in n)}
    assert len(frame) >= 4 + 8 + 5 + 8, sorted(frame)
    for n, v in frame.items():
        assert v['scratch'] == 0, (n, v)
        assert v['vgpr'] <= (512 if 'nerf16_kernel' in n and ', 4, PrecBf16, 4>' in n else 256), (n, v)      # (the 4 x 64-column NeRF shape owns a SIMD per wave)
        # register-to-register moves: the sort networks, the odd / even tails' out-of-line copies (<= 64 registers each) and the batch heads — never
        # hundreds (the copies named above: 272 in the 8-wave DoNeRFTRT kernel)
        assert v['vmov'] <= (420 if ', 4, PrecBf16, 4>' in n else 200), (n, v)
    # A WIDE fused workgroup (8 waves, two per SIMD) owns its SIMDs' register file: 256 VGPRs per wave in the kernel descriptor whatever the code uses
    # (own_the_simd, pnrf_mlp_kernels.hip).  With 240 + 240 allocated a small wave of another stream's kernel fits beside the pair, and in exactly that
    # configuration the refine stage returned wrong rows a few times in 10^4 calls (NOTEBOOK 22, tools/wide_repro.py); at 256 + 256 nothing can share the SIMD.
    wide = {n: v for n, v in k.items() if (n.startswith(('void sampler_p1_kernel<8>', 'void sampler_h16_kernel<8>', 'void sampler_kernel<')) or
                                           ('refine_kernel<1, 8,' in n) or ('refine16_kernel<8,' in n) or ('nerf16_kernel<' in n and n.endswith(', 8>(NerfArgs)')) or ('nerf_kernel<1, 8,' in n))}
    assert len(wide) >= 29, sorted(wide)          # 1 + 1 + 3 sampler, 18 refine + 4 refine16, 4 nerf16, 2 nerf (32x32x16) instances
    for n, v in wide.items():
        assert v['vgpr'] == 256, (n, v)
    fern = {'void sampler_p1_kernel<8>(SamplerArgs)': 424, 'void sampler_h16_kernel<8>(SamplerArgs)': 1248, 'void refine_kernel<1, 8, 1, 1, PrecF16, 2>(RefineArgs)': 472,
            'void nerf16_kernel<false, 2, PrecBf16, 8>(NerfArgs)': 594 + 18, 'void nerf16_kernel<true, 2, PrecBf16, 8>(NerfArgs)': 1578}
    for n, mfma in fern.items():
        assert n in k, (n, [x for x in k if x.split('<')[0] == n.split('<')[0]])
        assert k[n]['mfma'] == mfma, (n, k[n])
    assert k['void nerf16_kernel<false, 2, PrecBf16, 8>(NerfArgs)']['vmov'] <= 64, k['void nerf16_kernel<false, 2, PrecBf16, 8>(NerfArgs)']
    # every instance of the projecting refine stage: 8 tiles x (3 NV + 3) k-steps of layer 0 + three hidden-layer bodies + the output tile
    for nv in (1, 2, 3, 4):
        assert k[f'void refine_kernel<1, 8, 1, 1, PrecF16, {nv}>(RefineArgs)']['mfma'] == 8 * (3 * nv + 3) + 3 * 128 + 16


def test_linspace_matches_torch(lib):
    from pronerf_amd import ops
    for n in (1, 2, 7, 48, 64, 255):
        np.testing.assert_array_equal(ops.linspace(0.0, 1.0, n), torch.linspace(0, 1, n).numpy())
    # the exploration offsets (pnrf_explore_fwd; orc.explore_samples): torch.linspace(0, 1 - 1/n_mult, n_mult), every n_mult, signs too
    for n_mult in range(1, 33):
        a, b = ops.linspace(0.0, 1 - 1 / n_mult, n_mult), torch.linspace(0, 1 - 1 / n_mult, n_mult).numpy()
        np.testing.assert_array_equal(a, b, err_msg=f'n_mult={n_mult}')
        np.testing.assert_array_equal(np.signbit(a), np.signbit(b), err_msg=f'n_mult={n_mult}')


def test_argument_errors_are_reported(lib):
    from pronerf_amd import _lib
    rc = lib.pnrf_posenc_fwd(None, None, 5, 10, None)
    assert rc == -1
    assert b'pnrf_posenc_fwd' in lib.pnrf_last_error()
    with pytest.raises(_lib.PnrfError):
        _lib.check(rc, 'posenc')
    assert lib.pnrf_posenc_fwd(None, None, 0, 10, None) == 0      # empty input is a no-op
    # the trainer's operator-level entry point refuses a missing trainer before any device work (the other checks need one: test_exact_train_gpu.py)
    assert lib.pnrf_trainer_net_fwd_bwd(None, 0, None, None, 1, 1, None, None, None, None) == -1
    assert b'pnrf_trainer_net_fwd_bwd' in lib.pnrf_last_error()


def test_engine_images_are_validated_before_any_device_work(lib):
    """pnrf_mlp_deserialize refuses short / foreign / inconsistent images on the host (no GPU here, so reaching hipMalloc would fail
    differently); pnrf_mlp_serialize refuses null arguments."""
    import ctypes as C
    import struct
    h = C.c_void_p()
    assert lib.pnrf_mlp_deserialize(b'x' * 16, 16, C.byref(h)) == -1 and b'shorter than the header' in lib.pnrf_last_error()
    assert lib.pnrf_mlp_deserialize(b'\0' * 128, 128, C.byref(h)) == -1 and b'bad magic' in lib.pnrf_last_error()
    hdr = b'PNRFENG\0' + struct.pack('<IIII', 99, 1, 0, 16384) + b'\0' * 104
    assert lib.pnrf_mlp_deserialize(hdr, 128, C.byref(h)) == -3 and b'another build' in lib.pnrf_last_error()
    assert not h.value
    size = C.c_int64()
    assert lib.pnrf_mlp_serialize(None, None, 0, C.byref(size)) == -1
    assert lib.pnrf_mlp_kind(None, None, None, None, None) == -1


def test_cpu_tensors_are_refused():
    from pronerf_amd import ops, _lib
    with pytest.raises(_lib.PnrfError):
        ops.posenc(torch.zeros(4, 3), 10)


NETWORK = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (1, 2), (5, 6), (0, 4), (3, 7),
           (1, 5), (2, 6), (1, 4), (3, 6), (2, 4), (3, 5), (3, 4)]


def test_sort_network_is_a_sorting_network_and_stable_with_index_keys():
    src = open(os.path.join(ROOT, 'pronerf_amd', 'csrc', 'pnrf_mlp_kernels.hip')).read()
    pairs = [(int(a), int(b)) for a, b in re.findall(r'PNRF_CSWAP\((\d), (\d)\)', src)]
    assert pairs == NETWORK           # the kernel uses exactly the network verified here
    for bits in itertools.product((0, 1), repeat=8):      # zero-one principle
        v = list(bits)
        for i, j in NETWORK:
            if v[i] > v[j]:
                v[i], v[j] = v[j], v[i]
        assert v == sorted(v)
    rs = np.random.RandomState(0)
    for _ in range(2000):                                   # ties: (value, index) keys == stable sort
        vals = rs.randint(0, 4, 8).astype(np.float32)
        keys = [(float(vals[i]), i) for i in range(8)]
        for i, j in NETWORK:
            if keys[i] > keys[j]:
                keys[i], keys[j] = keys[j], keys[i]
        ref = torch.sort(torch.from_numpy(vals), stable=True)[1].tolist()
        assert [k[1] for k in keys] == ref
