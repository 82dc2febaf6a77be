"""GPU: the compacted-column path of the NeRF stage (pnrf_ctx_set_nerf_skip).

Compositing multiplies a sample's alpha by relu(mul), mul an output of the sampler: a sample with mul <= 0 (or NaN) has weight exactly 0, and on
this path its network evaluation is skipped — a builder kernel lists the live columns, the MLP kernel runs over the list, a compositing pass follows.
The contract is bit identity of rgbd with the fused kernel, so every comparison here is ``torch.equal``; the live count is compared with the CPU oracle.
"""
import numpy as np
import pytest
import torch

from oracle import pronerf_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu

S = 8


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from pronerf_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def weights_of(kind):
    from pronerf_amd import synthetic
    return synthetic.load_trained_fixture(kind) if kind in ('pictures', 'scene3d') else synth.make_weights(0, kind)


def mul_rows():
    """Rows of the sampler's output layer that are ``mul``, read off the oracle's output map: a one-layer identity 'network' returns its input, so the
    values sampler_forward hands back as density_mul are the row numbers."""
    ident = {'W': [np.eye(4 * S, dtype=np.float32)], 'b': [np.zeros(4 * S, dtype=np.float32)]}
    _, _, mul, _ = orc.sampler_forward(ident, torch.arange(4 * S, dtype=torch.float32)[None], S)
    rows = mul[0].long().tolist()
    assert len(set(rows)) == S
    return rows


def constant_mul_weights(mul_values, kind='trained'):
    """``kind`` weights whose sampler emits the given 8 constants as mul on every ray (output-layer rows zeroed, biases set): each ray's mul_sorted is a
    permutation of them, so a call of n rays has exactly n * (number of positive values) live columns."""
    w = weights_of(kind)
    smp = {'W': [np.array(x, dtype=np.float32) for x in w['sampler']['W']], 'b': [np.array(x, dtype=np.float32) for x in w['sampler']['b']]}
    for r, v in zip(mul_rows(), mul_values):
        smp['W'][-1][r, :] = 0.0
        smp['b'][-1][r] = v
    return {**w, 'sampler': smp}


def renderer(weights, dev, H=40, W=52, shape=None, max_rays=None):
    """A frame of H x W rays over 24 x 32 neighbour views (the 24 x 32 scene holds 768 rays; the cases below need up to 2 080 and 9 000)."""
    from pronerf_amd.render import Renderer
    scene = synth.make_scene(0, H=H, W=W, Hf=24, Wf=32, rotate=True)
    rend = Renderer(weights, max_rays=max_rays or H * W, device=dev, shape=shape)
    rend.set_views(scene['c2w'], scene['poses'], scene['images'], scene['K'])
    rays, or_rays = rend.frame_rays(scene['K'], scene['c2w'], H, W)
    return rend, rays, or_rays, scene


def render(rend, rays, or_rays, n, mode):
    rend.ctx.set_nerf_skip(mode)
    out = rend.render_rays(rays[:n].contiguous(), or_rays[:n].contiguous())[0].clone()
    return out, rend.ctx.nerf_live()


@pytest.mark.parametrize('shape', ['wide', 'narrow'])
@pytest.mark.parametrize('kind', ['trained', 'default', 'spread', 'pictures'])
def test_forced_list_equals_forced_dense(dev, kind, shape):
    """Both NeRF forms (DoNeRFTRT: the three synthetic kinds; the NeRF class: the 'pictures' fixture), both workgroup shapes; the calls get smaller on one
    context, so every one after the first also proves that the builder's counters and the batch queue were re-armed."""
    rend, rays, or_rays, _ = renderer(weights_of(kind), dev, shape=shape)
    for n in (2080, 768, 33, 31, 1):
        lst, (live, list_mode) = render(rend, rays, or_rays, n, 'always')
        assert list_mode and 0 <= live <= n * S, (n, live, list_mode)
        dense, (live0, mode0) = render(rend, rays, or_rays, n, 'never')
        assert (live0, mode0) == (-1, False)
        print(f'{kind} {shape} n={n}: {live} of {n * S} columns live')
        assert torch.equal(lst, dense), (kind, shape, n, float((lst - dense).abs().max()))


def test_every_sample_dead_and_none_dead(dev):
    rend, rays, or_rays, _ = renderer(constant_mul_weights([-1.0] * S), dev)
    out, (live, list_mode) = render(rend, rays, or_rays, 2080, 'always')
    assert (live, list_mode) == (0, True)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) == 0.0
    assert torch.equal(out, render(rend, rays, or_rays, 2080, 'never')[0])
    rend, rays, or_rays, _ = renderer(constant_mul_weights([0.5 + 0.25 * s for s in range(S)]), dev)
    out, (live, list_mode) = render(rend, rays, or_rays, 2080, 'always')
    assert (live, list_mode) == (2080 * S, True)
    dense = render(rend, rays, or_rays, 2080, 'never')[0]
    assert torch.equal(out, dense) and float(dense[:, :3].max()) > 0.0


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_one_live_sample_per_ray(dev, n):
    """One open gate among the 8: a call of n rays has n live columns — exactly one in the whole call at n = 1, and one short of / exactly / one past a
    256-column batch."""
    rend, rays, or_rays, _ = renderer(constant_mul_weights([-1.0, -2.0, 0.75, -0.5, 0.0, -3.0, -1.5, -0.25]), dev)
    out, (live, list_mode) = render(rend, rays, or_rays, n, 'always')
    assert (live, list_mode) == (n, True)
    dense = render(rend, rays, or_rays, n, 'never')[0]
    assert torch.equal(out, dense) and float(dense[:, :3].max()) > 0.0


def test_nan_mul_counts_as_dead(dev):
    """The compositing takes fmaxf(mul, 0), which is 0 for a NaN: the builder's test ``mul > 0`` agrees."""
    rend, rays, or_rays, _ = renderer(constant_mul_weights([float('nan'), 1.0, -1.0, float('nan'), 0.5, 2.0, float('nan'), -0.0]), dev)
    out, (live, list_mode) = render(rend, rays, or_rays, 768, 'always')
    assert (live, list_mode) == (3 * 768, True)
    dense = render(rend, rays, or_rays, 768, 'never')[0]
    assert bool(torch.isfinite(dense).all())
    assert torch.equal(out, dense)


@pytest.mark.parametrize('kind', ['trained', 'default', 'spread'])
def test_live_count_matches_the_oracle(dev, kind):
    """The builder's count on the whole 24 x 32 frame (768 rays, 6 144 columns), three ways.

    1. Exactly, against a reference that sees the same values: the device sampler's own ``mul`` output from the operator-level call on the same rays
       (``ops.sampler_fwd(two_pass=True)`` runs the very kernels of the frame path, which are deterministic).  ``>=`` for ``>``, a sign slip or a NaN
       counted as live would show here, on every sample however close to zero.
    2. Against the fp32 oracle's sampler for the same rays (the count does not depend on the sort: mul_sorted is a permutation of mul per ray).  Seed 0
       keeps every oracle mul at least 1e-6 away from zero — asserted.  That margin alone does not separate the signs: the frame path's sampler evaluates
       most rays in plain fp16 (unit round-off 2^-11 through seven 256-wide layers), and on this frame of the 'trained' nets it differs from the oracle
       in one sample (5 567 against 5 568 live; the oracle's smallest |mul| there is 1.3e-4).  So, like the sort indices, the count is compared outside a
       tie set: the oracle samples within 2^-6 of the frame's largest |mul| of zero — 32 fp16 round-offs of the output scale — may fall either way, and
       the whole-frame count may differ from the oracle's by no more than their number.
    3. Exactly against the oracle on the rays that have no sample in that tie set."""
    from pronerf_amd import ops
    w = weights_of(kind)
    rend, rays, or_rays, scene = renderer(w, dev, H=24, W=32)
    n = 24 * 32
    fr = orc.frame_setup({**scene, 'H': 24, 'W': 32})
    np.testing.assert_array_equal(rays.cpu().numpy(), fr['rays'].numpy())
    _, _, mul, _ = orc.sampler_forward(w['sampler'], fr['mm_input'], S)
    assert float(mul.abs().min()) > 1e-6
    tie = mul.abs() <= float(mul.abs().max()) / 64
    want = int((mul > 0).sum())
    _, (live, list_mode) = render(rend, rays, or_rays, n, 'always')
    dev_mul = ops.sampler_fwd(rend.sampler, rays[:n].contiguous(), want_idx=False, want_rgb=False, two_pass=True)[3]
    dev_live = int((dev_mul > 0).sum())
    print(f'{kind}: whole frame {live} of {n * S} columns live, device sampler {dev_live}, oracle {want}, tie set {int(tie.sum())} samples')
    assert list_mode
    assert live == dev_live
    assert abs(live - want) <= int(tie.sum())
    clear = ~tie.any(1)
    m = int(clear.sum())
    assert m >= 64, m
    sel = clear.to(dev)
    _, (live, _) = render(rend, rays[sel], or_rays[sel], m, 'always')
    print(f'{kind}: {m} of 768 rays outside the tie set, {live} of {m * S} columns live')
    assert live == int((mul[clear] > 0).sum())


def test_auto_mode_engages_by_call_size_and_dead_share(dev):
    H, W = 90, 100                                                   # 9 000 rays: above PNRF_NERF_SKIP_MIN_RAYS = 8 192
    rend, rays, or_rays, _ = renderer(weights_of('default'), dev, H=H, W=W)
    out, (live, list_mode) = render(rend, rays, or_rays, H * W, 'auto')
    assert list_mode and 0 < live < H * W * S // 2, (live, list_mode)       # 'default' nets: 62 % of the samples dead
    assert torch.equal(out, render(rend, rays, or_rays, H * W, 'never')[0])
    _, (live, list_mode) = render(rend, rays, or_rays, 4096, 'auto')
    assert (live, list_mode) == (-1, False)                          # a small call does not take the path at all
    rend, rays, or_rays, _ = renderer(weights_of('scene3d'), dev, H=H, W=W)
    out, (live, list_mode) = render(rend, rays, or_rays, H * W, 'auto')
    assert not list_mode and live > H * W * S * 99 // 100, (live, list_mode)  # scene-trained nets: none dead (any break-even is a whole percent at least)
    assert torch.equal(out, render(rend, rays, or_rays, H * W, 'never')[0])
    _, (live, list_mode) = render(rend, rays, or_rays, 4096, 'auto')
    assert (live, list_mode) == (-1, False)


def test_large_call_in_a_graph(dev):
    """Four more launches and no host read: the call captures, and two replays give the eager result."""
    H, W = 90, 100
    rend, rays, or_rays, _ = renderer(weights_of('default'), dev, H=H, W=W)
    eager, (_, list_mode) = render(rend, rays, or_rays, H * W, 'auto')       # (also the context's first call on the path: allocates its workspace)
    assert list_mode
    out = torch.empty(H * W, 4, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rend.render_rays(rays, or_rays, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rend.render_rays(rays, or_rays, out=out)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_whole_frame_auto_equals_never(dev):
    """The 756 x 1008 frame of the benchmark's headline nets: auto mode takes the list path there and changes no bit."""
    rend, rays, or_rays, _ = renderer(weights_of('trained'), dev, H=756, W=1008)
    n = 756 * 1008
    auto, (live, list_mode) = render(rend, rays, or_rays, n, 'auto')
    print(f'headline frame: {live} of {n * S} columns live ({1 - live / (n * S):.1%} dead), list mode {list_mode}')
    assert list_mode
    assert torch.equal(auto, render(rend, rays, or_rays, n, 'never')[0])
