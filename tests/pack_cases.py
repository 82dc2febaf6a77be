"""The nets whose packed engine images tests/test_pack_image_cpu.py pins to the parent commit's bytes (and tests/pack_host_check.cpp packs by shape):
name -> (net kind, weights, biases).  Weights are the seeded numpy draws of pronerf_amd.synthetic (seed 3, 'trained'), deterministic on the CPU."""
import functools

from oracle import synth

NET_SAMPLER, NET_REFINE, NET_NERF, NET_NERFCLS = 0, 1, 2, 3
NETS = {'sampler': NET_SAMPLER, 'refine': NET_REFINE, 'nerf': NET_NERF}

# case -> (make_weights arguments, nets taken from the set)
SHAPES = {
    'fern': (dict(), ('sampler', 'refine', 'nerf')),                                                    # 48 points, depth 6, 4 views, netdepth 8
    'smallest': (dict(n_pts=1, mmnetdepth=2, num_neighbor=1, netdepth=3), ('sampler', 'refine', 'nerf')),
    'offfern': (dict(n_pts=32, mmnetdepth=8, num_neighbor=3, netdepth=5), ('sampler', 'refine', 'nerf')),
    'skip4': (dict(mmnetskips=[4]), ('sampler', 'refine')),
    'skip02': (dict(n_pts=5, mmnetdepth=4, num_neighbor=5, mmnetskips=[0, 2]), ('sampler', 'refine')),   # first and last allowed position, no unfolded sampler stream
    'deepest': (dict(mmnetdepth=32, num_neighbor=8), ('sampler', 'refine')),
}
for _nb in range(2, 9):      # views per lane half 1 .. 4 and both refine-16x16 widths (num_neighbor 1 is 'smallest')
    SHAPES[f'nb{_nb}'] = (dict(n_pts=1, mmnetdepth=2, num_neighbor=_nb, netdepth=3), ('refine',))

NAMES = [f'{c}-{n}' for c, (_, nets) in SHAPES.items() for n in nets] + ['nerfcls']


def cls_stack(wc):
    """NeRF-class weights in pack order: pts 0..7, feature, alpha, views, rgb."""
    order = list(wc['pts_linears']) + [wc['feature_linear'], wc['alpha_linear'], wc['views_linears'][0], wc['rgb_linear']]
    return [w for w, _ in order], [b for _, b in order]


@functools.lru_cache(maxsize=2)
def _weights(case):
    return synth.make_weights(3, 'trained', **SHAPES[case][0])


def case(name):
    """-> (net kind, list of W[out, in], list of b[out])"""
    if name == 'nerfcls':
        return (NET_NERFCLS,) + cls_stack(synth.make_nerfcls_weights(3))
    c, n = name.split('-')
    w = _weights(c)[n]
    return NETS[n], w['W'], w['b']
