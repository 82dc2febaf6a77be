"""LPIPS of one frame pair on the device against the only thing a user had before: the float32 restatement run eagerly in torch on the same GPU.

    python tools/lpips_bench.py [--H 756 --W 1008] [--nets alex,vgg] [--rounds 7] [--calls 3] [--out profiles/lpips.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/lpips_bench.py --calls-only      # a run of its own for the kernel split
    python tools/lpips_bench.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/lpips.json              # ... merged into the file

Seeded weights (conv N(0, 2 / fan_in), biases N(0, 0.05^2), lin uniform / C): times do not depend on the values.  Per round the two
implementations alternate in one process — ours, eager, eager again —, each timed by device events around ``calls`` back-to-back calls
after a warm-up; the medians over the rounds are reported, and the eager run against itself gives the spread a difference has to exceed.
FLOP counts are 2 M N K of every convolution for the pair, from the layer shapes.  Agreement with the lpips package on its real weights is
NOT measured here: neither the package nor its weights are part of this tree (DESIGN §4.8 has the lines to check it)."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (pool window in front of the conv, stride, padding) per conv layer; tap behind the layer or -1
GEOM = {'alex': [(0, 4, 2, 0), (3, 1, 2, 1), (3, 1, 1, 2), (0, 1, 1, 3), (0, 1, 1, 4)],
        'vgg': [(2 if i in (2, 4, 7, 10) else 0, 1, 1, {1: 0, 3: 1, 6: 2, 9: 3, 12: 4}.get(i, -1)) for i in range(13)]}


def make_net(net, seed=0):
    import torch
    from pronerf_amd import ops
    g = torch.Generator().manual_seed(seed)
    W = [torch.randn(s, generator=g) * (2.0 / (s[1] * s[2] * s[3])) ** 0.5 for s in ops.LPIPS_CONVS[net]]
    b = [torch.randn(s[0], generator=g) * 0.05 for s in ops.LPIPS_CONVS[net]]
    lin = [torch.rand(c, generator=g) / c for c in ops.LPIPS_LIN[net]]
    return W, b, lin


def eager(net, W, b, lin, x0, x1):
    """The definition in float32 with torch's own operators on the device (x0, x1: [H,W,3])."""
    import torch
    import torch.nn.functional as F
    x = torch.stack([x0, x1]).permute(0, 3, 1, 2)
    x = (2 * x - 1 - x.new_tensor([-.030, -.088, -.188])[None, :, None, None]) / x.new_tensor([.458, .448, .450])[None, :, None, None]
    d = 0
    for i, (pool, stride, pad, tap) in enumerate(GEOM[net]):
        if pool:
            x = F.max_pool2d(x, pool, 2)
        x = F.relu(F.conv2d(x, W[i], b[i], stride=stride, padding=pad))
        if tap >= 0:
            n = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + 1e-10)
            d = d + (lin[tap][:, None, None] * (n[0] - n[1]) ** 2).sum(0).mean()
    return d


def flops(net, H, W):
    from pronerf_amd import ops
    total, h, w = 0, H, W
    for (co, ci, k, _), (pool, stride, pad, _t) in zip(ops.LPIPS_CONVS[net], GEOM[net]):
        if pool:
            h, w = (h - pool) // 2 + 1, (w - pool) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        total += 2 * (2 * h * w) * co * (ci * k * k)
    return total


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def kernel_split(path):
    rows = [r for r in csv.DictReader(open(path)) if 'lpips_' in r['Name']]
    total = sum(int(r['TotalDurationNs']) for r in rows) or 1
    return [{'kernel': r['Name'].replace('(anonymous namespace)::', '').split('(')[0], 'calls': int(r['Calls']), 'total_ms': int(r['TotalDurationNs']) / 1e6,
             'share_of_lpips_kernels': int(r['TotalDurationNs']) / total} for r in sorted(rows, key=lambda r: -int(r['TotalDurationNs']))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--H', type=int, default=756)
    ap.add_argument('--W', type=int, default=1008)
    ap.add_argument('--nets', default='alex,vgg')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lpips.json'))
    ap.add_argument('--calls-only', action='store_true', help='only run the library calls (for a profiler run of its own); writes nothing')
    ap.add_argument('--kernel-stats', default=None, help="a rocprofv3 --kernel-trace --stats csv of a --calls-only run: merged into --out as 'kernel_split'")
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out))
        res['kernel_split'] = kernel_split(a.kernel_stats)
        json.dump(res, open(a.out, 'w'), indent=1)
        print(json.dumps(res['kernel_split']))
        return
    import torch
    from pronerf_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(1)
    x0 = torch.rand(a.H, a.W, 3, generator=g).to(dev)
    x1 = (0.6 * x0.cpu() + 0.4 * torch.rand(a.H, a.W, 3, generator=g)).to(dev)
    res = {'H': a.H, 'W': a.W, 'rounds': a.rounds, 'calls_per_round': a.calls, 'device': torch.cuda.get_device_name(0), 'nets': {},
           'not_measured': 'agreement with the lpips package on its real weights (neither is part of this tree)'}
    for net in a.nets.split(','):
        W, b, lin = make_net(net)
        sd = {f'features.{i}.weight': w for i, w in enumerate(W)}
        sd.update({f'features.{i}.bias': v for i, v in enumerate(b)})
        lp = ops.Lpips(net, sd, {f'lin{k}.weight': v for k, v in enumerate(lin)}, device=dev)
        ours = lambda: lp(x0, x1)
        if a.calls_only:
            for _ in range(1 + a.calls):
                ours()
            torch.cuda.synchronize()
            continue
        Wd, bd, lind = [[t.to(dev) for t in ts] for ts in (W, b, lin)]
        ref = lambda: eager(net, Wd, bd, lind, x0, x1)
        d_ours, d_ref = float(ours()), float(ref())                     # warm-up of both, and the two values
        t_ours, t_ref, t_ref2 = [], [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours, a.calls)); t_ref.append(timed(ref, a.calls)); t_ref2.append(timed(ref, a.calls))
        fl = flops(net, a.H, a.W)
        m_ours, m_ref, m_ref2 = (statistics.median(t) for t in (t_ours, t_ref, t_ref2))
        res['nets'][net] = {'ms': m_ours, 'ms_min_max': [min(t_ours), max(t_ours)], 'eager_ms': m_ref, 'eager_ms_min_max': [min(t_ref + t_ref2), max(t_ref + t_ref2)],
                            'eager_against_itself': m_ref2 / m_ref, 'ours_over_eager': m_ours / m_ref, 'conv_flop': fl, 'tflops': fl / m_ours / 1e9,
                            'eager_tflops': fl / m_ref / 1e9, 'd': d_ours, 'd_eager_float32': d_ref, 'rel_diff': abs(d_ours - d_ref) / abs(d_ref)}
        # the value against the float64 definition on the CPU at a small size, beside what float32 on the CPU gives (the tests hold every plane to it)
        s0, s1 = x0[:64, :80].contiguous(), x1[:64, :80].contiguous()
        on_cpu = lambda dt: float(eager(net, *[[t.to(dt) for t in ts] for ts in (W, b, lin)], s0.cpu().to(dt), s1.cpu().to(dt)))
        d64, d32, dk = on_cpu(torch.float64), on_cpu(torch.float32), float(lp(s0, s1))
        res['nets'][net]['error_check_64x80'] = {'d': dk, 'd_float64_cpu': d64, 'rel_error': abs(dk - d64) / abs(d64), 'rel_error_float32_cpu': abs(d32 - d64) / abs(d64)}
        print(net, json.dumps(res['nets'][net]), flush=True)
        del lp
    if not a.calls_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
