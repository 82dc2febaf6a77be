"""Reference side of the PNG encoder's tests: plain numpy / zlib / PIL, nothing of the library.

* ``parse``: the chunks of a file with every CRC checked by ``zlib.crc32``, the IDAT inflated by ``zlib.decompress`` (which checks the Adler-32);
* ``unfilter`` / ``refilter``: this file's own statement of the five PNG filters and of the adaptive rule (smallest sum of |residual as int8|,
  ties to the lowest type), so the filter byte of every row is known exactly;
* ``reference_size``: zlib level 6, strategy Z_RLE, one full flush per ``segment_rows`` rows, on the encoder's own filtered bytes;
* ``parent_file``: what ``_write_png`` of the driver writes for the same pixels;
* ``cases``: the images both test files run.
"""
import io
import struct
import zlib

import numpy as np

SIG = b'\x89PNG\r\n\x1a\n'


def parse(data):
    """-> dict(W, H, channels, filtered = the inflated IDAT bytes, zdata, chunks = [(tag, payload)])."""
    assert data[:8] == SIG, 'signature'
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, f'CRC of {tag}'
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data) and [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND'] and chunks[2][1] == b''
    W, H, depth, ctype, comp, flt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, comp, flt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 1 if ctype == 0 else 3
    z = chunks[1][1]
    filtered = zlib.decompress(z)                                   # raises on a bad stream or Adler-32
    assert len(filtered) == H * (W * ch + 1)
    assert struct.unpack('>I', z[-4:])[0] == zlib.adler32(filtered) & 0xffffffff
    return dict(W=W, H=H, channels=ch, filtered=filtered, zdata=z, chunks=chunks)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _shift(row, bpp):
    out = np.zeros_like(row)
    out[bpp:] = row[:-bpp] if bpp < len(row) else row[:0]
    return out


def residuals(row, prev, bpp):
    """The five filtered forms of a row (int arrays 0 .. 255) given the row above (zeros for the first)."""
    row, prev = row.astype(np.int64), prev.astype(np.int64)
    a, c = _shift(row, bpp), _shift(prev, bpp)
    preds = [np.zeros_like(row), a, prev, (a + prev) // 2, _paeth(a, prev, c)]
    return [((row - p) & 255).astype(np.uint8) for p in preds]


def refilter(img, filter=-1):
    """Filtered bytes of a uint8 image [H,W] / [H,W,3] by the rule; filter -1 adaptive, 0 .. 4 forced."""
    H = img.shape[0]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    rows = img.reshape(H, -1)
    out = []
    for y in range(H):
        prev = rows[y - 1] if y else np.zeros_like(rows[0])
        cand = residuals(rows[y], prev, bpp)
        if filter < 0:
            cost = [int(np.abs(r.view(np.int8).astype(np.int64)).sum()) for r in cand]
            t = cost.index(min(cost))
        else:
            t = filter
        out.append(bytes([t]) + cand[t].tobytes())
    return b''.join(out)


def unfilter(filtered, H, W, ch):
    """The pixels [H, W*ch] of filtered bytes."""
    rb = W * ch
    f = np.frombuffer(filtered, np.uint8).reshape(H, rb + 1)
    out = np.zeros((H, rb), np.int64)
    for y in range(H):
        t, r = int(f[y, 0]), f[y, 1:].astype(np.int64)
        prev = out[y - 1] if y else np.zeros(rb, np.int64)
        assert 0 <= t <= 4
        if t == 0:
            out[y] = r
        elif t == 2:
            out[y] = (r + prev) & 255
        else:
            for x in range(rb):
                a = out[y, x - ch] if x >= ch else 0
                b = prev[x]
                c = prev[x - ch] if x >= ch else 0
                p = a if t == 1 else (a + b) // 2 if t == 3 else int(_paeth(np.int64(a), np.int64(b), np.int64(c)))
                out[y, x] = (r[x] + p) & 255
    return out.astype(np.uint8)


def reference_size(filtered, row_bytes, segment_rows):
    """Bytes of the zlib stream of the reference scheme: level 6, Z_RLE, a full flush behind every ``segment_rows`` rows."""
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    step, n = row_bytes * segment_rows, 0
    for lo in range(0, len(filtered), step):
        n += len(co.compress(filtered[lo:lo + step]))
        n += len(co.flush(zlib.Z_FULL_FLUSH if lo + step < len(filtered) else zlib.Z_FINISH))
    return n


def huffman_depths(counts):
    """Leaf depths of an unconstrained Huffman tree of the counts (heap construction; any tie order: the callers' counts leave the depth no choice)."""
    import heapq
    h = [(c, i, [i]) for i, c in enumerate(counts)]
    heapq.heapify(h)
    depth, k = [0] * len(counts), len(counts)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for i in a[2] + b[2]:
            depth[i] += 1
        heapq.heappush(h, (a[0] + b[0], k, a[2] + b[2]))
        k += 1
    return depth


def first_block_header(z):
    """The first deflate block of a zlib stream: dict(btype, ll = literal / length code lengths, dist, cl = the code-length code's lengths by symbol,
    cl_freq = how often each of the 19 code-length symbols is used to write the lengths)."""
    pos = [16]

    def bits(n):
        v = 0
        for k in range(n):
            v |= ((z[pos[0] >> 3] >> (pos[0] & 7)) & 1) << k
            pos[0] += 1
        return v
    bits(1)
    btype = bits(2)
    if btype != 2:
        return dict(btype=btype)
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl = [0] * 19
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][:hclen]:
        cl[s] = bits(3)
    code, table = 0, {}
    for n in range(1, 8):
        for s in range(19):
            if cl[s] == n:
                table[(n, code)] = s
                code += 1
        code <<= 1
    lens, freq = [], [0] * 19
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while (n, c) not in table:
            c, n = c << 1 | bits(1), n + 1
            assert n <= 7, 'code-length code'
        s = table[(n, c)]
        freq[s] += 1
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits(2))
        else:
            lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
    assert len(lens) == hlit + hdist
    return dict(btype=2, ll=lens[:hlit], dist=lens[hlit:], cl=cl, cl_freq=freq)


def chain_counts(start, n):
    """Counts, ascending, whose Huffman tree is a chain above ``start``: every further count exceeds the sum of all but the one before it."""
    w = list(start)
    while len(w) < n:
        w.append(sum(w[:-1]) + 1)
    return w


def deep_segment(counts, S):
    """A gray image of ONE segment (S rows) whose bytes under filter 0 have the histogram ``counts`` (ascending; the first entry is the end-of-block
    symbol's 1 and takes no pixel), the rest of the pixels going to the most frequent value.  That value is 0, the filter bytes' value, and no two
    neighbours are equal: no match forms, the symbols' histogram is the bytes'.  -> (image, the symbols' counts)"""
    w = list(counts[1:])
    assert len(w) <= 200
    W = -(-int(sum(w) * 1.06) // (2 * S)) * 2
    w[-1] += S * W - sum(w)
    assert w[-2] < w[-1] <= S * W // 2
    values = np.r_[(np.arange(1, len(w)) * 13 % 251 + 1), 0].astype(np.uint8)            # distinct, 0 for the last (251 is prime)
    assert len(set(values.tolist())) == len(w)
    vals = np.repeat(values, w)[::-1]                                                     # most frequent first
    flat = np.empty(S * W, np.uint8)
    flat[0::2], flat[1::2] = vals[:S * W // 2], vals[S * W // 2:]
    return flat.reshape(S, W), [1] + w[:-1] + [w[-1] + S]


def deep_cases(S):
    """{name: (counts, wanted unconstrained depth)}: segment-local histograms whose Huffman tree is deeper than the 15-bit limit."""
    out = {f'depth{d}': (chain_counts([1, 1], d + 1), d) for d in (17, 18, 19, 20)}
    n = 5
    while max(huffman_depths(chain_counts([1, 1, 1, 1], n))) < 17:                       # bushy: four leaves at depth 17 under two roots at depth 16
        n += 1
    out['bushy17'] = (chain_counts([1, 1, 1, 1], n), 17)
    return out


def cl_deep_image(S):
    """A gray image of ONE segment (S x 512, filter 0) whose literal code lengths 3, 5, 6, 8, 9, 11, 12, 13 belong to 4, 6, 10, 16, 26, 42, 91, 1 pixel
    values: the counts are dyadic (a value of length l occurs 2^(13 - l) times; Kraft sum 1 with the end-of-block symbol at length 13), so the
    Huffman lengths are those.  No two neighbouring values have the same length and the unused values are one run, so the code-length symbols that
    write the lengths occur 1 (the zero run), 2 (the distance lengths), 2, 4, 6, 10, 16, 26, 42, 91 times: each more than all but the one before it
    together, a chain 9 deep against that code's limit of 7."""
    n_len = {3: 4, 5: 6, 6: 10, 8: 16, 9: 26, 11: 42, 12: 91, 13: 1}
    assert sum(n << (13 - l) for l, n in n_len.items()) + 1 == 1 << 13
    rest = dict(n_len)
    rest[3] -= 1                                                                                     # value 0, the filter bytes' value, has length 3
    pool = [l for l, n in sorted(rest.items(), key=lambda kv: -kv[1]) for _ in range(n)]              # most frequent length first
    lens = [0] * len(pool)
    half = -(-len(pool) // 2)
    lens[0::2], lens[1::2] = pool[:half], pool[half:]
    lens = [3] + lens
    assert all(a != b for a, b in zip(lens, lens[1:]))
    order = sorted(range(len(lens)), key=lambda v: lens[v])                                          # the values by descending count
    counts = [1 << (13 - lens[v]) for v in order]
    assert order[0] == 0
    counts[0] += S * 512 - sum(counts)                                                               # the pixel the end-of-block symbol leaves over
    vals = np.repeat(np.array(order, np.uint8), counts)
    flat = np.empty(S * 512, np.uint8)
    flat[0::2], flat[1::2] = vals[:S * 256], vals[S * 256:]
    return flat.reshape(S, 512)


def parent_file(img):
    """The bytes ``_write_png`` writes: filter type 0 on every row, zlib.compress level 6."""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    rows = np.ascontiguousarray(img).reshape(h, w * ch)
    raw = b''.join(b'\x00' + rows[i].tobytes() for i in range(h))

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    return SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, {1: 0, 3: 2}[ch], 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b'')


def decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def scene_views(H=189, W=252, seed=3):
    """(rgb uint8 [H,W,3], depth uint8 [H,W]) of a ``llff_synth.Scene3D`` view, 8-bit as the driver writes them."""
    import llff_synth
    p35 = np.array([[1., 0, 0, 0.05, H], [0, 1., 0, -0.03, W], [0, 0, 1., 0.02, llff_synth.FOCAL_PER_WIDTH * W]])
    rgb, depth = llff_synth.Scene3D(seed).render(p35, H, W, llff_synth.FOCAL_PER_WIDTH * W, ss=1)
    to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)
    return to8b(rgb.astype(np.float32)), to8b((depth / np.max(depth)).astype(np.float32))


def runs_image(value, lengths, W, other=None):
    """A gray image of width W: runs of ``value`` of the given lengths, each followed by one byte that differs."""
    rng = np.random.RandomState(7)
    flat = []
    for n in lengths:
        flat += [value] * n + [int(other if other is not None else (value + 1 + rng.randint(200)) % 256)]
    flat += [value ^ 0x55] * (-len(flat) % W)
    return np.array(flat, np.uint8).reshape(-1, W)


def cases(segment_rows):
    """[(name, image, filter)]: the images of the issue's list.  filter None = adaptive and every forced type are all run by the CPU test; the GPU
    test takes 'adaptive' unless a filter is named."""
    rng = np.random.RandomState(11)
    S = segment_rows
    out = []
    for h, w in ((1, 1), (1, 2), (2, 1)):
        out.append((f'gray{h}x{w}', rng.randint(0, 256, (h, w)).astype(np.uint8), None))
        out.append((f'rgb{h}x{w}', rng.randint(0, 256, (h, w, 3)).astype(np.uint8), None))
    for w in range(1, 10):
        smooth = (np.add.outer(np.arange(3) * 9, np.arange(w) * 5)[..., None] + np.array([0, 40, 90])).astype(np.uint8)
        out.append((f'rgb3x{w}', smooth, None))
        out.append((f'gray3x{w}', smooth[..., 1].copy(), None))
    for h in (S - 1, S, S + 1, 2 * S + 1):
        y, x = np.mgrid[0:h, 0:21]
        out.append((f'rows{h}', ((x * 7 + y * 3) % 256).astype(np.uint8), None))
        out.append((f'rows{h}rgb', np.stack([(x * 2 + y) % 256, (x + y * 5) % 256, (x * y) % 256], -1).astype(np.uint8), None))
    out.append(('noise64x33', rng.randint(0, 256, (64, 33, 3)).astype(np.uint8), None))
    out.append(('zero64x33', np.zeros((64, 33), np.uint8), None))
    out.append(('zero64x33rgb', np.zeros((64, 33, 3), np.uint8), None))
    out.append(('runs_short', runs_image(9, [1, 2, 3, 4, 257, 258, 259, 260, 261, 262], 97), 0))
    out.append(('runs_258k', runs_image(200, [258 * k + r for k in (1, 2, 3, 17) for r in (0, 1, 2, 3)], 1031), 0))
    out.append(('runs_adaptive', runs_image(0, [258 * k + r for k in (1, 2) for r in (0, 1, 2, 3)], 300), None))
    out.append(('two_valued', np.where(rng.rand(40, 57) < 0.3, 17, 240).astype(np.uint8), None))
    out.append(('uniform', rng.randint(0, 256, (50, 301)).astype(np.uint8), 0))
    # forced depth: value counts 1, 1, 2, 4, ..., 2^16 in 256 x 512 = 2^17 pixels: an unconstrained Huffman tree is 17 deep
    counts = [1] + [1 << k for k in range(17)]
    vals = np.repeat(np.arange(18, dtype=np.uint8) * 13 + 5, counts)
    assert vals.size == 256 * 512
    out.append(('forced_depth', rng.permutation(vals).reshape(256, 512), 0))
    # ... and the same inside ONE segment (the codes are per segment), segment_rows x 512 pixels: with the end-of-block symbol's count of 1 in front,
    # every count exceeds the sum of all but the one before it, so the Huffman tree is a chain (17 deep); the most frequent value is 0, the filter
    # bytes' value; no two neighbours are equal, so no match forms and the histogram of the symbols is the histogram of the bytes
    # (deep_cases: chains 17 .. 20 deep and a bushy tree with four leaves at depth 17)
    for name, (counts, _) in deep_cases(S).items():
        out.append((name, deep_segment(counts, S)[0], 0))
    # a frame-sized image of geometric noise (ratio 0.55), adaptive filter: every segment's histogram falls off over many octaves
    out.append(('geometric_frame', np.minimum(np.random.RandomState(1).geometric(0.45, (756, 1008, 3)) - 1, 255).astype(np.uint8), None))
    out.append(('cl_deep', cl_deep_image(S), 0))
    rgb, depth = scene_views()
    out.append(('scene_rgb', rgb, None))
    out.append(('scene_depth', depth, None))
    return out
