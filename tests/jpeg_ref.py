"""Test infrastructure for the JPEG encoder and the Motion-JPEG writer, numpy and pure Python, written from the format rules (baseline JPEG, ITU T.81;
the rules as DESIGN §4.8.3 lists them), not from the C++:

* ``coefficients``: colour conversion, edge replication, the 13-bit scaled integer DCT, quantisation, zigzag — the statement in int64;
* ``decode``: a decoder of the entropy stream: parses the markers, builds the Huffman codes from the file's own DHT, undoes stuffing, follows DRI
  and RSTm, returns the quantised coefficients and event counts (ZRL runs, blocks without EOB, stuffed bytes, the largest DC and AC category);
* ``riff_walk``: a walker of RIFF files for the AVI tests;
* ``cases``: the images of the tests, the smallest shapes at which each mechanism can go wrong."""
import collections
import struct

import numpy as np

# Annex K.1 / K.2, row-major
LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def zigzag():
    """Row-major index of each zigzag position: anti-diagonals in turn, odd ones downwards (row ascending), even ones upwards."""
    order = sorted(((r, c) for r in range(8) for c in range(8)), key=lambda rc: (rc[0] + rc[1], rc[0] if (rc[0] + rc[1]) % 2 else rc[1]))
    return np.array([8 * r + c for r, c in order])


ZZ = zigzag()


def qtable(which, quality):
    """IJG scaling of the Annex K table (0: luminance, 1: chrominance), row-major, entries 1 .. 255."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(CHROMA if which else LUMA, np.int64) * s + 50) // 100, 1, 255)


def ycc(img):
    """[H,W,3] uint8 RGB -> int64 Y, Cb, Cr 0 .. 255: full-range BT.601, 16-bit fixed point."""
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], -1)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, up):
    """One 1-D pass over the last axis (8 values): the 12-multiplication flow graph with constants round(c 2^13); outputs 0 and 4 scaled by 2^up,
    the others descaled by 13 - up bits."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - up
    o = [None] * 8
    o[0], o[4] = ((t10 + t11) << up, (t10 - t11) << up) if up >= 0 else (_descale(t10 + t11, -up), _descale(t10 - t11, -up))
    e = (t12 + t13) * 4433
    o[2], o[6] = _descale(e + t13 * 6270, n), _descale(e - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    b1, b2, b3, b4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = _descale(a4 + b1 + b3, n), _descale(a5 + b2 + b4, n), _descale(a6 + b2 + b3, n), _descale(a7 + b1 + b4, n)
    out = np.stack(o, -1)
    assert np.abs(out).max(initial=0) < 2 ** 31 and all(np.abs(v).max(initial=0) < 2 ** 31 for v in (e, z5, a4, a5, a6, a7, b1, b2, b3, b4))      # 32-bit intermediates
    return out


def coefficients(img, quality):
    """uint8 [H,W] or [H,W,3] -> int64 [MCU rows, MCU columns, components, 64]: the quantised coefficients in zigzag order."""
    planes = img.astype(np.int64)[..., None] if img.ndim == 2 else ycc(img)
    H, W, ch = planes.shape
    planes = np.pad(planes, ((0, -H % 8), (0, -W % 8), (0, 0)), mode='edge') - 128
    R, Cc = planes.shape[0] // 8, planes.shape[1] // 8
    blocks = planes.reshape(R, 8, Cc, 8, ch).transpose(0, 2, 4, 1, 3)                  # [R, C, ch, y, x]
    rows = _pass(blocks, 2)                                                              # along x
    both = _pass(rows.swapaxes(-1, -2), -2).swapaxes(-1, -2)                             # along y
    q = np.stack([qtable(1 if c else 0, quality) for c in range(ch)]).reshape(1, 1, ch, 8, 8) * 8
    quant = np.sign(both) * ((np.abs(both) + q // 2) // q)
    return quant.reshape(R, Cc, ch, 64)[..., ZZ]


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------------------
NAMES = {0xd8: 'SOI', 0xe0: 'APP0', 0xdb: 'DQT', 0xc0: 'SOF0', 0xc4: 'DHT', 0xdd: 'DRI', 0xda: 'SOS', 0xd9: 'EOI'}


class _Bits:
    """MSB-first reader of one interval's unstuffed bytes."""

    def __init__(self, data):
        self.data, self.n, self.pos = data, 8 * len(data), 0

    def take(self, k):
        assert self.pos + k <= self.n, 'the interval ends inside a symbol'
        v = 0
        while k:
            byte, used = self.data[self.pos >> 3], self.pos & 7
            m = min(k, 8 - used)
            v = v << m | ((byte >> (8 - used - m)) & ((1 << m) - 1))
            self.pos += m
            k -= m
        return v


def _symbol(bits, table):
    code = 0
    for length in range(1, 17):
        code = code << 1 | bits.take(1)
        if (length, code) in table:
            return table[(length, code)]
    raise AssertionError('no code of the table matches')


def _extend(v, n):
    return v if n == 0 or v >> (n - 1) else v - (1 << n) + 1


def decode(data):
    """The file's structure and quantised coefficients.  Returns a dict: markers (names in order), H, W, channels, qtables {id: 64 zigzag entries},
    dht {(class, id): (counts, symbols)}, dri, rst (the m of every RSTm in order), coefficients [MCU rows, MCU cols, channels, 64] int64, and
    events: stuffed, zrl_runs (Counter: length of a run of consecutive ZRL symbols -> how often), no_eob, max_dc_category, max_ac_category,
    intervals.  Asserts everything a baseline decoder relies on."""
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
    markers, qt, dht, pos, info = ['SOI'], {}, {}, 2, {}
    while True:
        assert data[pos] == 0xff, f'no marker at {pos}'
        m, n = data[pos + 1], struct.unpack('>H', data[pos + 2:pos + 4])[0]
        body = data[pos + 4:pos + 2 + n]
        assert len(body) == n - 2
        markers.append(NAMES.get(m, hex(m)))
        if m == 0xe0:
            assert body == b'JFIF\0\x01\x01\0\0\x01\0\x01\0\0'
        elif m == 0xdb:
            assert len(body) % 65 == 0
            for k in range(0, len(body), 65):
                assert body[k] in (0, 1)                          # 8-bit entries, table 0 or 1
                qt[body[k]] = list(body[k + 1:k + 65])
        elif m == 0xc0:
            assert body[0] == 8
            info['H'], info['W'], info['channels'] = struct.unpack('>HH', body[1:5]) + (body[5],)
            assert len(body) == 6 + 3 * body[5]
            info['comp_q'] = []
            for c in range(body[5]):
                cid, samp, tq = body[6 + 3 * c:9 + 3 * c]
                assert cid == c + 1 and samp == 0x11
                info['comp_q'].append(tq)
        elif m == 0xc4:
            k = 0
            while k < len(body):
                counts = list(body[k + 1:k + 17])
                syms = list(body[k + 17:k + 17 + sum(counts)])
                dht[(body[k] >> 4, body[k] & 15)] = (counts, syms)
                k += 17 + sum(counts)
            assert k == len(body)
        elif m == 0xdd:
            info['dri'] = struct.unpack('>H', body)[0]
        elif m == 0xda:
            assert body[0] == info['channels'] and tuple(body[-3:]) == (0, 63, 0)
            info['comp_h'] = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
            assert [body[1 + 2 * c] for c in range(body[0])] == list(range(1, body[0] + 1))
            pos += 2 + n
            break
        else:
            raise AssertionError(f'unexpected marker {m:02x}')
        pos += 2 + n
    tables = {}
    for key, (counts, syms) in dht.items():
        t, code, i = {}, 0, 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                t[(length, code)] = syms[i]
                code += 1
                i += 1
            assert code <= 1 << length
            code <<= 1
        tables[key] = t
    # entropy data: undo stuffing, cut at RSTm
    scan, intervals, rst, cur, stuffed, i = data[pos:-2], [], [], bytearray(), 0, 0
    while i < len(scan):
        if scan[i] != 0xff:
            cur.append(scan[i]); i += 1
            continue
        assert i + 1 < len(scan), 'FF at the end of the entropy data'
        nxt = scan[i + 1]
        if nxt == 0:
            cur.append(0xff); stuffed += 1
        else:
            assert 0xd0 <= nxt <= 0xd7, f'marker {nxt:02x} inside the entropy data'
            rst.append(nxt - 0xd0); intervals.append(bytes(cur)); cur = bytearray()
        i += 2
    intervals.append(bytes(cur))
    H, W, ch = info['H'], info['W'], info['channels']
    R, Cc = -(-H // 8), -(-W // 8)
    assert info['dri'] == Cc and len(intervals) == R and rst == [k % 8 for k in range(R - 1)]
    coef = np.zeros((R, Cc, ch, 64), np.int64)
    zrl_runs, no_eob, max_dc, max_ac = collections.Counter(), 0, 0, 0
    for r, chunk in enumerate(intervals):
        bits, pred = _Bits(chunk), [0] * ch
        for c in range(Cc):
            for comp in range(ch):
                td, ta = info['comp_h'][comp]
                s = _symbol(bits, tables[(0, td)])
                assert s <= 11
                max_dc = max(max_dc, s)
                pred[comp] += _extend(bits.take(s), s)
                coef[r, c, comp, 0] = pred[comp]
                k, zrl = 1, 0
                while k < 64:
                    rs = _symbol(bits, tables[(1, ta)])
                    run, s = rs >> 4, rs & 15
                    if s == 0:
                        if run == 15:
                            k += 16; zrl += 1
                            assert k < 64, 'ZRL past the block'
                            continue
                        assert run == 0 and zrl == 0, 'ZRL in front of EOB'
                        break
                    if zrl:
                        zrl_runs[zrl] += 1
                        zrl = 0
                    k += run
                    assert k < 64 and s <= 10
                    max_ac = max(max_ac, s)
                    coef[r, c, comp, k] = _extend(bits.take(s), s)
                    k += 1
                else:
                    no_eob += 1
        left = bits.n - bits.pos
        assert left < 8 and bits.take(left) == (1 << left) - 1, 'an interval ends with fewer than 8 bits, all 1'
    info.update(markers=markers + ['EOI'], qtables=qt, dht=dht, rst=rst, coefficients=coef, header_bytes=pos,
                events=dict(stuffed=stuffed, zrl_runs=zrl_runs, no_eob=no_eob, max_dc_category=max_dc, max_ac_category=max_ac, intervals=R))
    return info


# ---- RIFF ---------------------------------------------------------------------------------------------------------------------------------------------
def riff_walk(data):
    """[(path, offset of the chunk's tag, body offset, size)] of every chunk, lists included ('RIFF:AVI /LIST:hdrl/avih').  Asserts that every chunk
    lies inside its parent and that odd-sized chunks are followed by a pad byte inside the parent."""
    out = []

    def walk(lo, hi, path):
        p = lo
        while p < hi:
            assert p + 8 <= hi, f'chunk header at {p} leaves {path}'
            tag, size = data[p:p + 4], struct.unpack('<I', data[p + 4:p + 8])[0]
            assert p + 8 + size + (size & 1) <= hi, f'{tag} at {p} with {size} bytes leaves {path or "the file"}'
            if tag in (b'RIFF', b'LIST'):
                name = path + '/' * bool(path) + tag.decode() + ':' + data[p + 8:p + 12].decode()
                out.append((name, p, p + 12, size - 4))
                walk(p + 12, p + 8 + size, name)
            else:
                out.append((path + '/' + tag.decode(), p, p + 8, size))
                if size & 1:
                    assert data[p + 8 + size] == 0
            p += 8 + size + (size & 1)
        assert p == hi

    walk(0, len(data), '')
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------------
def idct_image(blocks, quality):
    """A gray image, one row of 8 x 8 blocks, whose quantised coefficients at ``quality`` are the given ones: blocks = [{zigzag position: level}].
    The pixels are 128 + the rounded inverse DCT of level x table entry; tables of 10 and more keep the rounding (below 0.5 a pixel) far from the
    quantiser's thresholds."""
    q = qtable(0, quality)
    u = np.arange(8)
    basis = np.cos((2 * u[None, :] + 1) * u[:, None] * np.pi / 16) * np.where(u == 0, np.sqrt(1 / 8), 0.5)[:, None]      # [frequency, position]
    img = np.zeros((8, 8 * len(blocks)))
    for i, levels in enumerate(blocks):
        F = np.zeros(64)
        for k, v in levels.items():
            F[ZZ[k]] = v * q[ZZ[k]]
        img[:, 8 * i:8 * i + 8] = 128 + basis.T @ F.reshape(8, 8) @ basis
    assert img.min() >= 0 and img.max() <= 255
    return np.round(img).astype(np.uint8)


ZRL_QUALITY = 50
ZRL_BLOCKS = [{0: 2, 17: 2}, {0: -1, 1: 1, 35: -2}, {0: 3, 50: 1}, {0: 1, 2: -1, 63: 1}, {0: 1, 20: 1, 40: -1}]      # 1, 2, 3 ZRL; 3 ZRL and no EOB; none


def cases():
    """[(name, image, quality)]: gray and RGB of each shape and content of the list."""
    rng = np.random.RandomState(23)
    out = []

    def both(name, gray, quality=90, rgb=None):
        out.append((name + '_gray', gray, quality))
        out.append((name + '_rgb', rgb if rgb is not None else np.stack([gray, np.roll(gray, 1, 1), 255 - gray], -1), quality))

    smooth = lambda H, W: np.clip(128 + 90 * np.sin(np.arange(W)[None, :] / 3.1 + np.arange(H)[:, None] / 2.3) + rng.randint(-9, 10, (H, W)), 0, 255).astype(np.uint8)
    for H, W in ((1, 1), (7, 9), (8, 8), (9, 17), (72, 16), (8, 2056)):      # edges replicated; RSTm wraps past 7; 257 blocks in a row
        both(f'{H}x{W}', smooth(H, W))
    both('constant', np.full((16, 24), 77, np.uint8), rgb=np.full((16, 24, 3), (200, 30, 77), np.uint8))
    yy, xx = np.mgrid[0:24, 0:32]
    both('checker', (((yy // 12 + xx // 8) % 2) * 255).astype(np.uint8), 100)                        # 8 wide: whole blocks of 0 and 255 side by side; 12 tall: edges inside blocks
    both('noise', rng.randint(0, 256, (64, 64)).astype(np.uint8), 100, rgb=rng.randint(0, 256, (64, 64, 3)).astype(np.uint8))
    z = idct_image(ZRL_BLOCKS, ZRL_QUALITY)
    both('zrl', z, ZRL_QUALITY, rgb=np.stack([z, z, z], -1))
    wide = rng.randint(0, 256, (21, 40)).astype(np.uint8)
    wide3 = rng.randint(0, 256, (21, 40, 3)).astype(np.uint8)
    both('strided', wide[:, :33], 75, rgb=wide3[:, :33])                                             # a view: row pitch 40 (120) for 33 (99) bytes
    import png_ref
    rgb, depth = png_ref.scene_views(189, 252)
    out.append(('scene_gray', depth, 90))
    out.append(('scene_rgb', rgb, 90))
    return out


def case_names():
    return [f'{n}_{k}' for n in ('1x1', '7x9', '8x8', '9x17', '72x16', '8x2056', 'constant', 'checker', 'noise', 'zrl', 'strided', 'scene') for k in ('gray', 'rgb')]
