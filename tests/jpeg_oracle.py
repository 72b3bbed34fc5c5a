"""TEST INFRASTRUCTURE: the JPEG encoder of include/lhw.h (lhw_jpeg_encode) restated in plain numpy and Python integers, one block at a
time, with its own copies of the tables of ITU-T T.81 Annex K.  It imports nothing from the product: what it returns -- the quantised
coefficients of every block and the entropy-coded bytes of the frame -- is what the header comment says, read independently.
"""
import numpy as np

# Annex K.3 - K.6: (BITS, HUFFVAL) of the DC and AC tables, luminance then chrominance
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
# Annex K.1 / K.2: the example quantisation tables, natural order
Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def quant_tables(quality):
    """the usual scaling of the Annex K tables: 50 = the tables, values clamped to 1..255; (luma, chroma) lists in natural order"""
    quality = min(100, max(1, int(quality)))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(255, max(1, (q * scale + 50) // 100)) for q in t] for t in (Q_LUMA, Q_CHROMA))


def huffman_codes(bits, vals):
    """{symbol: (code, length)}: the canonical code of Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def zigzag_order():
    """natural index 8 v + u of the k-th coefficient in zig-zag order, from the anti-diagonals"""
    order = []
    for s in range(15):
        diag = [(s - u, u) for u in range(8) if 0 <= s - u < 8]      # (v, u), u growing: the direction of an even diagonal
        order += [8 * v + u for v, u in (diag if s % 2 == 0 else diag[::-1])]
    return order


def _d(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_1d(d, first):
    """one pass of the header's DCT on eight Python integers"""
    n = 11 if first else 15
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z = (e2 + e3) * 4433
    o = [0] * 8
    o[0], o[4] = ((e0 + e1) * 4, (e0 - e1) * 4) if first else (_d(e0 + e1, 2), _d(e0 - e1, 2))
    o[2], o[6] = _d(z + e3 * 6270, n), _d(z - e2 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    a3, a4 = z5 - z3 * 16069, z5 - z4 * 3196
    o[7], o[5] = _d(t4 * 2446 - z1 * 7373 + a3, n), _d(t5 * 16819 - z2 * 20995 + a4, n)
    o[3], o[1] = _d(t6 * 25172 - z2 * 20995 + a3, n), _d(t7 * 12299 - z1 * 7373 + a4, n)
    return o


def fdct(block):
    """8 x 8 level-shifted samples [y][x] -> 8 x (orthonormal DCT-II) as Python integers [v][u]: rows first, then columns"""
    rows = [fdct_1d([int(x) for x in r], True) for r in block]
    cols = [fdct_1d([rows[y][u] for y in range(8)], False) for u in range(8)]
    return [[cols[u][v] for u in range(8)] for v in range(8)]


def quantise(coef, table):
    out = []
    for c, q in zip([c for r in coef for c in r], table):
        k = (abs(c) + 4 * q) // (8 * q)
        out.append(k if c >= 0 else -k)
    return out


def ycbcr(rgb):
    """uint8 [H][W][3] -> int64 [3][H][W], the header's fixed-point matrix"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16])


class _Bits:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> (n - 1 - k)) & 1 for k in range(n)]

    def magnitude(self, v, s):
        self.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)

    def close(self):
        """padded with 1-bits, as stuffed bytes"""
        self.bits += [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(self.bits), 8):
            byte = int("".join(map(str, self.bits[i:i + 8])), 2)
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
        return bytes(out)


def encode(rgb, qluma, qchroma):
    """One frame, uint8 [H][W][3] -> (blocks, segment): blocks int [R][M][6][64], the quantised coefficients of every block in natural order
    (MCU order Y Y Y Y Cb Cr); segment: the bytes between the SOS header and EOI."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    M, R = -(-W // 16), -(-H // 16)
    padded = rgb[np.minimum(np.arange(16 * R), H - 1)][:, np.minimum(np.arange(16 * M), W - 1)]
    y, cb, cr = ycbcr(padded)
    half = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    planes = [y - 128, half(cb) - 128, half(cr) - 128]
    dc_codes, ac_codes = [huffman_codes(*DC_LUMA), huffman_codes(*DC_CHROMA)], [huffman_codes(*AC_LUMA), huffman_codes(*AC_CHROMA)]
    zz = zigzag_order()
    blocks = np.zeros((R, M, 6, 64), dtype=np.int64)
    segment = b""
    for r in range(R):
        out, pred = _Bits(), [0, 0, 0]
        for m in range(M):
            for slot in range(6):
                comp = 0 if slot < 4 else slot - 3
                if comp == 0:
                    x0, y0 = 16 * m + 8 * (slot & 1), 16 * r + 8 * (slot >> 1)
                else:
                    x0, y0 = 8 * m, 8 * r
                q = quantise(fdct(planes[comp][y0:y0 + 8, x0:x0 + 8]), qluma if comp == 0 else qchroma)
                blocks[r, m, slot] = q
                t = min(comp, 1)
                diff, pred[comp] = q[0] - pred[comp], q[0]
                s = abs(diff).bit_length()
                assert s <= 11
                out.put(*dc_codes[t][s])
                out.magnitude(diff, s)
                run = 0
                for k in range(1, 64):
                    c = q[zz[k]]
                    if c == 0:
                        run += 1
                        continue
                    while run >= 16:
                        out.put(*ac_codes[t][0xF0])
                        run -= 16
                    s = abs(c).bit_length()
                    assert s <= 10
                    out.put(*ac_codes[t][(run << 4) | s])
                    out.magnitude(c, s)
                    run = 0
                if run:
                    out.put(*ac_codes[t][0x00])
        segment += out.close()
        if r != R - 1:
            segment += bytes([0xFF, 0xD0 + r % 8])
    return blocks, segment
