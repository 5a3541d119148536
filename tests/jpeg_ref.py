"""A baseline sequential JPEG (JFIF) encoder in numpy / pure Python: the definition of include/fluxmi.h (fluxmi_jpeg_encode) and nothing
else, in int32 / int64 only.  It is what tests/test_jpeg_gpu.py compares the device encoder with byte for byte, and what
tests/test_jpeg_cpu.py compares with Pillow (libjpeg-turbo at its defaults).

    jpeg_ref(px, quality=99, subsampling="4:2:0", restart_interval=0) -> bytes

px is uint8 [H, W, 3] or [B, H, W, 3]; a batch is ONE image of height B * H.  `stats`, when a dict, receives what the stream contained
(the coverage condition of the tests); the three `mutate_*` switches are the deliberately wrong encoders the tests' teeth use."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.1: the example quantisation tables, in natural (row-major) order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32)

# Annex K.3: the example Huffman tables as (code counts per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
            0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
            0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
            0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
              0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
              0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])


def quant_table(base, quality: int):
    """libjpeg's quality rule on an Annex K table (natural order) -> int64 [64] of 1..255"""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_ref: quality={quality!r}: expected an integer in 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(base, np.int64) * s + 50) // 100, 1, 255)


def huff_codes(table):
    """(counts, symbols) -> {symbol: (code, length)}: the canonical code of Annex C"""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _fdct_pass(d, first: bool):
    """one pass of libjpeg's accurate integer DCT over the LAST axis of d (int64 [..., 8]): 13-bit constants, 2 extra bits kept by the first
    pass and removed by the second"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15

    def ds(x, n):
        return (x + (1 << (n - 1))) >> n

    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = ds(t10 + t11, 2), ds(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = ds(z1 + t13 * 6270, sh), ds(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, sh), ds(t5 + z2 + z4, sh), ds(t6 + z2 + z3, sh), ds(t7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def _levels(plane, qt):
    """plane int64 [h, w] (h, w multiples of 8, samples 0..255) -> quantised levels int64 [h/8, w/8, 64] in zigzag order"""
    h, w = plane.shape
    blk = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # [by, bx, row, col]
    blk = _fdct_pass(blk, True)                                            # rows
    blk = _fdct_pass(blk.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)  # columns
    c = blk.reshape(h // 8, w // 8, 64)
    lev = np.sign(c) * ((np.abs(c) + 4 * qt) // (8 * qt))
    return lev[..., ZIGZAG]


class _Bits:
    """the entropy-coded segment: most significant bit first, 0xFF followed by a stuffed 0x00"""

    def __init__(self, stats):
        self.out, self.acc, self.n, self.stats = bytearray(), 0, 0, stats

    def put(self, code: int, length: int):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
                self.stats["stuffed_ff"] += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v: int) -> int:
    return int(abs(int(v))).bit_length()


def _encode_block(bits: _Bits, lev, pred: int, dc, ac, stats):
    diff = int(lev[0]) - pred
    n = _category(diff)
    stats["max_dc_category"] = max(stats["max_dc_category"], n)
    bits.put(*dc[n])
    if n:
        bits.put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
    run = 0
    nz = np.nonzero(lev[1:])[0] + 1
    last = 0
    for k in nz:
        run = int(k) - last - 1
        last = int(k)
        while run >= 16:
            bits.put(*ac[0xF0])
            stats["zrl"] += 1
            run -= 16
        v = int(lev[k])
        n = _category(v)
        stats["max_ac_category"] = max(stats["max_ac_category"], n)
        bits.put(*ac[(run << 4) | n])
        bits.put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)
    if last != 63:
        bits.put(*ac[0x00])
        if last == 0:
            stats["eob_only_blocks"] += 1
    else:
        stats["blocks_without_eob"] += 1


def header(height: int, width: int, quality: int, subsampling: str, restart_interval: int) -> bytes:
    """SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI when restart_interval > 0, SOS"""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)

    h = bytes([0xFF, 0xD8]) + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, base in enumerate((Q_LUMA, Q_CHROMA)):
        h += seg(0xDB, bytes([i]) + bytes(int(v) for v in quant_table(base, quality)[ZIGZAG]))
    samp = 0x22 if subsampling == "4:2:0" else 0x11
    h += seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3, 1, samp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (counts, symbols) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        h += seg(0xC4, bytes([tc_th]) + bytes(counts) + bytes(symbols))
    if restart_interval > 0:
        h += seg(0xDD, restart_interval.to_bytes(2, "big"))
    return h + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def new_stats() -> dict:
    return dict(zrl=0, blocks_without_eob=0, stuffed_ff=0, rst=[], max_dc_category=0, max_ac_category=0, eob_only_blocks=0,
                replicated_right=False, replicated_bottom=False)


def jpeg_ref(px, quality: int = 99, subsampling: str = "4:2:0", restart_interval: int = 0, stats=None, mutate_bias_2: bool = False,
             mutate_swap_cbcr: bool = False, mutate_rst_no_wrap: bool = False) -> bytes:
    px = np.asarray(px)
    if px.dtype != np.uint8 or px.ndim not in (3, 4) or px.shape[-1] != 3 or min(px.shape) < 1:
        raise ValueError(f"jpeg_ref: expected uint8 [H, W, 3] or [B, H, W, 3], got {px.dtype} {px.shape}")
    if subsampling not in ("4:2:0", "4:4:4"):
        raise ValueError(f"jpeg_ref: subsampling={subsampling!r}: expected \"4:2:0\" or \"4:4:4\"")
    if isinstance(restart_interval, bool) or not 0 <= int(restart_interval) <= 65535:
        raise ValueError(f"jpeg_ref: restart_interval={restart_interval!r}: expected an integer in 0..65535")
    R = int(restart_interval)
    px = px.reshape(-1, px.shape[-2], 3)  # the batch stacked vertically
    H, W = px.shape[:2]
    if H > 65535 or W > 65535:
        raise ValueError(f"jpeg_ref: {W} x {H} is beyond JPEG's 65535 x 65535")
    stats = new_stats() if stats is None else stats
    m = 16 if subsampling == "4:2:0" else 8
    mw, mh = -(-W // m), -(-H // m)
    stats["replicated_right"] |= mw * m != W
    stats["replicated_bottom"] |= mh * m != H
    px = np.pad(px, ((0, mh * m - H), (0, mw * m - W), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if mutate_swap_cbcr:
        cb, cr = cr, cb
    if subsampling == "4:2:0":
        bias = np.full(mw * 8, 2, np.int64) if mutate_bias_2 else 1 + (np.arange(mw * 8, dtype=np.int64) & 1)
        cb, cr = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2 for c in (cb, cr))
        # below the image it is the last CHROMA row that repeats (the box of rows H - 2 and H - 1 when H is even), as libjpeg pads
        ch = (H + 1) // 2
        cb, cr = (np.concatenate([c[:ch], np.repeat(c[ch - 1:ch], mh * 8 - ch, axis=0)]) for c in (cb, cr))
    ql, qc = quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)
    ly, lcb, lcr = _levels(y, ql), _levels(cb, qc), _levels(cr, qc)
    dcl, acl, dcc, acc = (huff_codes(t) for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA))
    bits = _Bits(stats)
    pred = [0, 0, 0]
    n_mcu, n_rst = mw * mh, 0
    nbw, nbh = -(-W // 8), -(-H // 8)
    for i in range(n_mcu):
        if R and i and i % R == 0:
            bits.flush()
            mk = n_rst if mutate_rst_no_wrap else n_rst % 8
            bits.out += bytes([0xFF, (0xD0 + mk) & 0xFF])
            stats["rst"].append(n_rst % 8)
            n_rst += 1
            pred = [0, 0, 0]
        my, mx = divmod(i, mw)
        if subsampling == "4:2:0":
            blocks = []
            for j in range(4):  # a Y block wholly outside the image is a dummy block: the DC level of the block before it, no AC
                by, bx = 2 * my + (j >> 1), 2 * mx + (j & 1)
                lev = ly[by, bx]
                if by >= nbh or bx >= nbw:
                    lev = np.zeros(64, np.int64)
                    lev[0] = blocks[j - 1][1][0]
                blocks.append((0, lev))
            blocks += [(1, lcb[my, mx]), (2, lcr[my, mx])]
        else:
            blocks = [(0, ly[my, mx]), (1, lcb[my, mx]), (2, lcr[my, mx])]
        for c, lev in blocks:
            _encode_block(bits, lev, pred[c], dcl if c == 0 else dcc, acl if c == 0 else acc, stats)
            pred[c] = int(lev[0])
    bits.flush()
    return header(H, W, quality, subsampling, R) + bytes(bits.out) + b"\xFF\xD9"


def scan_bytes(stream: bytes) -> bytes:
    """the entropy-coded segment of a baseline JPEG: from the end of the SOS header to EOI, RST markers included"""
    i = 2
    while True:
        assert stream[i] == 0xFF, f"marker expected at {i}"
        marker, n = stream[i + 1], int.from_bytes(stream[i + 2:i + 4], "big")
        if marker == 0xDA:
            assert stream[-2:] == b"\xFF\xD9"
            return stream[i + 2 + n:-2]
        i += 2 + n


def segments(stream: bytes, marker: int) -> list:
    """the payloads of every `marker` segment ahead of SOS"""
    i, out = 2, []
    while True:
        assert stream[i] == 0xFF, f"marker expected at {i}"
        mk, n = stream[i + 1], int.from_bytes(stream[i + 2:i + 4], "big")
        if mk == marker:
            out.append(stream[i + 4:i + 2 + n])
        if mk == 0xDA:
            return out
        i += 2 + n
