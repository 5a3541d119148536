"""The PNG encoder's filter rule and strip rule (include/fluxmi.h, fluxmi_png_*) restated in numpy: the filtered scanlines and the strip
boundaries, nothing else -- zlib and Pillow are the decoders of record for the deflate blocks."""
import numpy as np

FILTERS = ("none", "sub", "up", "average", "paeth")
STRIP_TARGET, STRIP_ROWS = 67584, 16
FRAME_BYTES = 63  # signature 8, IHDR 25, IDAT framing 12, zlib header 2, Adler-32 4, IEND 12


def filtered(px: np.ndarray, filter: str = "adaptive") -> np.ndarray:
    """px uint8 [B, H, W, C] or [B, H, W] -> uint8 [B * H, 1 + W * C]: the batch is one image; the row above row 0 is zero"""
    C = 1 if px.ndim == 3 else px.shape[3]
    x = px.reshape(px.shape[0] * px.shape[1], -1).astype(np.int32)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b[1:] = x[:-1]
    c[1:, C:] = x[:-1, :-C]
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([(x - p) & 255 for p in (0 * x, a, b, (a + b) >> 1, paeth)])
    if filter == "adaptive":
        choice = np.minimum(res, 256 - res).sum(axis=2).argmin(axis=0)  # the first minimum: ties go to the lowest number
    else:
        choice = np.full(x.shape[0], FILTERS.index(filter))
    rows = res[choice, np.arange(x.shape[0])]
    return np.concatenate([choice[:, None], rows], axis=1).astype(np.uint8)


def strip_rows(W: int, C: int) -> int:
    return max(1, min(STRIP_ROWS, STRIP_TARGET // (1 + W * C)))


def strips(rows_total: int, W: int, C: int):
    r = strip_rows(W, C)
    return [(y, min(y + r, rows_total)) for y in range(0, rows_total, r)]


def strip_bound(n: int) -> int:
    return n + 5 * -(-n // 65535) + 5


def file_bound(rows_total: int, W: int, C: int) -> int:
    return FRAME_BYTES + sum(strip_bound((y1 - y0) * (1 + W * C)) for y0, y1 in strips(rows_total, W, C))


def idat_payload(png: bytes) -> bytes:
    """the concatenated data of the file's IDAT chunks"""
    pos, data = 8, b""
    while pos < len(png):
        n, kind = int.from_bytes(png[pos:pos + 4], "big"), png[pos + 4:pos + 8]
        if kind == b"IDAT":
            data += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return data
