"""A plain Python restatement of the label-PNG stream format, written from the format's description and
RFC 1951 only: Up-filtered rows, one fixed-Huffman block plus an empty stored block per row, run-length tokens by a
closed-form rule per maximal run.  Slow and obvious on purpose; the HIP encoder must produce these bytes."""
import zlib

import numpy as np

# RFC 1951 §3.2.5: (first length, extra bits) of the length codes 257 .. 285
_LENGTH_CODES = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1),
                 (19, 2), (23, 2), (27, 2), (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4),
                 (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0)]


class BitWriter:
    """Deflate's bit order: bits fill a byte from its least significant end; Huffman codes go in most significant
    bit first, every other field least significant bit first."""

    def __init__(self):
        self.bits = []

    def field(self, value, n):
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, value, n):
        self.bits += [(value >> i) & 1 for i in range(n - 1, -1, -1)]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def tobytes(self):
        assert len(self.bits) % 8 == 0
        return np.packbits(np.array(self.bits, dtype=np.uint8), bitorder="little").tobytes()


def fixed_symbol(w, sym):
    """RFC 1951 §3.2.6: the fixed code of a literal/length symbol."""
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def match(w, length):
    """A match of `length` (3 .. 258) at distance 1."""
    if length == 258:
        idx = 28
    else:
        idx = max(i for i, (first, _) in enumerate(_LENGTH_CODES[:28]) if first <= length)
    first, extra = _LENGTH_CODES[idx]
    fixed_symbol(w, 257 + idx)
    w.field(length - first, extra)
    w.code(0, 5)                                     # distance 1: code 0, five bits, no extra bits


def runs(data):
    """[(value, length)] of the maximal runs of a byte sequence."""
    out = []
    for v in data:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(int(v), n) for v, n in out]


def row_piece(filtered):
    w = BitWriter()
    w.field(0, 1)                                    # BFINAL = 0
    w.field(1, 2)                                    # BTYPE = 01
    for v, L in runs(filtered):
        fixed_symbol(w, v)
        for _ in range((L - 1) // 258):
            match(w, 258)
        r = (L - 1) % 258
        if r >= 3:
            match(w, r)
        else:
            for _ in range(r):
                fixed_symbol(w, v)
    fixed_symbol(w, 256)                             # end of block
    w.field(0, 1)                                    # an empty stored block: BFINAL = 0, BTYPE = 00
    w.field(0, 2)
    w.align()
    return w.tobytes() + b"\x00\x00\xff\xff"


def filtered_rows(image):
    """uint8 [H,W] -> uint8 [H,W+1]: filter type 2 (Up), the row above row 0 all zeros."""
    image = np.asarray(image, dtype=np.uint8)
    above = np.zeros_like(image)
    above[1:] = image[:-1]
    out = np.empty((image.shape[0], image.shape[1] + 1), dtype=np.uint8)
    out[:, 0] = 2
    out[:, 1:] = image - above                       # uint8 arithmetic wraps mod 256
    return out


def deflate_labels(image):
    """The zlib stream of a uint8 [H,W] image."""
    f = filtered_rows(image)
    body = b"".join(row_piece(row.tolist()) for row in f)
    return b"\x78\x01" + body + b"\x03\x00" + (zlib.adler32(f.tobytes()) & 0xffffffff).to_bytes(4, "big")


def bound(H, W):
    return 2 + H * ((9 * (W + 1) + 13 + 7) // 8 + 4) + 2 + 4
