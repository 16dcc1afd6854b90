"""Test helper: write DEFLATE streams (RFC 1951) and gzip / BGZF members (RFC 1952, SAM/BAM spec 4.1) bit by bit, including
the streams no compressor writes — single 1-bit codes, incomplete or over-subscribed codes, symbols 286/287 and 30/31, code-length
repeats that cross from the literal lengths into the distance lengths, distances that reach exactly to the start of the output or
one byte further, stored blocks whose LEN/NLEN disagree — and a named corpus of such cases (CASES, EMPTY_CASES).

Nothing here decides whether a stream is valid: `zlib_verdict` asks zlib's inflate, the library every decoder of this project is
held to.  The writer only keeps count of the output a decoder would produce (bytes in front of the start read as zeros), so that a
case can state a distance relative to the output position and a test can compare bytes when zlib accepts."""
import random
import struct
import zlib

# RFC 1951 3.2.5
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def canonical(lengths):
    """Codes of a canonical Huffman code (RFC 1951 3.2.2) per symbol (None where the length is 0).  Works for any lengths:
    an over-subscribed set gets codes that collide, which is what a stream built on one carries."""
    mx = max(lengths) if lengths else 0
    count = [0] * (mx + 2)
    for n in lengths:
        if n:
            count[n] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lengths:
        if n:
            out.append(nxt[n] & ((1 << n) - 1))
            nxt[n] += 1
        else:
            out.append(None)
    return out


def complete_lengths(symbols, size):
    """Code lengths (a list of `size`) of a complete prefix code over `symbols` (at least two): depth d - 1 and d."""
    k = len(symbols)
    assert k >= 2
    d = (k - 1).bit_length()
    shallow = (1 << d) - k
    lens = [0] * size
    for i, s in enumerate(sorted(symbols)):
        lens[s] = d - 1 if i < shallow else d
    return lens


class Deflate:
    """A DEFLATE stream being written.  `history`: output that is already there in front of the stream (the records in front of
    a case inside one gzip member); distances may reach into it.  `pos` is the output position (history included)."""

    def __init__(self, history=b""):
        self.acc = 0
        self.nacc = 0
        self.buf = bytearray()
        self.out = bytearray(history)
        self.start = len(history)

    @property
    def pos(self):
        return len(self.out)

    def data(self):
        return bytes(self.out[self.start:])

    # bits
    def bits(self, v, n):                      # header fields and extra bits: least significant bit first
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, c, n):                      # Huffman codes: most significant bit first
        r = 0
        for i in range(n):
            r |= ((c >> i) & 1) << (n - 1 - i)
        self.bits(r, n)

    def align(self):
        if self.nacc:
            self.bits(0, 8 - self.nacc)

    def raw(self, b):                          # bytes at the current (byte-aligned) position
        assert self.nacc == 0
        self.buf += b

    def finish(self, trailing=b""):
        self.align()
        return bytes(self.buf) + bytes(trailing)

    # output bookkeeping
    def _copy(self, length, dist):
        for _ in range(length):
            i = len(self.out) - dist
            self.out.append(self.out[i] if 0 <= i else 0)

    # blocks
    def header(self, final, btype):
        self.bits(1 if final else 0, 1)
        self.bits(btype, 2)

    def stored(self, data, final=False, length=None, nlength=None, body=None):
        """A stored block; length / nlength override LEN / NLEN, body the bytes that follow them (default: data)."""
        self.header(final, 0)
        self.align()
        ln = len(data) if length is None else length
        nl = (~ln & 0xFFFF) if nlength is None else nlength
        self.raw(struct.pack("<HH", ln, nl))
        self.raw(data if body is None else body)
        self.out += data

    def fixed(self, items, final=False, eob=True):
        self.header(final, 1)
        self._symbols(items, canonical(FIXED_LIT), FIXED_LIT, canonical(FIXED_DIST), FIXED_DIST, eob)

    def dynamic(self, lit, dist, items, final=False, eob=True, cl_seq=None, cl_lens=None, hlit=None, hdist=None, hclen=None):
        """A dynamic block with literal/length code lengths `lit` and distance code lengths `dist` (their lengths give HLIT / HDIST
        unless stated).  cl_seq: the code-length symbols as (symbol, extra) pairs (default: every length spelled out, no repeat);
        cl_lens: the code-length code's 19 lengths by symbol (default: a complete code over the symbols cl_seq uses)."""
        hlit = len(lit) if hlit is None else hlit
        hdist = len(dist) if hdist is None else hdist
        if cl_seq is None:
            cl_seq = [(n, 0) for n in list(lit) + list(dist)]
        if cl_lens is None:
            used = sorted({s for s, _ in cl_seq})
            if len(used) == 1:
                used.append(0 if used[0] else 1)
            cl_lens = complete_lengths(used, 19)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        self.header(final, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CL_ORDER[i]], 3)
        clc = canonical(cl_lens)
        for s, extra in cl_seq:
            self.code(clc[s], cl_lens[s])
            if s >= 16:
                self.bits(extra, {16: 2, 17: 3, 18: 7}[s])
        self._symbols(items, canonical(lit), lit, canonical(dist) if dist else [], dist, eob)

    def _symbols(self, items, lcodes, llens, dcodes, dlens, eob):
        """items: a bytes object (literals), ("M", length, dist) a match, ("M", length, dist, lsym, lextra, dsym, dextra) a match
        spelled with explicit symbols (None: the standard one), ("S", symbol) a bare literal/length symbol."""
        def lsym(s):
            assert llens[s], "symbol %d has no code" % s
            self.code(lcodes[s], llens[s])
        for it in items:
            if isinstance(it, (bytes, bytearray)):
                for b in it:
                    lsym(b)
                    self.out.append(b)
            elif it[0] == "S":
                lsym(it[1])
            else:
                _, length, d = it[:3]
                ls, le, ds, de = (list(it[3:]) + [None] * 4)[:4]
                if ls is None:
                    i = 28 if length == 258 else max(k for k in range(29) if LBASE[k] <= length)
                    ls, le = 257 + i, length - LBASE[i]
                lsym(ls)
                if ls - 257 < 29:
                    self.bits(le, LEXT[ls - 257])
                if ds is None:
                    ds = max(k for k in range(30) if DBASE[k] <= d)
                    de = d - DBASE[ds]
                assert dlens[ds], "distance symbol %d has no code" % ds
                self.code(dcodes[ds], dlens[ds])
                if ds < 30:
                    self.bits(de, DEXT[ds])
                self._copy(length, d)
        if eob:
            lsym(256)


def member(comp, data_len, crc, bgzf=True, fname=None, fcomment=None, fhcrc=False, hcrc=None, reserved=0, sub_before=b"",
           sub_after=b"", bsize=None):
    """A gzip member holding the raw deflate bytes `comp`, trailer (crc, data_len & 0xFFFFFFFF).  bgzf: FEXTRA with the "BC"
    subfield (BSIZE - 1 = the member's length - 1 unless `bsize` says otherwise), other subfields before / after it as given.
    fname / fcomment: bytes without the terminating zero; fhcrc: the header CRC-16 (hcrc overrides it); reserved: flag bits 5-7."""
    flg = reserved | (2 if fhcrc else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0)
    extra = b""
    if bgzf:
        flg |= 4
        xlen = len(sub_before) + 6 + len(sub_after)
        tail = (len(fname) + 1 if fname is not None else 0) + (len(fcomment) + 1 if fcomment is not None else 0) + (2 if fhcrc else 0)
        total = 12 + xlen + tail + len(comp) + 8 if bsize is None else bsize
        extra = struct.pack("<H", xlen) + sub_before + b"BC" + struct.pack("<HH", 2, total - 1) + sub_after
    h = bytes([0x1F, 0x8B, 8, flg]) + b"\0\0\0\0" + b"\x00\xff" + extra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) if hcrc is None else hcrc)
    return h + comp + struct.pack("<II", crc & 0xFFFFFFFF, data_len & 0xFFFFFFFF)


def zlib_verdict(comp, data_len, crc):
    """(accepted, output): zlib's inflate of the raw deflate bytes reaches the end of the final block exactly at the end of
    `comp`, and its output has the announced length and CRC-32."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(comp)
    except zlib.error:
        return False, None
    ok = d.eof and not d.unused_data and len(out) == data_len and zlib.crc32(out) == (crc & 0xFFFFFFFF)
    return ok, (out if ok else None)


def device_status(comp, data_len, crc):
    """What the device decoder reports for the block: 0 accepted, 2 a stream zlib inflates to the announced length whose CRC-32
    differs, 1 anything else."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(comp)
    except zlib.error:
        return 1
    if not d.eof or d.unused_data or len(out) != data_len:
        return 1
    return 0 if zlib.crc32(out) == (crc & 0xFFFFFFFF) else 2


def gunzip_members(buf):
    """zlib's reading of a multi-member gzip stream (what the sequential path does): (bytes, error or None)."""
    out, pos = [], 0
    while pos < len(buf):
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(buf[pos:]))
        except zlib.error as e:
            return b"".join(out), e
        if not d.eof:
            return b"".join(out), EOFError("the stream ends inside a member")
        pos = len(buf) - len(d.unused_data)
    return b"".join(out), None


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
def _fill(w, n, seed=7):
    """Stored blocks of pseudo-random bytes until the output holds `n` bytes (a window for long distances)."""
    r = random.Random(seed)
    while w.pos < n:
        k = min(n - w.pos, 0xFFFF)
        w.stored(bytes(r.getrandbits(8) for _ in range(k)))


LIT2 = [0] * 288                                       # lengths for "two literals and end-of-block"
LIT2[ord("a")], LIT2[ord("b")], LIT2[256] = 2, 2, 1
LIT2 = LIT2[:257]


def _lit_all(extra=None, n=286):
    """A complete literal/length code over all n symbols (lengths 8 and 9), optionally adjusted."""
    lens = complete_lengths(list(range(n)), n)
    for k, v in (extra or {}).items():
        lens[k] = v
    return lens


D30 = complete_lengths(list(range(30)), 30)        # a complete distance code over all 30 symbols


def _c(name, build, isize=0, crc=0):
    return (name, build, isize, crc)


def _dyn_eob_only(w):
    w.dynamic([0] * 256 + [1], [0], [], final=True)


def _dyn_two_lits(w):
    w.dynamic(LIT2, [0], [b"abba"], final=True)


def _dyn_one_dist(code_one):
    def b(w):
        lit = _lit_all()
        dist = [1]                                     # one distance code of 1 bit: symbol 0 (distance 1)
        items = [b"xy", ("M", 5, 1)]
        if code_one:                                   # the unused code "1": written by hand behind a length symbol
            w.dynamic(lit, dist, [b"xy", ("S", 259)], final=False, eob=False)
            w.code(1, 1)
            w.fixed([], final=True)
            return
        w.dynamic(lit, dist, items, final=True)
    return b


def _dyn_lit(lens_patch, n=286):
    def b(w):
        lit = _lit_all(n=n)
        for k, v in lens_patch.items():
            lit[k] = v
        w.dynamic(lit, D30, [b"q"], final=True)
    return b


def _dyn_oversub_dist(w):
    w.dynamic(_lit_all(), [1, 1, 1], [b"ab", ("M", 3, 2)], final=True)


def _dyn_incomplete_clc(w):
    seq = [(8, 0)] * 256 + [(5, 0)] * 31
    lens = [0] * 19
    lens[8], lens[5], lens[9] = 2, 2, 2              # 3 of 4 two-bit codes: incomplete
    w.dynamic([8] * 256 + [5], [5] * 30, [], final=True, cl_seq=seq, cl_lens=lens, eob=False)


def _dyn_zero_clc(w):
    w.header(True, 2)
    w.bits(0, 5)
    w.bits(0, 5)
    w.bits(15, 4)
    w.bits(0, 19 * 3)
    w.bits(0, 16)


def _dyn_no_eob(w):
    w.dynamic([8] * 256 + [0], D30, [b"x"], final=True, eob=False)


def _dyn_hlit(n):
    def b(w):
        lit = _lit_all(n=n)
        w.dynamic(lit, D30, [b"hi"], final=True)
    return b


def _dyn_hdist(n):
    def b(w):
        w.dynamic(_lit_all(), complete_lengths(list(range(n)), n), [b"hey", ("M", 3, 3)], final=True)
    return b


def _dyn_16_first(w):
    lit = _lit_all()
    seq = [(16, 3)] + [(n, 0) for n in lit[6:]] + [(n, 0) for n in D30]
    w.dynamic(lit, D30, [], final=True, cl_seq=seq, eob=False)


def _dyn_repeat_past_end(sym):
    def b(w):                                          # 29 distance lengths written, then a repeat of 6 / 10 / 138 for the last one
        lit = _lit_all()
        seq = [(n, 0) for n in lit] + [(n, 0) for n in D30[:29]] + [(sym, {16: 3, 17: 7, 18: 127}[sym])]
        w.dynamic(lit, D30, [], final=True, cl_seq=seq, eob=False)
    return b


def _dyn_repeat_crossing(w):
    # HLIT 259: literals 0..250 of 8 bits, 251..256 of 9, 257 / 258 of 8 (complete); HDIST 10: 8, 8, 8, 1, 2, ..., 6, 8 (complete).
    # The code-length sequence writes literal 257's 8, then ONE "16" (repeat 3 times) for literal 258 and distances 0 and 1.
    lit = [8] * 251 + [9] * 6 + [8, 8]
    dist = [8, 8, 8, 1, 2, 3, 4, 5, 6, 8]
    seq = [(8, 0)] * 251 + [(9, 0), (16, 2), (8, 0), (16, 0), (8, 0)] + [(n, 0) for n in dist[3:]]
    w.dynamic(lit, dist, [b"cross", ("M", 4, 5), ("M", 3, 1), ("M", 3, 2)], final=True, cl_seq=seq)


def _dyn_15_bits(w):
    # literal/length: 'a'..'m', 256, 257, 258 of lengths 1, 2, ..., 15, 15 (complete; lengths 3 and 4 have 15-bit codes);
    # distance: symbols 0..15 of lengths 1, ..., 15, 15 (distances 129 ... 256 have 15-bit codes)
    lit = [0] * 286
    for i, s in enumerate([ord(c) for c in "abcdefghijklm"] + [256, 257, 258]):
        lit[s] = min(i + 1, 15)
    dist = [min(i + 1, 15) for i in range(16)]
    items = [b"abcdefghijklm"] + [("M", 4, 13)] * 50 + [("M", 3, 130), ("M", 4, 200), b"m"]
    w.dynamic(lit, dist, items, final=True)


def _dyn_hclen(n):
    def b(w):
        if n == 4:                                     # only 16, 17, 18, 0 have code-length codes: every length is zero
            lens = [0] * 19
            lens[17], lens[18] = 1, 1
            w.dynamic([0] * 257, [0], [], final=True, cl_seq=[(18, 127), (18, 109)], cl_lens=lens, hclen=4,
                      hlit=257, hdist=1, eob=False)
        else:
            w.dynamic(_lit_all(), D30, [b"all19"], final=True, cl_lens=complete_lengths(list(range(19)), 19), hclen=19)
    return b


CASES = [
    _c("fixed_abc", lambda w: w.fixed([b"abc"], final=True)),
    _c("fixed_258_as_285", lambda w: w.fixed([b"z", ("M", 258, 1)], final=True)),
    _c("fixed_258_as_284_31", lambda w: w.fixed([b"z", ("M", 258, 1, 284, 31)], final=True)),
    _c("fixed_lit_286", lambda w: w.fixed([b"z", ("M", 3, 1, 286, 0)], final=True)),
    _c("fixed_lit_287", lambda w: w.fixed([b"z", ("M", 3, 1, 287, 0)], final=True)),
    _c("fixed_dist_30", lambda w: w.fixed([b"zz", ("M", 3, 1, None, None, 30, 0)], final=True)),
    _c("fixed_dist_31", lambda w: w.fixed([b"zz", ("M", 3, 1, None, None, 31, 0)], final=True)),
    _c("dist_exactly_start", lambda w: w.fixed([b"0123456789", ("M", 10, w.pos + 10)], final=True)),
    _c("dist_one_past_start", lambda w: w.fixed([b"0123456789", ("M", 10, w.pos + 11)], final=True)),
    _c("dist_32768", lambda w: (_fill(w, 32768), w.fixed([("M", 40, 32768)], final=True))),
    _c("match_spans_blocks", lambda w: (w.fixed([b"spanspan"]), w.stored(b"!"), w.fixed([("M", 20, 9)], final=True))),
    _c("empty_stored_between", lambda w: (w.fixed([b"left"]), w.stored(b""), w.fixed([b"right", ("M", 5, 9)], final=True))),
    _c("stored_nlen_mismatch", lambda w: w.stored(b"hello", final=True, nlength=0x1234)),
    _c("stored_len_past_end", lambda w: w.stored(b"hello", final=True, length=6)),
    _c("btype_3", lambda w: (w.fixed([b"ok"]), w.header(True, 3), w.bits(0, 16))),
    _c("nonfinal_at_end", lambda w: w.fixed([b"not the end"], final=False)),
    _c("trailing_byte", lambda w: (w.fixed([b"end"], final=True), w.align(), w.raw(b"\0"))),
    _c("dyn_eob_only", _dyn_eob_only),
    _c("dyn_two_lits_empty_dist", _dyn_two_lits),
    _c("dyn_one_dist_code0", _dyn_one_dist(False)),
    _c("dyn_one_dist_code1", _dyn_one_dist(True)),
    _c("dyn_lit_incomplete", _dyn_lit({0: 0, 1: 0})),
    _c("dyn_lit_oversubscribed", _dyn_lit({0: 7})),
    _c("dyn_dist_oversubscribed", _dyn_oversub_dist),
    _c("dyn_clc_incomplete", _dyn_incomplete_clc),
    _c("dyn_clc_all_zero", _dyn_zero_clc),
    _c("dyn_no_eob", _dyn_no_eob),
    _c("dyn_hlit_287", _dyn_hlit(287)),
    _c("dyn_hlit_288", _dyn_hlit(288)),
    _c("dyn_hdist_31", _dyn_hdist(31)),
    _c("dyn_hdist_32", _dyn_hdist(32)),
    _c("dyn_16_first", _dyn_16_first),
    _c("dyn_16_past_end", _dyn_repeat_past_end(16)),
    _c("dyn_17_past_end", _dyn_repeat_past_end(17)),
    _c("dyn_18_past_end", _dyn_repeat_past_end(18)),
    _c("dyn_repeat_crossing", _dyn_repeat_crossing),
    _c("dyn_15_bit_codes", _dyn_15_bits),
    _c("dyn_hclen_4", _dyn_hclen(4)),
    _c("dyn_hclen_19", _dyn_hclen(19)),
    _c("isize_minus_1", lambda w: w.fixed([b"records and more records"], final=True), isize=-1),
    _c("isize_minus_1000", lambda w: (_fill(w, 3000), w.fixed([b"x"], final=True)), isize=-1000),
    _c("isize_plus_1", lambda w: w.fixed([b"records"], final=True), isize=+1),
    _c("crc_wrong", lambda w: w.fixed([b"checksummed"], final=True), crc=0x80000000),
]

# blocks of 0 to 2 bytes: (name, raw deflate bytes)
EMPTY_CASES = [
    ("empty_03_00", b"\x03\x00"),
    ("empty_01_00", b"\x01\x00"),
    ("empty_00_00", b"\x00\x00"),
    ("empty_one_byte", b"\x03"),
    ("empty_clen_0", b""),
]


def build(case, history=b""):
    """(raw deflate bytes, the output a decoder gives if it accepts, announced length, announced CRC-32) of a corpus case
    written behind `history`."""
    name, fn, disize, dcrc = case
    w = Deflate(history)
    fn(w)
    comp = w.finish()
    data = w.data()
    return comp, data, len(data) + disize, zlib.crc32(data) ^ dcrc


def all_cases(history=b""):
    """[(name, raw, data, isize, crc)] of CASES and EMPTY_CASES (the empty ones announce 0 bytes, CRC 0)."""
    out = []
    for c in CASES:
        comp, data, isize, crc = build(c, history)
        out.append((c[0], comp, data, isize, crc))
    for name, raw in EMPTY_CASES:
        out.append((name, raw, b"", 0, 0))
    return out
