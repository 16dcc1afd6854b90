"""The acceptance rules of the host DEFLATE decoders and of the BGZF member walks, case by case against zlib.

Every stream in test_pgzip.py / test_gpu_inflate.py was written by zlib's encoder (plus random bit flips), and the encoder never
writes most of the edges the decoders' rules are about: a single 1-bit code, length 258 spelled as 284 + 31, a repeat run that
crosses from the literal lengths into the distance lengths, a distance that reaches exactly the first byte, a 2-byte block that
is not the EOF marker, a gzip header with FNAME or FHCRC.  tests/deflate_craft.py writes them bit by bit; zlib's inflate gives the
verdict.  Each case is put into a BGZF file as one block among good ones (at the first block behind the header's, in the middle,
at the end) and into the tail of ONE ordinary gzip member, and the file is read through

  - the BGZF source with its own decoder (RawInflater, pgzip.cpp) — the default Reader of a BGZF file;
  - the BGZF source with zlib's inflate (IBU_BGZF_ZLIB=1);
  - the sequential zlib path (IBU_NO_PARALLEL_BGZF=1 IBU_NO_PARALLEL_GZIP=1);
  - the parallel single-member decoder (ParGzSource, several threads, small chunks);

and each must deliver what zlib's multi-member reading of the file gives: the same records, or Niffler with only good records in
front of the bad block delivered.  The device decoder runs the same corpus in test_gpu_deflate_edges.py."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import ibu_amd as ia
from tests import deflate_craft as dc

CASES = dc.all_cases()
CASE_IDS = [c[0] for c in CASES]
PATHS = ("raw", "zlib", "sequential")


def _records(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, n * 24, dtype=np.uint8).tobytes()


HEADER = ia.Header(16, 12).as_bytes()


def _set_path(monkeypatch, path):
    for k in ("IBU_BGZF_ZLIB", "IBU_NO_PARALLEL_BGZF", "IBU_NO_PARALLEL_GZIP", "IBU_PGZ_THREADS", "IBU_PGZ_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    if path == "zlib":
        monkeypatch.setenv("IBU_BGZF_ZLIB", "1")
    elif path == "sequential":
        monkeypatch.setenv("IBU_NO_PARALLEL_BGZF", "1")
        monkeypatch.setenv("IBU_NO_PARALLEL_GZIP", "1")
    elif path == "pgz":
        monkeypatch.setenv("IBU_PGZ_THREADS", "4")
        monkeypatch.setenv("IBU_PGZ_CHUNK", "2048")


def _read(p):
    """(record bytes delivered, error kind or None) of a Reader over the file."""
    out, kind = [], None
    try:
        r = ia.Reader.from_path(p)
    except ia.IbuError as e:
        return b"", e.kind
    try:
        while r.read_batch():
            b = r.buffered()
            out.append(np.array(b, copy=True).tobytes())
            r.consume(len(b))
    except ia.IbuError as e:
        kind = e.kind
    finally:
        r.close()
    return b"".join(out), kind


def _check_outcome(got, file_bytes, good, bad_at):
    """`got` (bytes, kind) against zlib's multi-member reading of `file_bytes`.  good: the bytes the file stands for if every
    block is accepted; bad_at: where the case's output starts in them."""
    want, err = dc.gunzip_members(file_bytes)
    data, kind = got
    if err is None and (len(want) - 32) % 24 == 0:
        assert data == want[32:] and kind is None
    elif err is None:                                            # (a case whose length no padding evens out)
        assert kind == "TruncatedRecord" and data == want[32:32 + len(data)]
    else:
        assert kind == "Niffler", (kind, err)
        assert data == good[32:32 + len(data)]                 # a prefix of the good records ...
        assert len(data) <= max(0, bad_at - 32)                  # ... from in front of the bad block only
    return err is None


def test_the_writer_against_zlib_literally():
    """A few verdicts stated outright, so that a broken writer cannot make every path agree on garbage."""
    by = {c[0]: c for c in CASES}
    expect = {"fixed_abc": b"abc", "fixed_258_as_284_31": b"z" * 259, "dyn_eob_only": b"", "dyn_two_lits_empty_dist": b"abba",
              "dyn_one_dist_code0": b"xy" + b"y" * 5, "dyn_repeat_crossing": b"crosscros" + b"s" * 6, "empty_03_00": b"",
              "dist_exactly_start": b"0123456789" * 2}
    for name, want in expect.items():
        _, comp, data, isize, crc = by[name]
        assert data == want and dc.zlib_verdict(comp, isize, crc) == (True, want), name
    for name in ("fixed_lit_286", "fixed_lit_287", "fixed_dist_30", "fixed_dist_31", "dist_one_past_start", "dyn_one_dist_code1",
                 "dyn_lit_incomplete", "dyn_lit_oversubscribed", "dyn_dist_oversubscribed", "dyn_clc_incomplete", "dyn_no_eob",
                 "dyn_hlit_287", "dyn_hdist_31", "dyn_16_first", "dyn_16_past_end", "stored_nlen_mismatch", "btype_3",
                 "trailing_byte", "nonfinal_at_end", "isize_minus_1", "crc_wrong", "empty_01_00", "empty_00_00", "empty_clen_0"):
        _, comp, data, isize, crc = by[name]
        assert dc.zlib_verdict(comp, isize, crc)[0] is False, name
    assert dc.device_status(*by["crc_wrong"][1:2], by["crc_wrong"][3], by["crc_wrong"][4]) == 2
    assert dc.zlib_verdict(b"\x03\x00", 0, 0) == (True, b"")
    assert dc.zlib_verdict(b"\x4b\x4c\x4a\x06\x00", 3, zlib.crc32(b"abc")) == (True, b"abc")   # zlib's own "abc"


def _bgzf_with_case(case, where):
    """(file bytes, good bytes, offset of the case's output) — a BGZF file: the header block, good record blocks, the case as one
    block at the first place behind the header's block, in the middle or at the end, and the EOF block."""
    _, comp, data, isize, crc = case
    recs = [_records(40, 1), _records(150, 2), _records(90, 3), _records(200, 4)]
    blocks = [HEADER + recs[0]] + recs[1:]
    at = {"first": 1, "middle": 3, "last": len(blocks)}[where]
    pad = (-len(data)) % 24                                      # the file stays whole records when the case is accepted
    blocks[at - 1] = blocks[at - 1] + _records(1, 9)[:pad]
    out, good, bad_at = bytearray(), bytearray(), 0
    for i, blk in enumerate(blocks[:at] + [None] + blocks[at:]):
        if blk is None:
            out += dc.member(comp, isize, crc)
            bad_at = len(good)
            good += data
        else:
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            cd = c.compress(blk) + c.flush()
            out += dc.member(cd, len(blk), zlib.crc32(blk))
            good += blk
    out += dc.BGZF_EOF
    return bytes(out), bytes(good), bad_at


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bgzf_block_edge_cases_read_as_zlib_reads_them(tmp_path, monkeypatch, case, where):
    f, good, bad_at = _bgzf_with_case(case, where)
    accepted = dc.zlib_verdict(*case[1:2], case[3], case[4])[0]
    want, err = dc.gunzip_members(f)
    assert (err is None) == accepted                             # the file stands or falls with its one odd block
    try:                                                         # Python's gzip module: the same reading
        assert gzip.decompress(f) == want and accepted
    except (OSError, EOFError, zlib.error):
        assert not accepted
    p = tmp_path / "f.ibu.gz"
    p.write_bytes(f)
    for path in PATHS:
        _set_path(monkeypatch, path)
        got = _read(p)
        try:
            _check_outcome(got, f, good, bad_at)
        except AssertionError as e:
            raise AssertionError(f"path {path}: {e}") from None


def _single_member_with_case(case_idx):
    """(file bytes, good bytes, offset of the case's output) — ONE gzip member: the header and records in non-final blocks
    (zlib's, closed with a sync flush), the case as the member's last blocks.  A few pad bytes behind the records keep the file
    whole records where the case's length allows it."""
    for pad in range(24):
        prefix = HEADER + _records(700, 5) + bytes(range(pad))
        if case_idx < len(dc.CASES):
            comp, data, isize, crc = dc.build(dc.CASES[case_idx], prefix)
        else:
            _, comp, data, isize, crc = CASES[case_idx]
        if (len(prefix) + len(data) - 32) % 24 == 0:
            break
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = c.compress(prefix) + c.flush(zlib.Z_SYNC_FLUSH)
    total = prefix + data
    trailer_len = len(total) + (isize - len(data))
    trailer_crc = zlib.crc32(total) ^ (crc ^ zlib.crc32(data))
    f = b"\x1f\x8b\x08\x00\0\0\0\0\x00\xff" + head + comp + struct.pack("<II", trailer_crc & 0xFFFFFFFF, trailer_len & 0xFFFFFFFF)
    return f, total, len(prefix)


@pytest.mark.parametrize("case_idx", range(len(CASES)), ids=CASE_IDS)
def test_single_member_tail_edge_cases_read_as_zlib_reads_them(tmp_path, monkeypatch, case_idx):
    f, good, bad_at = _single_member_with_case(case_idx)
    p = tmp_path / "f.ibu.gz"
    p.write_bytes(f)
    for path in ("pgz", "sequential"):
        _set_path(monkeypatch, path)
        got = _read(p)
        try:
            _check_outcome(got, f, good, bad_at)
        except AssertionError as e:
            raise AssertionError(f"path {path}: {e}") from None


HEADER_VARIANTS = {
    "fname": dict(fname=b"records.ibu"),
    "fcomment": dict(fcomment=b"a comment"),
    "fname_fcomment": dict(fname=b"r.ibu", fcomment=b"c"),
    "fhcrc": dict(fhcrc=True),
    "fhcrc_wrong": dict(fhcrc=True, hcrc=0x1234),
    "reserved_20": dict(reserved=0x20),
    "reserved_80": dict(reserved=0x80),
    "bc_after_other": dict(sub_before=b"XY\x03\x00abc"),
    "bc_before_other": dict(sub_after=b"ZZ\x01\x00q"),
    "everything": dict(fname=b"n", fcomment=b"cc", fhcrc=True, sub_before=b"AB\x00\x00", sub_after=b"CD\x02\x00xy"),
}
# Python's gzip module reads the gzip header itself and neither checks FHCRC nor refuses reserved flag bits; zlib (and with it
# every decoder of this project and the reference's flate2 for FHCRC) refuses both.  zlib is the yardstick; gzip.decompress
# agrees everywhere else.
GZIP_MODULE_LENIENT = {"fhcrc_wrong", "reserved_20", "reserved_80"}


def _bgzf_variant(kw, where):
    """A BGZF file whose member `where` ("head", "middle", "all") carries the header variant."""
    recs = [HEADER + _records(30, 11), _records(120, 12), _records(80, 13), _records(60, 14)]
    out, good, spans = bytearray(), bytearray(), []
    for i, blk in enumerate(recs):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        cd = c.compress(blk) + c.flush()
        odd = where == "all" or (where == "head" and i == 0) or (where == "middle" and i == 2)
        m = dc.member(cd, len(blk), zlib.crc32(blk), **(kw if odd else {}))
        spans.append((len(out) + len(m) - 8 - len(cd), len(cd), len(good), odd))
        out += m
        good += blk
    out += dc.BGZF_EOF
    return bytes(out), bytes(good), spans


@pytest.mark.parametrize("where", ["head", "middle", "all"])
@pytest.mark.parametrize("variant", sorted(HEADER_VARIANTS))
def test_gzip_header_flags_of_bgzf_members(tmp_path, monkeypatch, variant, where):
    f, good, spans = _bgzf_variant(HEADER_VARIANTS[variant], where)
    want, err = dc.gunzip_members(f)
    if variant not in GZIP_MODULE_LENIENT:
        try:
            assert gzip.decompress(f) == want and err is None
        except (OSError, EOFError, zlib.error):
            assert err is not None
    bad_at = next(o for (_, _, o, odd) in spans if odd)
    p = tmp_path / "f.ibu.gz"
    p.write_bytes(f)
    for path in PATHS + ("pgz",):
        _set_path(monkeypatch, path)
        got = _read(p)
        try:
            _check_outcome(got, f, good, bad_at)
        except AssertionError as e:
            raise AssertionError(f"path {path}: {e}") from None
    # the walk the device loaders use: each member it describes is described exactly; it may refuse an odd member (Niffler)
    blocks, consumed, total, rc = ia.bgzf_scan(f)
    assert len(blocks) <= len(spans) + 1
    for b, (coff, clen, ooff, _) in zip(blocks, spans):
        assert (b.comp_offset, b.comp_len, b.out_offset) == (coff, clen, ooff)
    if rc == 0:
        assert err is None and len(blocks) == len(spans) + 1 and consumed == len(f) and total == len(want)
    else:
        assert rc == 2 and len(blocks) < len(spans) and spans[len(blocks)][3]   # it stops AT an odd member


@pytest.mark.parametrize("path", PATHS)
def test_a_batch_of_nothing_but_valid_empty_blocks(tmp_path, monkeypatch, path):
    """Valid blocks with empty output that are not the EOF marker (a dynamic block holding only end-of-block, 42 bytes), so many
    of them that a whole batch of the BGZF source (IBU_BGZF_BATCH, its least 128 KiB) inflates to nothing: zlib's inflate must
    still be given an output pointer."""
    _, comp, data, isize, crc = next(c for c in CASES if c[0] == "dyn_eob_only")
    first, last = HEADER + _records(50, 21), _records(70, 22)
    out = bytearray()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cd = c.compress(first) + c.flush()
    out += dc.member(cd, len(first), zlib.crc32(first))
    out += dc.member(comp, 0, 0) * (8 * (128 << 10) // (len(comp) + 26))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cd = c.compress(last) + c.flush()
    out += dc.member(cd, len(last), zlib.crc32(last)) + dc.BGZF_EOF
    f = bytes(out)
    assert dc.gunzip_members(f) == (first + last, None)
    p = tmp_path / "f.ibu.gz"
    p.write_bytes(f)
    _set_path(monkeypatch, path)
    monkeypatch.setenv("IBU_BGZF_BATCH", str(128 << 10))
    assert _read(p) == ((first + last)[32:], None)
