"""GPU tests of the pull stream over a path (ibu_stream_open_path, csrc/stream.cpp): Reader::from_path + the stream, with a BGZF file read
in ranges whose blocks are inflated on the device.  Every comparison is against the oracle's iterator or against ibu_stream_open_reader
(Reader.device_stream) on the same file and ring: the concatenated batches, first_index, the batch-size rule, the errors and their detail,
and stats.bytes_h2d below records x 24 — the proof that the compressed bytes, not the records, crossed the link."""
import contextlib
import gzip
import math
import struct

import numpy as np
import pytest

from tests import deflate_craft as dc
from tests.bgzf import bgzf_compress

pytestmark = pytest.mark.gpu

SEED = 0x1B00030
REFILL = 49_152
RINGS = [{"slots": 2, "slot_records": 1000, "feeder_threads": 2}, {"slots": 3, "slot_records": REFILL, "feeder_threads": 2},
         {"slots": 4, "slot_records": 65_536, "feeder_threads": 2}, {"slots": 2, "slot_records": 4 << 20, "feeder_threads": 4}]


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def _opts(ctx, **kv):
    """Context options for the length of a block, back to their defaults afterwards."""
    defaults = {"bgzf_range_bytes": 0, "bgzf_device": 1, "bgzf_stream_ahead": 1}
    try:
        for k, v in kv.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kv:
            ctx.set_option(k, defaults[k])


_FILES = {}


def _plain(oracle, n, bc_len=16, umi_len=12):
    key = (n, bc_len, umi_len)
    if key not in _FILES:
        recs = oracle.generate(SEED + n, 0, n, bc_len, umi_len)
        hdr = struct.pack("<IIIIQ8s", 0x21554249, 2, bc_len, umi_len, 0, b"\0" * 8)
        _FILES[key] = (recs, hdr + recs.tobytes())
    return _FILES[key]


def _range_target(comp_len, n, refills):
    """bgzf_range_bytes for ranges of `refills` refills at the file's ratio."""
    return math.ceil(comp_len * refills * REFILL / max(n, 1)) + 1


def _slot(ring):
    return (ring["slot_records"] + 127) // 128 * 128


def _pull(stream, check_align=True):
    """(batches [(first_index, n)], records as one byte string, the error or None), every batch released in order."""
    batches, parts, err = [], [], None
    try:
        for b in stream:
            with b:
                assert not check_align or b.ptr % 16 == 0
                batches.append((b.first_index, b.n))
                parts.append(b.download().tobytes())
    except Exception as e:                                          # noqa: BLE001 (compared below)
        err = e
    return batches, b"".join(parts), err


def _reader_pull(ia, ctx, path, ring):
    r = ia.Reader.from_path(path)
    try:
        s = r.device_stream(ctx, ring=ring)
        try:
            out = _pull(s)
            st = s.stats()
        finally:
            s.close()
    finally:
        r.close()
    return out, st


def _path_pull(ia, ctx, path, ring):
    with ia.DeviceStream.from_path(path, ctx, ring=ring) as s:
        out = _pull(s)
        st = s.stats()
    return out, st


def _same_error(a, b):
    if a is None or b is None:
        return a is None and b is None
    return (type(a), getattr(a, "kind", None), getattr(a, "a", None), getattr(a, "b", None), str(a)) == \
           (type(b), getattr(b, "kind", None), getattr(b, "a", None), getattr(b, "b", None), str(b))


def _check_batches(batches, n, slot):
    at = 0
    for i, (first, bn) in enumerate(batches):
        assert first == at and 0 < bn <= slot
        at += bn
        if i + 1 < len(batches):                                    # a short batch only at a range's end (ranges: whole refills)
            assert bn == slot or at % REFILL == 0, (i, first, bn)
    assert at == n


@pytest.mark.parametrize("ranges", ["one", "many"])
@pytest.mark.parametrize("ring", range(4))
@pytest.mark.parametrize("n", [0, 1, REFILL - 1, REFILL + 1, 1_000_003])
def test_parity_with_the_oracle(ia, ctx, oracle, tmp_path, n, ring, ranges):
    recs, plain = _plain(oracle, n)
    comp = bgzf_compress(plain)
    p = tmp_path / "f.ibu.gz"
    p.write_bytes(comp)
    ring = RINGS[ring]
    with _opts(ctx, bgzf_range_bytes=_range_target(len(comp), n, 1) if ranges == "many" else 0):
        (batches, got, err), st = _path_pull(ia, ctx, p, ring)
    assert err is None
    assert got == recs.tobytes()
    _check_batches(batches, n, _slot(ring))
    assert (st.records, st.batches) == (n, len(batches))
    if ranges == "one" and n:                                       # one range: every batch but the last is a whole slot
        assert all(bn == _slot(ring) for _, bn in batches[:-1])
    if n >= REFILL - 1:
        assert 0 < st.bytes_h2d < n * 24, (st.bytes_h2d, n * 24)    # the compressed bytes crossed the link, not the records


@pytest.mark.parametrize("lens", [(32, 32), (1, 1)])
@pytest.mark.parametrize("n", [REFILL + 1, 1_000_003])
@pytest.mark.parametrize("ahead", [0, 1])
def test_parity_other_lengths_and_both_launch_forms(ia, ctx, oracle, tmp_path, lens, n, ahead):
    recs, plain = _plain(oracle, n, *lens)
    comp = bgzf_compress(plain, block=4093)
    p = tmp_path / "l.ibu.gz"
    p.write_bytes(comp)
    ring = RINGS[2]
    with _opts(ctx, bgzf_range_bytes=_range_target(len(comp), n, 2), bgzf_stream_ahead=ahead):
        (batches, got, err), st = _path_pull(ia, ctx, p, ring)
        with ia.DeviceStream.from_path(p, ctx, ring=ring) as s:
            h = s.header()
    assert err is None and got == recs.tobytes() and (h.bc_len, h.umi_len) == lens
    _check_batches(batches, n, _slot(ring))
    assert st.bytes_h2d < n * 24


def _zstd(data):
    import ctypes as C
    z = C.CDLL("libzstd.so.1")
    z.ZSTD_compressBound.restype = C.c_size_t
    z.ZSTD_compress.restype = C.c_size_t
    z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    out = C.create_string_buffer(z.ZSTD_compressBound(C.c_size_t(len(data))))
    k = z.ZSTD_compress(out, len(out), data, len(data), 1)
    return out.raw[:k]


def _corrupt_crc(comp, block):
    b = bytearray(comp)
    at = block["comp_offset"] + block["comp_len"]
    struct.pack_into("<I", b, at, struct.unpack_from("<I", b, at)[0] ^ 1)
    return bytes(b)


def _blocks(ia, comp):
    blocks, _, _, rc = ia.bgzf_scan(comp)
    assert rc == 0
    return [{"comp_offset": b.comp_offset, "comp_len": b.comp_len, "out_offset": b.out_offset, "out_len": b.out_len} for b in blocks]


def _block_at(blocks, byte):
    return next(b for b in blocks if b["out_offset"] <= byte < b["out_offset"] + b["out_len"])


@pytest.mark.parametrize("case", ["plain", "gzip", "zstd", "foreign_member", "cut_in_block", "bad_crc_only_range", "bad_crc_range_3_of_4",
                                  "bgzf_device_0"])
@pytest.mark.parametrize("ring", [0, 2])
def test_fallbacks_match_the_reader_stream(ia, ctx, oracle, tmp_path, case, ring):
    n = 4 * REFILL if case == "bad_crc_range_3_of_4" else 300_007
    recs, plain = _plain(oracle, n)
    comp = bgzf_compress(plain, block=0x7F00)
    opts = {}
    stats_too = True
    if case == "plain":
        data = plain
    elif case == "gzip":
        data = gzip.compress(plain, 1)
    elif case == "zstd":
        data = _zstd(plain)
    elif case == "foreign_member":
        cut = 32 + 24 * 100_000 + 5
        data = bgzf_compress(plain[:cut], eof=False) + gzip.compress(plain[cut:cut + 24 * 1000], 1) + bgzf_compress(plain[cut + 24 * 1000:])
    elif case == "cut_in_block":
        data = comp[:len(comp) // 2 + 7]
    elif case == "bad_crc_only_range":
        data = _corrupt_crc(comp, _block_at(_blocks(ia, comp), 32 + 24 * 150_000))
        stats_too = False
    elif case == "bad_crc_range_3_of_4":
        data = _corrupt_crc(comp, _block_at(_blocks(ia, comp), 32 + 24 * (2 * REFILL + REFILL // 2)))
        opts = {"bgzf_range_bytes": _range_target(len(comp), n, 1)}
        stats_too = False
    else:
        data = comp
        opts = {"bgzf_device": 0}
    p = tmp_path / "fb.bin"
    p.write_bytes(data)
    ring = RINGS[ring]
    with _opts(ctx, **opts):
        (pb, pgot, perr), pst = _path_pull(ia, ctx, p, ring)
        (rb, rgot, rerr), rst = _reader_pull(ia, ctx, p, ring)
    assert pgot == rgot and _same_error(perr, rerr), (perr, rerr)
    if case in ("plain", "gzip", "bgzf_device_0"):
        assert perr is None and pgot == recs.tobytes()
    if case.startswith("bad_crc"):
        assert perr.kind == "Niffler" and len(pgot) % (24 * REFILL) == 0
    if case == "bad_crc_range_3_of_4":
        assert len(pgot) == 24 * 2 * REFILL                       # ranges 1 and 2 from the device, nothing of the refill the block spoils
    if stats_too:
        assert (pb, pst.records, pst.batches, pst.bytes_h2d) == (rb, rst.records, rst.batches, rst.bytes_h2d)
    # Reader.process_device on the same file, on the device form and through the Reader's host inflate: the same result or error
    reduce_, decode = {}, {}
    for dev in (1, 0):
        with _opts(ctx, **{**opts, "bgzf_device": dev}):
            reduce_[dev] = _process(ia, ctx, p, ring, ia.PROC_REDUCE)
            decode[dev] = _process(ia, ctx, p, ring, ia.PROC_DECODE, n)
    for got in (reduce_, decode):
        (r1, e1), (r0, e0) = got[1], got[0]
        assert _same_error(e1, e0) and r1 == r0, (case, e1, e0)
    if reduce_[0][1] is None:
        assert reduce_[0][0] == oracle.reduce_records(recs)
    if case == "bad_crc_range_3_of_4":                              # the rows of ranges 1 and 2, decoded on the device before the error
        bc, umi, idx = oracle.decode_records(recs[:2 * REFILL], 16, 12)
        for dev in (1, 0):
            cols = decode[dev][0]
            assert (cols[0][:len(bc.tobytes())], cols[1][:len(umi.tobytes())], cols[2][:len(idx.tobytes())]) == \
                   (bc.tobytes(), umi.tobytes(), idx.tobytes()), dev


def _process(ia, ctx, path, ring, proc, n=0):
    """Reader.from_path(path).process_device: (the reduce result / the decoded columns of a sink of n rows, the error or None)."""
    r = ia.Reader.from_path(path)
    cols = [ctx.alloc(max(n, 1) * w) for w in (16, 12, 8)] if proc == ia.PROC_DECODE else None
    if cols:
        for c in cols:
            c.upload(np.zeros(c.nbytes, np.uint8))
    res, err = None, None
    try:
        res, _ = r.process_device(ctx, proc, sink=tuple(cols) if cols else None, ring=ring)
    except ia.IbuError as e:
        err = e
    finally:
        r.close()
    if cols:
        res = tuple(c.download().tobytes()[:n * w] for c, w in zip(cols, (16, 12, 8)))
        for c in cols:
            c.free()
    return res, err


def _ranged(ia, ctx, oracle, tmp_path, n, refills_per_range):
    recs, plain = _plain(oracle, n)
    comp = bgzf_compress(plain)
    p = tmp_path / "h.ibu.gz"
    p.write_bytes(comp)
    return recs, p, _range_target(len(comp), n, refills_per_range)


def test_holding_a_batch_of_range_k_blocks_range_k_plus_2_without_hanging(ia, ctx, oracle, tmp_path):
    recs, p, target = _ranged(ia, ctx, oracle, tmp_path, 4 * REFILL, 1)
    ring = {"slots": 2, "slot_records": REFILL, "feeder_threads": 2}   # one batch per range
    with _opts(ctx, bgzf_range_bytes=target), ia.DeviceStream.from_path(p, ctx, ring=ring) as s:
        b0 = s.next_batch()                                         # range 0, held
        b1 = s.next_batch()                                         # range 1: all of it
        assert (b0.first_index, b1.first_index) == (0, REFILL)
        with pytest.raises(ia.IbuError) as e:                       # range 2 goes to b0's buffer
            s.next_batch()
        assert e.value.kind == "InvalidArg"
        with pytest.raises(ia.IbuError):                            # again: nothing changed
            s.next_batch()
        got0 = b0.download().tobytes()
        b0.release()
        b2 = s.next_batch()                                         # the same call succeeds now
        assert b2.first_index == 2 * REFILL
        got = got0 + b1.download().tobytes() + b2.download().tobytes()
        b1.release()
        b2.release()
        rest = _pull(s)
        assert rest[2] is None
    assert got + rest[1] == recs.tobytes()


def test_batches_of_a_range_released_out_of_order(ia, ctx, oracle, tmp_path):
    recs, p, target = _ranged(ia, ctx, oracle, tmp_path, 6 * REFILL + 999, 2)
    ring = {"slots": 2, "slot_records": REFILL, "feeder_threads": 2}   # two batches per range
    parts = {}
    with _opts(ctx, bgzf_range_bytes=target), ia.DeviceStream.from_path(p, ctx, ring=ring) as s:
        while True:
            a = s.next_batch()
            if a is None:
                break
            b = s.next_batch()
            for x in (a, b):
                if x is not None:
                    parts[x.first_index] = x.download().tobytes()
            if b is not None:
                b.release()
            a.release()
    assert b"".join(parts[k] for k in sorted(parts)) == recs.tobytes()


def test_close_mid_load_and_destroy_the_context_under_an_open_stream(ia, oracle, tmp_path):
    c = ia.Context(0)
    recs, p, target = _ranged(ia, c, oracle, tmp_path, 1_000_003, 3)
    c.set_option("bgzf_range_bytes", target)
    s = ia.DeviceStream.from_path(p, c, ring=RINGS[1])
    b = s.next_batch()                                              # the next range is loading
    assert b.download().tobytes() == recs[:REFILL].tobytes()
    s.close()                                                       # with a batch held and a load in flight
    s = ia.DeviceStream.from_path(p, c, ring=RINGS[1])
    b = s.next_batch()
    c.close()                                                       # the stream becomes an orphan
    with pytest.raises(ia.IbuError) as e:
        s.next_batch()
    assert e.value.kind == "InvalidArg"
    with pytest.raises(ia.IbuError):
        b.release()
    s.close()
    c2 = ia.Context(0)                                              # the device is fine afterwards
    d = c2.alloc(24 * 256)
    c2.generate(1, 0, 256, 16, 12, d)
    assert c2.reduce(d, 256)["count"] == 256
    c2.close()


def test_library_kernels_on_a_held_batch_while_the_next_range_loads(ia, ctx, oracle, tmp_path):
    """The caller's decode and sort on the SAME context, on a second stream, over each batch while the producer loads the next range."""
    n, bc_len, umi_len = 8 * REFILL + 4321, 16, 12
    recs, p, target = _ranged(ia, ctx, oracle, tmp_path, n, 2)
    other = ia.Context(0)
    st = other.stream
    slot = REFILL
    d_bc, d_umi, d_idx = ctx.alloc(n * bc_len), ctx.alloc(n * umi_len), ctx.alloc(n * 8)
    d_sorted, d_tmp = ctx.alloc(slot * 24), ctx.alloc(slot * 24)
    sorted_batches = []
    with _opts(ctx, bgzf_range_bytes=target), ia.DeviceStream.from_path(p, ctx, ring={"slots": 2, "slot_records": slot, "feeder_threads": 2}) as s:
        while True:
            b = s.next_batch(stream=st)
            if b is None:
                break
            row = b.first_index
            ctx.decode_ascii(b.ptr, b.n, bc_len, umi_len, d_bc.ptr + row * bc_len, d_umi.ptr + row * umi_len, d_idx.ptr + row * 8, stream=st)
            ctx.copy(d_sorted, b.ptr, b.n * 24, stream=st)
            b.release(stream=st)                                    # the buffer may be loaded again once decode and copy have run
            ctx.sort_records(d_sorted, d_tmp, b.n, stream=st)
            other.synchronize(st)
            sorted_batches.append((row, b.n, d_sorted.download(count=b.n * 24).view(ia.REC_DTYPE).copy()))
        assert s.stats().bytes_h2d < n * 24
    other.synchronize(st)
    bc, umi, idx = oracle.decode_records(recs, bc_len, umi_len)
    assert d_bc.download().tobytes() == bc.tobytes() and d_umi.download().tobytes() == umi.tobytes()
    assert d_idx.download(np.uint64).tobytes() == idx.tobytes()
    assert sum(bn for _, bn, _ in sorted_batches) == n
    for row, bn, got in sorted_batches:
        assert got.tobytes() == oracle.sort_records(recs[row:row + bn]).tobytes()
    other.close()


def test_empty_blocks_and_a_header_across_blocks(ia, ctx, oracle, tmp_path):
    n = 3 * REFILL + 11
    recs, plain = _plain(oracle, n)
    edge = 32 + 24 * REFILL
    cuts = [0, 7, 7, 32, 32, 5000, edge - 100, edge - 100, edge, edge, edge + 9000, 2 * edge, len(plain)]
    comp = b"".join(bgzf_compress(plain[a:z], eof=False) if z > a else dc.BGZF_EOF for a, z in zip(cuts, cuts[1:])) + dc.BGZF_EOF
    p = tmp_path / "e.ibu.gz"
    p.write_bytes(comp)
    with _opts(ctx, bgzf_range_bytes=_range_target(len(comp), n, 1)):
        (batches, got, err), st = _path_pull(ia, ctx, p, RINGS[0])
    assert err is None and got == recs.tobytes() and st.bytes_h2d < n * 24
    _check_batches(batches, n, _slot(RINGS[0]))
