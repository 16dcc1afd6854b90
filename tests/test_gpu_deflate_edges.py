"""The device DEFLATE decoder (k_inflate.hip) and the BGZF loads on the corpus of tests/deflate_craft.py: streams no compressor
writes (single 1-bit codes, symbols 286/287 and 30/31, distances to exactly the first byte, repeat runs across the two code
length lists, 0 to 2 byte blocks, ...), each judged by zlib's inflate.  A case runs in one lane of a wave whose other lanes
inflate long zlib blocks, so its lane diverges from its neighbours, at lane 0, 37 and 63, through both forms of the kernel (the
scratch-table form takes calls of more than 3 x cus waves); the blocks' outputs lie between guard bytes, none of which may
change.  End to end, the files with an invalid empty block or an FNAME member go through every device load and must read as
zlib reads them (the loads may refuse what they do not take: Niffler).  The host decoders: test_deflate_edges.py."""
import struct
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc

pytestmark = pytest.mark.gpu

CASES = dc.all_cases()
PAD = 2048
GAP = 64              # guard bytes (0xA5) in front of and behind every block's output range
LANES = (0, 37, 63)


@pytest.fixture(scope="module")
def ia():
    import ibu_amd
    return ibu_amd


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.Context(0)
    yield c
    c.close()


def _filler(n_bytes, seed):
    rng = np.random.default_rng(seed)
    data = (rng.integers(0, 1 << 20, n_bytes // 8, dtype=np.uint64) * 0x10001).tobytes()[:n_bytes]
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush(), data


def _run(ia, ctx, n_blocks, placed, filler):
    """Inflate n_blocks blocks: the cases placed[i] = (block index, case) there, the filler (comp, data) everywhere else.
    Checks statuses, bytes and guard zones; returns the number of blocks that were cases."""
    fcomp, fdata = filler
    comp = bytearray(fcomp)
    at = {}
    for i, case in placed:
        at[i] = (len(comp), case)
        comp += case[1]
    desc = np.zeros(n_blocks, ia.INFLATE_BLOCK_DTYPE)
    want_st = np.zeros(n_blocks, np.uint32)
    out_off, spans = GAP, []
    for i in range(n_blocks):
        if i in at:
            off, (_, raw, data, isize, crc) = at[i]
            desc[i] = (off, out_off, len(raw), isize & 0xFFFFFFFF, crc & 0xFFFFFFFF, 0)
            want_st[i] = dc.device_status(raw, isize, crc)
            spans.append((out_off, isize, data if want_st[i] == 0 else None))
            out_off += isize + GAP
        else:
            desc[i] = (0, out_off, len(fcomp), len(fdata), zlib.crc32(fdata), 0)
            spans.append((out_off, len(fdata), fdata))
            out_off += len(fdata) + GAP
    assert desc["out_len"].max() <= 65536
    d_comp = ctx.alloc(len(comp) + PAD)
    d_comp.upload(np.frombuffer(bytes(comp) + bytes(PAD), np.uint8))
    d_out = ctx.alloc(out_off)
    d_out.upload(np.full(out_off, 0xA5, np.uint8))
    try:
        st, first = ctx.inflate_blocks(d_comp, desc, d_out)
        got = d_out.download(np.uint8)
    finally:
        d_comp.free()
        d_out.free()
    bad = np.nonzero(st != want_st)[0]
    assert len(bad) == 0, [(int(i), at[i][1][0] if i in at else "filler", int(st[i]), int(want_st[i])) for i in bad[:10]]
    nz = np.nonzero(want_st)[0]
    assert first == (int(nz[0]) if len(nz) else None)
    inside = np.zeros(out_off, bool)
    for i, (o, n, data) in enumerate(spans):
        inside[o:o + n] = True
        if data is not None:
            assert got[o:o + n].tobytes() == data, (i, at[i][1][0] if i in at else "filler")
    assert (got[~inside] == 0xA5).all(), "a byte outside every block's output range was written"
    return len(at)


@pytest.mark.parametrize("lane", LANES)
def test_every_case_in_a_diverging_lane(ia, ctx, lane):
    """One wave per case, the case at `lane`, the other 63 lanes inflating 24 KiB zlib blocks (the short form: one round)."""
    placed = [(64 * k + lane, c) for k, c in enumerate(CASES)]
    assert _run(ia, ctx, 64 * len(CASES), placed, _filler(24 << 10, lane)) == len(CASES)


def test_every_case_in_the_scratch_table_form(ia, ctx):
    """More blocks than three waves per CU hold (70 000 tiny ones): the form with its tables in scratch; every case at lanes 0,
    37 and 63 of waves spread over the call."""
    n = 70_000
    placed, k = [], 0
    for j, c in enumerate(CASES):
        for lane in LANES:
            placed.append((64 * (7 + 7 * k) + lane, c))
            k += 1
    assert max(i for i, _ in placed) < n
    assert _run(ia, ctx, n, placed, _filler(48, 99)) == len(placed)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _file(odd, where, oracle, seed):
    """(file bytes, records) — a BGZF file of the records (the 32-byte header in block 0) with one odd member: "empty_01_00" /
    "empty_03_00" (a 2-byte block with empty output), or "fname" (a member whose header carries FNAME)."""
    n = 40_000
    recs = oracle.generate(seed, 0, n, 16, 12)
    plain = struct.pack("<IIIIQ8s", 0x21554249, 2, 16, 12, 0, b"\0" * 8) + recs.tobytes()
    pieces = [plain[i:i + 0xFF00] for i in range(0, len(plain), 0xFF00)]
    members = []
    for i, pc in enumerate(pieces):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        cd = c.compress(pc) + c.flush()
        members.append(dict(comp=cd, data_len=len(pc), crc=zlib.crc32(pc)))
    at = {"head": 0, "middle": len(members) // 2, "tail": len(members)}[where]
    if odd == "fname":
        members[min(at, len(members) - 1)]["fname"] = b"records.ibu"
    else:
        members.insert(at, dict(comp=b"\x01\x00" if odd == "empty_01_00" else b"\x03\x00", data_len=0, crc=0))
    f = b"".join(dc.member(**m) for m in members) + dc.BGZF_EOF
    return f, recs


FILES = [("empty_01_00", "head"), ("empty_01_00", "middle"), ("empty_01_00", "tail"), ("fname", "head"), ("fname", "middle"),
         ("empty_03_00", "middle")]


@pytest.mark.parametrize("odd,where", FILES)
def test_odd_members_through_every_device_load(ia, oracle, tmp_path, odd, where):
    f, rec_arr = _file(odd, where, oracle, 0x1B00D0 + len(where))
    recs = rec_arr.tobytes()
    want, err = dc.gunzip_members(f)
    assert (err is None) == (odd != "empty_01_00")
    if err is None:
        assert want[32:] == recs
    n = len(recs) // 24
    p = tmp_path / "f.ibu.gz"
    p.write_bytes(f)
    ring = {"slots": 3, "slot_records": 20_000, "feeder_threads": 2}
    c = ia.Context(0)
    try:
        try:                                                     # the whole file
            h, q, got_n, st = c.load_bgzf_to_device(str(p), ring=ring)
            assert err is None and got_n == n
            assert ia.DeviceBuffer.wrap(c, q, 24 * n).download().tobytes() == recs
            c.free(q)
        except ia.IbuError as e:
            assert e.kind == "Niffler" and err is not None, e
        for k in (2, 3):                                         # shards: the odd block a lead, device or edge block
            per, refused = n // k, 0
            for i in range(k):
                try:
                    h, q, got_n, first, st = c.load_bgzf_shard_to_device(str(p), i, k, ring=ring)
                except ia.IbuError as e:
                    assert e.kind == "Niffler" and err is not None, e
                    refused += 1
                    continue
                assert first == i * per and got_n == (per if i + 1 < k else n - per * (k - 1))
                if got_n:
                    assert ia.DeviceBuffer.wrap(c, q, 24 * got_n).download().tobytes() == recs[24 * first:24 * (first + got_n)]
                if q:
                    c.free(q)
            if err is not None:
                assert refused >= 1                              # the shard that holds the bad block does not take it
        pulled, kind, r = [], None, None
        try:                                                     # the pull stream
            r = ia.Reader.from_path(p)
            with r.device_stream(c, ring=ring) as s:
                for b in s:
                    with b:
                        pulled.append(b.download().copy().tobytes())
        except ia.IbuError as e:
            kind = e.kind
        finally:
            if r is not None:
                r.close()
        got = b"".join(pulled)
        if err is None:
            assert kind is None and got == recs
        else:
            assert kind == "Niffler" and recs.startswith(got)
        outcomes = {}
        for dev in (1, 0):                                       # Reader.process_device, on the device and on the host
            c.set_option("bgzf_device", dev)
            r = None
            try:
                r = ia.Reader.from_path(p)
                res, st = r.process_device(c, ia.PROC_REDUCE, ring=ring)
                outcomes[dev] = ("ok", res)
            except ia.IbuError as e:
                outcomes[dev] = (e.kind, getattr(e, "pos", None))
            finally:
                if r is not None:
                    r.close()
        c.set_option("bgzf_device", 1)
        assert outcomes[1] == outcomes[0], outcomes
        if err is None:
            assert outcomes[1] == ("ok", oracle.reduce_records(rec_arr))
        else:
            assert outcomes[1][0] == "Niffler"
    finally:
        c.close()
