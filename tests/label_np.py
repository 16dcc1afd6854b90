"""The numpy statement of the per-barcode labels (include/ibu_hip.h: ibu_labels_create, ibu_labels_set, ibu_labels_get,
ibu_label_records), written from the header comment alone.  Test infrastructure: the product never imports it.

A label table holds one byte per whitelist entry, all `fill` at first.  set: the label of a code that is an entry becomes the byte
given with it; a code that is no entry — not in the whitelist, or with bits at or above 2*bc_len — is skipped and counted.  get:
the label of an entry, `missing` for anything else.  label_records: a record is found when barcode & mask(2*bc_len) is an entry;
plain mode gives it the label (missing_class where not found), match mode 0 / 1 / 2 for label == match / another label / not
found; the histogram counts the found records per label in bins 0..255 and the records not found in bin 256, in either mode."""
import numpy as np

from tests import whitelist_np as wnp

REC = wnp.REC
IS, OTHER, MISSING = 0, 1, 2
BINS = 257


class Labels:
    """The labels of a whitelist: `wl` its distinct codes, ascending, `lab[k]` the label of wl[k]."""

    def __init__(self, whitelist, bc_len, fill=255):
        if not 0 <= fill <= 255:
            raise ValueError("fill is a byte")
        self.wl = np.unique(np.asarray(whitelist, dtype=np.uint64))
        self.bc_len = bc_len
        self.lab = np.full(len(self.wl), fill, np.uint8)


def _find(lb, keys):
    """-> (position of every key in lb.wl, whether it is there).  No entry has bits at or above 2*bc_len, so a key with such bits
    is never found."""
    keys = np.asarray(keys, dtype=np.uint64)
    pos = np.searchsorted(lb.wl, keys)
    pos[pos == len(lb.wl)] = 0
    return pos, lb.wl[pos] == keys


def set_labels(lb, codes, labels):
    """ibu_labels_set -> the number of codes skipped.  Codes that occur twice: the last one wins here (the device promises only one
    of them), so the tests give distinct codes per call."""
    codes = np.asarray(codes, dtype=np.uint64).reshape(-1)
    labels = np.asarray(labels, dtype=np.uint8).reshape(-1)
    assert len(codes) == len(labels)
    pos, hit = _find(lb, codes)
    lb.lab[pos[hit]] = labels[hit]
    return int((~hit).sum())


def get_labels(lb, codes, missing=255):
    """ibu_labels_get."""
    pos, hit = _find(lb, codes)
    return np.where(hit, lb.lab[pos], np.uint8(missing)).astype(np.uint8)


def _barcodes(recs_or_bc):
    a = np.asarray(recs_or_bc)
    return a["barcode"] if a.dtype.names else a.astype(np.uint64)


def label_records(lb, recs, match=None, missing_class=255):
    """ibu_label_records -> (class bytes, the 257-bin histogram).  match=None: plain mode."""
    bc = _barcodes(recs)
    low = bc & wnp.mask(lb.bc_len) if lb.bc_len < 32 else bc
    pos, hit = _find(lb, low)
    bins = np.where(hit, lb.lab[pos].astype(np.int64), 256)
    hist = np.bincount(bins, minlength=BINS).astype(np.uint64)
    if match is None:
        cls = np.where(hit, lb.lab[pos], np.uint8(missing_class)).astype(np.uint8)
    else:
        cls = np.where(~hit, MISSING, np.where(lb.lab[pos] == match, IS, OTHER)).astype(np.uint8)
    return cls, hist


# ---- brute force: a Python dict ------------------------------------------------------------------------------------------------
def brute_table(whitelist, bc_len, fill=255):
    return {int(c): fill for c in whitelist}


def brute_set(table, bc_len, codes, labels):
    skipped = 0
    for c, v in zip((int(x) for x in codes), (int(x) for x in labels)):
        if c >> (2 * bc_len) or c not in table:
            skipped += 1
        else:
            table[c] = v
    return skipped


def brute_label(table, bc_len, barcodes, match=None, missing_class=255):
    m = (1 << (2 * bc_len)) - 1
    cls, hist = [], [0] * BINS
    for b in (int(v) for v in barcodes):
        lab = table.get(b & m)
        hist[256 if lab is None else lab] += 1
        if match is None:
            cls.append(missing_class if lab is None else lab)
        else:
            cls.append(MISSING if lab is None else IS if lab == match else OTHER)
    return np.array(cls, np.uint8), np.array(hist, np.uint64)


# ---- case builders, shared by tests/test_label_host.py and tests/test_gpu_labels.py -----------------------------------------------
def records(rng, bc):
    recs = np.zeros(len(bc), REC)
    recs["barcode"] = bc
    recs["umi"] = rng.integers(0, 1 << 63, len(bc), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, len(bc), dtype=np.uint64)
    recs["index"] = np.arange(len(bc), dtype=np.uint64)
    return recs


def whitelist(rng, bc_len, w, ones=False):
    """w distinct random codes (as many as the code space has where it is smaller); at 32 bases with the all-ones key on request."""
    space = 4 ** bc_len
    if space <= 4 * w:
        wl = rng.permutation(space)[:min(w, space)].astype(np.uint64)
    else:
        wl = np.unique(wnp.random_codes(rng, bc_len, 2 * w))
        wl = rng.permutation(wl[wl != np.uint64(wnp.FREE)])[:w]
    if ones:
        assert bc_len == 32
        wl[0] = np.uint64(wnp.FREE)
    return wl


def outsiders(rng, wl, bc_len, count):
    """`count` codes that are not in the whitelist: one substitution of an entry, filtered (none where the whitelist is the whole
    code space)."""
    if len(np.unique(wl)) >= 4 ** bc_len:
        return np.empty(0, np.uint64)
    out = wnp.substitute(rng, wl[rng.integers(0, len(wl), 2 * count + 16)], bc_len)
    out = out[~np.isin(out, wl)]
    return np.resize(out, count) if 0 < len(out) < count else out[:count]   # (a nearly full code space has few: they repeat)


def barcodes(rng, wl, bc_len, n, order="shuffled", miss=0.1):
    """n barcodes: about `miss` of them not in the whitelist, the rest entries; junk bits above 2*bc_len on half of them below 32
    bases.  order "shuffled", or "sorted": ascending, with one entry over 300 consecutive records from record 100 on (the run
    crosses the tile seams at 128 and 256, and at 129 and 257 of an array that peels a record) and, where n allows, a run that
    ends exactly at record 128 in front of it."""
    out = outsiders(rng, wl, bc_len, max(int(miss * n), 1))
    k_out = min(len(out), int(round(miss * n)))
    bc = np.concatenate([wl[rng.integers(0, len(wl), n - k_out)], out[:k_out]]) if n else np.empty(0, np.uint64)
    if order == "sorted":
        bc = np.sort(bc)
        if n >= 500:
            bc[100:128] = bc[100]          # a run that ends exactly at record 128 ...
            j = 428 + int(np.flatnonzero(np.isin(bc[428:], wl))[0])
            bc[128:j + 1] = bc[j]          # ... and one of at least 300 records of an ENTRY behind it, over two tile seams (still ascending)
    else:
        bc = rng.permutation(bc)
    return wnp.with_junk(rng, bc, bc_len)


PATTERNS = ("equal", "rank256", "low8")


def label_pattern(wl, pattern):
    """-> (codes to set, their labels).  equal: every entry 7.  rank256: entry of rank r gets r % 256, except every fifth entry,
    which is never set (fill survives there).  low8: labels 0..7 only."""
    u = np.unique(wl)
    r = np.arange(len(u))
    if pattern == "equal":
        return u, np.full(len(u), 7, np.uint8)
    if pattern == "rank256":
        keep = r % 5 != 4
        return u[keep], (r[keep] % 256).astype(np.uint8)
    if pattern == "low8":
        return u, (r * 2654435761 % 8).astype(np.uint8)
    raise ValueError(pattern)
