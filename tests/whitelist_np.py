"""The numpy statement of barcode correction against a whitelist (include/ibu_hip.h, ibu_correct_barcodes), written from
the header comment alone.  Test infrastructure: the product never imports it.

A whitelist is a set of bc_len-base codes.  low = barcode & mask(2*bc_len); a neighbour of low is low ^ (x << 2i) for
i in [0, bc_len), x in {1, 2, 3}.  Classes: 0 exact (low in the whitelist), 1 corrected (not exact, exactly one
neighbour in it: the low bits become that neighbour), 2 ambiguous (not exact, two or more), 3 unmatched."""
import numpy as np

EXACT, CORRECTED, AMBIGUOUS, UNMATCHED = 0, 1, 2, 3
REC = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("index", "<u8")])


def mask(bc_len):
    return np.uint64((1 << (2 * bc_len)) - 1)


def _member(wl_sorted, keys):
    pos = np.searchsorted(wl_sorted, keys)
    pos[pos == len(wl_sorted)] = 0
    return wl_sorted[pos] == keys


def classify(barcodes, whitelist, bc_len, max_mismatches=1):
    """-> (class per barcode as uint8, the barcodes after correction as uint64)."""
    bc = np.ascontiguousarray(barcodes, dtype=np.uint64)
    wl = np.unique(np.asarray(whitelist, dtype=np.uint64))
    m = mask(bc_len)
    low = bc & m
    exact = _member(wl, low)
    cls = np.where(exact, EXACT, UNMATCHED).astype(np.uint8)
    out = bc.copy()
    if max_mismatches == 0:
        return cls, out
    miss = np.flatnonzero(~exact)
    lm = low[miss]
    hits = np.zeros(len(miss), np.int64)
    cand = np.zeros(len(miss), np.uint64)
    for i in range(bc_len):
        for x in (1, 2, 3):
            nb = lm ^ np.uint64(x << (2 * i))
            h = _member(wl, nb)
            cand = np.where(h & (hits == 0), nb, cand)
            hits += h
    cls[miss] = np.where(hits == 1, CORRECTED, np.where(hits >= 2, AMBIGUOUS, UNMATCHED)).astype(np.uint8)
    one = hits == 1
    out[miss[one]] = (bc[miss[one]] & ~m) | cand[one]
    return cls, out


def correct_records(recs, whitelist, bc_len, max_mismatches=1):
    """-> (records after correction, class bytes, {"exact", "corrected", "ambiguous", "unmatched"})."""
    recs = np.ascontiguousarray(recs).view(REC).reshape(-1)
    cls, bc = classify(recs["barcode"], whitelist, bc_len, max_mismatches)
    out = recs.copy()
    out["barcode"] = bc
    n = np.bincount(cls, minlength=4)
    return out, cls, {"exact": int(n[0]), "corrected": int(n[1]), "ambiguous": int(n[2]), "unmatched": int(n[3])}


def select(recs, cls, keep_mask):
    kept = [c for c in range(8) if (keep_mask >> c) & 1]
    return np.ascontiguousarray(recs).view(REC).reshape(-1)[np.isin(cls, kept)]


def brute_force(barcodes, whitelist, bc_len, max_mismatches=1):
    """The same with a Python set and a Hamming loop over the WHITELIST (no neighbour enumeration): small inputs only."""
    m = (1 << (2 * bc_len)) - 1
    wl = sorted({int(c) for c in whitelist})
    wls = set(wl)
    cls, out = [], []
    for b in (int(v) for v in barcodes):
        low = b & m
        if low in wls:
            cls.append(EXACT); out.append(b)
            continue
        near = []
        if max_mismatches:
            for c in wl:
                d = low ^ c
                pairs = (d | (d >> 1)) & 0x5555555555555555   # one bit per base that differs
                if pairs and pairs & (pairs - 1) == 0:
                    near.append(c)
        if len(near) == 1:
            cls.append(CORRECTED); out.append((b & ~m) | near[0])
        else:
            cls.append(AMBIGUOUS if near else UNMATCHED); out.append(b)
    return np.array(cls, np.uint8), np.array(out, np.uint64)


def make_case(rng, bc_len, w, n, junk=True, shares=(0.25, 0.25, 0.25, 0.25)):
    """A whitelist of w distinct random codes holding a planted pair at Hamming distance 2 (their midpoint is
    ambiguous), and n barcodes: `shares` of exact / one substitution / that midpoint / uniform random, shuffled; junk
    bits above 2*bc_len on half the barcodes where bc_len < 32.  -> (whitelist u64[w], barcodes u64[n])."""
    space = 4 ** bc_len
    if w > space:
        raise ValueError("4^bc_len < w")
    if space <= 1 << 20:
        wl = rng.permutation(space)[:w].astype(np.uint64)
    else:
        wl = np.empty(0, np.uint64)
        while len(wl) < w:
            more = rng.integers(0, 1 << 62, size=2 * w, dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, size=2 * w, dtype=np.uint64)
            more &= mask(bc_len)
            wl = np.unique(np.concatenate([wl, more]))
        wl = rng.permutation(wl)[:w]
    mid = None
    if bc_len >= 2 and w >= 2:   # plant the pair: wl[1] = wl[0] with bases 0 and 1 substituted; the midpoint substitutes base 0 only
        a = int(wl[0])
        b = a ^ 0b0110
        midv = a ^ 0b0010
        rest = wl[2:][(wl[2:] != np.uint64(b)) & (wl[2:] != np.uint64(midv))]
        wl = np.concatenate([np.array([a, b], np.uint64), rest])
        mid = midv
    counts = [int(round(s * n)) for s in shares]
    counts[0] += n - sum(counts)
    exact = wl[rng.integers(0, len(wl), counts[0])]
    sub = wl[rng.integers(0, len(wl), counts[1])]
    sub = sub ^ (rng.integers(1, 4, counts[1], dtype=np.uint64) << (np.uint64(2) * rng.integers(0, bc_len, counts[1], dtype=np.uint64)))
    midp = np.full(counts[2], mid if mid is not None else int(wl[0]), np.uint64)
    rnd = (rng.integers(0, 1 << 62, size=counts[3], dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, size=counts[3], dtype=np.uint64)) & mask(bc_len)
    bc = rng.permutation(np.concatenate([exact, sub, midp, rnd]))
    if junk and bc_len < 32:
        j = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) << np.uint64(2 * bc_len)
        bc = np.where(rng.random(n) < 0.5, bc | j, bc)
    return wl, bc


# ---------------------------------------------------------------------------------------------------------------------
# A model of the device table (DESIGN.md "Whitelist", the head of ibu_amd/csrc/k_whitelist.hip): a power of two of slots,
# at least MIN_SLOTS and at least 2 w (w counts the codes as given, duplicates included); home slot = the top
# log2(slots) bits of key * PHI mod 2^64; linear probing; the all-ones key never enters the table.  The device gives no
# view of its table, so this is what lets a test state and assert its premise ("one cluster of 512 slots that starts at
# slot 1023").  The comparisons with the device never depend on it: they go through classify(), which knows no tables.
# ---------------------------------------------------------------------------------------------------------------------
PHI = 0x9E3779B97F4A7C15
PHI_INV = pow(PHI, -1, 1 << 64)
MIN_SLOTS = 1024
FREE = (1 << 64) - 1


def table_slots(w):
    s = MIN_SLOTS
    while s < 2 * w:
        s <<= 1
    return s


def home_slots(keys, slots):
    """The home slot of every key in a table of `slots` slots (uint64 multiplication wraps mod 2^64)."""
    shift = 64 - (slots.bit_length() - 1)
    return ((np.asarray(keys, dtype=np.uint64) * np.uint64(PHI)) >> np.uint64(shift)).astype(np.int64)


def table_model(whitelist, bc_len):
    """-> (slots, home slot of every code of `whitelist` as given, table): `table` is what inserting the codes one after
    the other in the given order leaves, FREE where a slot is free.  Which slots are taken does not depend on the order
    (linear probing); which key sits in which slot of a cluster does."""
    codes = [int(c) for c in np.asarray(whitelist, dtype=np.uint64)]
    if bc_len < 32 and any(c >> (2 * bc_len) for c in codes):
        raise ValueError("a code has bits at or above 2*bc_len")
    slots = table_slots(len(codes))
    homes = home_slots(np.array(codes, np.uint64), slots)
    table = [FREE] * slots
    for c, s in zip(codes, homes.tolist()):
        if c == FREE:                       # out of band (a legal code at 32 bases only)
            continue
        while table[s] != FREE and table[s] != c:
            s = (s + 1) & (slots - 1)
        table[s] = c
    return slots, homes, np.array(table, np.uint64)


def clusters(table):
    """The maximal runs of taken slots of a table_model table as (first slot, length), a run through the last slot into
    slot 0 counted as one (its first slot is then the larger number); longest first."""
    taken = np.asarray(table) != np.uint64(FREE)
    n = len(taken)
    if taken.all():
        return [(0, n)]
    first_free = int(np.flatnonzero(~taken)[0])
    rot = np.roll(taken, -first_free)                                   # rot[0] is free: no run wraps any more
    edge = np.diff(np.concatenate([[0], rot.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    runs = [((int(s) + first_free) % n, int(e - s)) for s, e in zip(starts, ends)]
    return sorted(runs, key=lambda r: (-r[1], r[0]))


def probe_lengths(table, keys):
    """Slots a lookup of each key reads in `table` (the slot that ends the search included)."""
    slots = len(table)
    tab = [int(v) for v in table]
    out = []
    for k, s in zip((int(v) for v in np.asarray(keys, dtype=np.uint64)), home_slots(keys, slots).tolist()):
        steps = 1
        while tab[s] != k and tab[s] != FREE:
            s = (s + 1) & (slots - 1)
            steps += 1
        out.append(steps)
    return np.array(out, np.int64)


def craft_keys(rng, bc_len, slots, homes, count, exclude=()):
    """`count` distinct legal bc_len-base codes (none of them all ones, none in `exclude`) whose home slot in a table of
    `slots` slots is in `homes`.  Below 32 bases: random codes, filtered (every code of the space where it is small); at 32 bases every
    64-bit value is a code, so (home << shift | random low bits) * PHI^-1 mod 2^64 has that home by construction."""
    homes = np.unique(np.asarray(list(homes), dtype=np.int64))
    assert ((homes >= 0) & (homes < slots)).all()
    shift = 64 - (slots.bit_length() - 1)
    exclude = np.append(np.asarray(exclude, dtype=np.uint64), np.uint64(FREE))
    got = np.empty(0, np.uint64)
    if bc_len == 32:
        while len(got) < count:
            h = homes[rng.integers(0, len(homes), 2 * count)].astype(np.uint64)
            v = (h << np.uint64(shift)) | rng.integers(0, 1 << shift, 2 * count, dtype=np.uint64)
            got = np.setdiff1d(np.concatenate([got, v * np.uint64(PHI_INV)]), exclude)
    elif 4 ** bc_len <= 1 << 22:
        every = np.arange(4 ** bc_len, dtype=np.uint64)
        got = np.setdiff1d(every[np.isin(home_slots(every, slots), homes)], exclude)
        if len(got) < count:
            raise ValueError(f"only {len(got)} of the {4 ** bc_len} {bc_len}-base codes have a home slot in {homes.tolist()}")
    else:
        for _ in range(64):
            if len(got) >= count:
                break
            v = (rng.integers(0, 1 << 62, 4_000_000, dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, 4_000_000, dtype=np.uint64)) & mask(bc_len)
            got = np.setdiff1d(np.concatenate([got, v[np.isin(home_slots(v, slots), homes)]]), exclude)
        if len(got) < count:
            raise ValueError(f"too few {bc_len}-base codes with a home slot in {homes.tolist()}")
    return rng.permutation(got)[:count]


# ---------------------------------------------------------------------------------------------------------------------
# Crafted cases, shared by the CPU tests that assert their premises (tests/test_whitelist_host.py) and the GPU tests that
# run them (tests/test_gpu_whitelist_edges.py).
# ---------------------------------------------------------------------------------------------------------------------
def random_codes(rng, bc_len, count):
    return (rng.integers(0, 1 << 62, size=count, dtype=np.uint64) * np.uint64(4) + rng.integers(0, 4, size=count, dtype=np.uint64)) & mask(bc_len)


def substitute(rng, codes, bc_len):
    """Every code with one base, drawn per code, replaced by one of the three others."""
    k = len(codes)
    return codes ^ (rng.integers(1, 4, k, dtype=np.uint64) << (np.uint64(2) * rng.integers(0, bc_len, k, dtype=np.uint64)))


def with_junk(rng, bc, bc_len):
    """Random bits above 2*bc_len on half of the barcodes (none at 32 bases, where there is no room above)."""
    if bc_len >= 32:
        return bc
    j = rng.integers(0, 1 << 62, size=len(bc), dtype=np.uint64) << np.uint64(2 * bc_len)
    return np.where(rng.random(len(bc)) < 0.5, bc | j, bc)


# kind -> (slots of the table, home slots of the keys, keys): a cluster that runs from the last slots into slot 0; the
# longest chain a 1024-slot table allows (load exactly 1/2); the same over two home slots of a 2048-slot table
CRAFTED_TABLES = {"wrap300": (1024, (1020, 1021, 1022, 1023), 300),
                  "chain512": (1024, (1023,), 512),
                  "chain1024": (2048, (2046, 2047), 1024)}
WALKER_HOMES = 32   # codes that are not in the whitelist but have one of the first slots of its cluster as home slot


def crafted_table_case(bc_len, kind, tripled, n=100_003):
    """-> (whitelist, keys, walkers, barcodes[n]).  `whitelist` is `keys`, or every key three times and shuffled (the table
    then has four times the slots, table_model() says where the cluster lies).  Barcodes: a quarter each of the keys (every
    one of them where n allows), one substitution of each at a random base, `walkers` (their lookup walks the chain to the
    free slot behind it) and uniform random codes, shuffled; junk bits on half of them below 32 bases."""
    rng = np.random.default_rng([0x1B00400, bc_len, sorted(CRAFTED_TABLES).index(kind), int(tripled)])
    slots, homes, w = CRAFTED_TABLES[kind]
    keys = craft_keys(rng, bc_len, slots, homes, w)
    wl = rng.permutation(np.repeat(keys, 3)) if tripled else keys
    real_slots, _, table = table_model(wl, bc_len)
    start, _ = clusters(table)[0]
    walkers = craft_keys(rng, bc_len, real_slots, [(start + k) % real_slots for k in range(WALKER_HOMES)], 256, exclude=keys)
    q = n // 4
    bc = np.concatenate([np.resize(rng.permutation(keys), q), substitute(rng, np.resize(rng.permutation(keys), q), bc_len),
                         np.resize(walkers, q), random_codes(rng, bc_len, n - 3 * q)])
    return wl, keys, walkers, with_junk(rng, rng.permutation(bc), bc_len)


def neighbour(code, j):
    """Neighbour number j of a code as the device counts them: base j // 3 replaced, substitution j % 3 + 1."""
    return int(code) ^ ((j % 3 + 1) << (2 * (j // 3)))


def ballot_specs(bc_len):
    """The neighbour numbers to plant around one centre each: the wave search tests neighbours 0..63 in its first ballot
    (bases 0..20 and the first substitution of base 21) and 64..3*bc_len-1 in its second.  Pairs: both in the first; one
    in each; both in the second (two bases, and one base with two substitutions); base 21 on either side of the seam.
    Singles: the first and last neighbour and those around the seam."""
    nn, last = 3 * bc_len, bc_len - 1
    pairs = [(3 * 3, 3 * 17 + 1), (3 * 5 + 2, 3 * 22), (3 * 22 + 1, 3 * last + 2), (3 * last, 3 * last + 1), (63, 64), (63, 65), (64, 65),
             (0, nn - 1)]
    singles = [0, 62, 63, 64, 65, nn - 1]
    out = []
    for spec in [(j,) for j in singles] + pairs:
        if max(spec) < nn and len(set(spec)) == len(spec) and spec not in out:
            out.append(spec)
    return out


def ballot_case(bc_len, with_ones=True):
    """-> (whitelist, barcodes, expected class, expected low bits after correction, specs).  One random centre per
    ballot_specs() entry with exactly those neighbours in the whitelist (class 1 for one, 2 for two), a centre that is
    itself an entry (0) and one with nothing near (3).  At 32 bases also centres next to the all-ones key: four whose only
    whitelisted neighbour it is (as neighbour 0, 63, 64 and 95) and two that have a second one (in the other ballot; in the
    same).  with_ones=False leaves all ones out of the whitelist and keeps the barcodes: those become 3 and 1."""
    rng = np.random.default_rng([0x1B00500, bc_len])
    specs = ballot_specs(bc_len)
    centres = [int(c) for c in random_codes(rng, bc_len, len(specs) + 2)]
    wl, bc, cls, low = [], [], [], []
    for c, spec in zip(centres, specs):
        near = [neighbour(c, j) for j in spec]
        wl += near
        bc.append(c); cls.append(CORRECTED if len(near) == 1 else AMBIGUOUS); low.append(near[0] if len(near) == 1 else c)
    wl.append(centres[-2]); bc.append(centres[-2]); cls.append(EXACT); low.append(centres[-2])
    bc.append(centres[-1]); cls.append(UNMATCHED); low.append(centres[-1])
    if bc_len == 32:
        specs = specs + [("ones", j) for j in (0, 63, 64, 95)] + [("ones", 3 * 5 + 1, 3 * 30), ("ones", 3 * 25 + 2, 3 * 28)]
        for spec in specs[-6:]:
            c = neighbour(FREE, spec[1])                      # neighbour spec[1] of c is all ones again
            second = [neighbour(c, j) for j in spec[2:]]
            wl += second
            near = second + ([FREE] if with_ones else [])
            bc.append(c); cls.append((UNMATCHED, CORRECTED, AMBIGUOUS)[len(near)]); low.append(near[0] if len(near) == 1 else c)
        if with_ones:
            wl.append(FREE)
    as_u64 = lambda v: np.array(v, dtype=np.uint64)
    return as_u64(wl), as_u64(bc), np.array(cls, np.uint8), as_u64(low), specs


def miss_case(bc_len=16, w=1000, planted=64):
    """-> (whitelist, {class: barcodes of that class}) for classes 1, 2, 3, none of them exact: w random codes, `planted`
    of them with a partner two substitutions away (the midpoints are ambiguous); the pools are sorted out by classify()."""
    rng = np.random.default_rng([0x1B00600, bc_len, w])
    wl = np.unique(random_codes(rng, bc_len, w))
    a = wl[:planted]
    i = rng.integers(0, bc_len - 1, planted, dtype=np.uint64)
    mid = a ^ (rng.integers(1, 4, planted, dtype=np.uint64) << (np.uint64(2) * i))
    partner = mid ^ (rng.integers(1, 4, planted, dtype=np.uint64) << (np.uint64(2) * (i + np.uint64(1))))
    wl = rng.permutation(np.unique(np.concatenate([wl, partner])))
    cand = np.concatenate([mid, substitute(rng, np.resize(wl, 4 * w), bc_len), random_codes(rng, bc_len, 4 * w)])
    cls, _ = classify(cand, wl, bc_len, 1)
    return wl, {c: np.unique(cand[cls == c]) for c in (CORRECTED, AMBIGUOUS, UNMATCHED)}
