"""ibu_partition_records in numpy: the statement the device is compared with, byte for byte.

part_of[c] is the part of class byte c (a value below n_parts, or NONE = 255: the record is dropped); the output is part 0, then
part 1, ..., each in input order; offsets[p] is the first record of part p and offsets[n_parts] the number of records kept."""
import numpy as np

NONE = 255


def identity(n_parts):
    """What part_of == NULL means: class c < n_parts is part c, every other class is dropped."""
    m = np.full(256, NONE, np.uint8)
    m[:n_parts] = np.arange(n_parts, dtype=np.uint8)
    return m


def check_map(part_of, n_parts):
    """The argument rules: n_parts in 1 .. 255, every entry below n_parts or NONE."""
    m = np.asarray(part_of)
    return 1 <= n_parts <= 255 and m.shape == (256,) and bool(((m < n_parts) | (m == NONE)).all())


def partition(recs, cls, part_of, n_parts):
    """-> (the kept records in output order, offsets u64[n_parts + 1], order: the input position of every output record)."""
    part_of = identity(n_parts) if part_of is None else np.asarray(part_of, np.uint8)
    assert check_map(part_of, n_parts)
    part = part_of[np.asarray(cls, np.uint8)]
    kept = part != NONE
    order = np.flatnonzero(kept)[np.argsort(part[kept], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(part[kept], minlength=n_parts))]).astype(np.uint64)
    return recs[order], offsets, order


def partition_loop(cls, part_of, n_parts):
    """The same with a plain loop (small inputs): -> (order, offsets)."""
    parts = [[] for _ in range(n_parts)]
    for i, c in enumerate(cls):
        p = int(part_of[int(c)]) if part_of is not None else (int(c) if int(c) < n_parts else NONE)
        if p != NONE:
            parts[p].append(i)
    offsets = [0]
    for p in parts:
        offsets.append(offsets[-1] + len(p))
    return [i for p in parts for i in p], offsets


def unit_of(n_parts):
    """Records per unit of the device's count and scatter passes (ibu_amd/csrc/partition_plan.hpp: partition_unit)."""
    unit = 2048
    while unit < 64 * n_parts:
        unit *= 2
    return unit
