"""Numpy / Python-int restatement of the device building blocks behind grx_device_scan, grx_device_key_sort,
grx_device_transpose, grx_wave_ops and grx_bisect_queue: what each must produce, stated without tiles, waves or DPP controls.

  exclusive_scan(values)                  exclusive prefix in uint64 and the total as a Python int
  fits(prefix, dtype)                     where a 64-bit prefix is representable in a 32-bit output type
  sort_mask(key_bits), stable_sort(...)   the sort's contract: ascending and stable on the low 8 * ceil(key_bits / 8) bits
  transpose(ro, ci, vals)                 inverse row offsets and every inverse row as a sorted multiset of (source, value)
  canonical_rows(ro, ci, vals)            ... the same form of a transpose that was computed elsewhere
  wave_inclusive / wave_segmented / wave_sum / rank_in_mask / dpp_move / block_scan
                                          per 64-lane wave (elements past the end count as zeros, as the entry point pads)
  bisect(...)                             the near/far split, as a loop over the queue
Integer arithmetic is done in the value's own numpy type, which wraps as the device's does.  tests/test_blocks_cpu.py checks
every vectorised function here against a naive loop.
"""
import numpy as np

import _advance_checker as ack

WAVE = 64
UFUNC = {"plus": np.add, "multiplies": np.multiply, "maximum": np.maximum, "minimum": np.minimum, "bit_or": np.bitwise_or,
         "bit_and": np.bitwise_and, "bit_xor": np.bitwise_xor}
identity = ack.identity


# ---------------------------------------------------------------- scan ---------------------------------------------------

def exclusive_scan(values):
    v = np.asarray(values, dtype=np.uint64)            # up to 2^23 terms below 2^32: far inside 64 bits
    inc = np.cumsum(v, dtype=np.uint64)
    prefix = np.zeros(v.size, dtype=np.uint64)
    prefix[1:] = inc[:-1]
    return prefix, (int(inc[-1]) if v.size else 0)


def fits(prefix, dtype):
    return np.asarray(prefix, dtype=np.uint64) <= np.uint64(np.iinfo(dtype).max)


# ---------------------------------------------------------------- sort ---------------------------------------------------

def sorted_bits(key_bits):
    """the sort runs whole 8-bit passes: the low 8 * ceil(key_bits / 8) bits are ordered"""
    return 8 * ((int(key_bits) + 7) // 8)


def sort_mask(key_bits):
    return np.uint64((1 << sorted_bits(key_bits)) - 1)


def stable_sort(keys, key_bits):
    keys = np.asarray(keys, dtype=np.uint64)
    return keys[np.argsort(keys & sort_mask(key_bits), kind="stable")]


# ---------------------------------------------------------------- transpose ----------------------------------------------

def canonical_rows(row_offsets, col_indices, values=None):
    """(row of every entry, column, value) with the entries of each row sorted by (column, value): a row as a multiset"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    vals = np.zeros(ci.size, dtype=np.int64) if values is None else np.asarray(values, dtype=np.int64)
    row = np.repeat(np.arange(ro.size - 1, dtype=np.int64), np.diff(ro))
    order = np.lexsort((vals, ci, row))
    return row[order], ci[order], vals[order]


def transpose(row_offsets, col_indices, values=None):
    """inverse row offsets (int64) and the canonical rows of the inverse graph: every edge (v, u, value) becomes (u, v, value),
    duplicates and self loops included"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    nodes = ro.size - 1
    vals = np.zeros(ci.size, dtype=np.int64) if values is None else np.asarray(values, dtype=np.int64)
    src = np.repeat(np.arange(nodes, dtype=np.int64), np.diff(ro))
    inv_ro = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=nodes))]).astype(np.int64)
    order = np.lexsort((vals, src, ci))
    return inv_ro, (ci[order], src[order], vals[order])


# ---------------------------------------------------------------- wave blocks --------------------------------------------

def _waves(a, fill=0):
    a = np.asarray(a)
    padded = np.full(-(-max(a.size, 1) // WAVE) * WAVE, fill, dtype=a.dtype)
    padded[:a.size] = a
    return padded.reshape(-1, WAVE)


def wave_inclusive(values, op="plus"):
    values = np.asarray(values)
    with np.errstate(over="ignore"):
        return UFUNC[op].accumulate(_waves(values), axis=1, dtype=values.dtype).reshape(-1)[:values.size]


def wave_segmented(values, heads, op):
    """lane i: op over the lanes of its segment up to i; a segment starts at every head and, implicitly, at lane 0"""
    values = np.asarray(values)
    v = _waves(values)
    h = _waves(np.zeros(values.size, dtype=bool) if heads is None else np.asarray(heads) != 0, False)
    out = v.copy()
    with np.errstate(over="ignore"):
        for lane in range(1, WAVE):                    # a loop over the lanes, every wave at once
            out[:, lane] = np.where(h[:, lane], v[:, lane], UFUNC[op](out[:, lane - 1], v[:, lane]))
    return out.reshape(-1)[:values.size]


def wave_sum(values):
    values = np.asarray(values)
    with np.errstate(over="ignore"):
        s = _waves(values).sum(axis=1, dtype=values.dtype)
    return np.repeat(s, WAVE)[:values.size]


def rank_in_mask(masks):
    """element i (lane i % 64): set bits of ITS mask strictly below its lane"""
    m = np.asarray(masks, dtype=np.uint64)
    lane = np.arange(m.size, dtype=np.uint64) % np.uint64(WAVE)
    below = m & ((np.uint64(1) << lane) - np.uint64(1))
    count = np.zeros(m.size, dtype=np.uint32)
    for b in range(WAVE):
        count += ((below >> np.uint64(b)) & np.uint64(1)).astype(np.uint32)
    return count


# step -> (what lane i reads, which 16-lane rows are written): gfx9 DPP row_shr:1/2/4/8 (lane i - k of the same row, full row mask),
# row_bcast:15 (lane 15 of the row before) under row mask 0xA, row_bcast:31 (lane 31) under row mask 0xC
DPP_STEPS = 6


def dpp_source(step):
    """per lane: the lane it receives from, or -1 when it keeps the identity"""
    lane = np.arange(WAVE)
    row, col = lane // 16, lane % 16
    if step < 4:
        k = 1 << step
        return np.where(col >= k, lane - k, -1)
    if step == 4:
        return np.where((row == 1) | (row == 3), row * 16 - 1, -1)
    return np.where(row >= 2, 31, -1)


def dpp_move(values, step, identity_value):
    values = np.asarray(values)
    v = _waves(values)
    src = dpp_source(step)
    out = np.where(src >= 0, v[:, np.maximum(src, 0)], values.dtype.type(identity_value))
    return out.astype(values.dtype).reshape(-1)[:values.size]


def block_scan(values, threads):
    """per workgroup of `threads` elements: (exclusive sum, total per thread) of the elements, then of the same elements in
    mirrored order (thread t takes element threads - 1 - t; elements past the end are zeros)"""
    values = np.asarray(values)
    padded = np.zeros(-(-max(values.size, 1) // threads) * threads, dtype=values.dtype)
    padded[:values.size] = values
    blocks = padded.reshape(-1, threads)
    res = []
    with np.errstate(over="ignore"):
        for b in (blocks, blocks[:, ::-1]):
            inc = np.cumsum(b, axis=1, dtype=values.dtype)
            res.append((inc - b).reshape(-1)[:values.size])
            res.append(np.repeat(inc[:, -1], threads)[:values.size])
    return tuple(res)


# ---------------------------------------------------------------- near/far split -----------------------------------------

def bucket_of(dist, delta):
    """PQFunctor::ComputePriorityScore: the distance itself for delta 0, else uint32(float32(dist) / float32(delta))"""
    if float(delta) == 0.0:
        return int(dist)
    return int(np.uint32(np.float32(dist) / np.float32(delta)))


def bisect(queue, count, dist, visit_lookup, tag, delta, level, parked=None):
    """walk the first `count` entries of the queue: skip -1, skip entries whose parked distance is not the current one, keep the
    first arrival of each vertex (an entry whose vertex already carries `tag` is a duplicate), near iff bucket <= level.
    Returns (near vertices, far (vertex, distance) pairs, smallest far bucket or UINT_MAX, visit_lookup afterwards), in
    queue order."""
    lookup = np.array(visit_lookup, dtype=np.int32)
    near, far, far_min = [], [], 0xFFFFFFFF
    for i in range(int(count)):
        v = int(queue[i])
        if v < 0:
            continue
        d = int(dist[v])
        if parked is not None and int(parked[i]) != d:
            continue
        if lookup[v] == tag:
            continue
        lookup[v] = tag
        b = bucket_of(d, delta)
        if b <= level:
            near.append(v)
        else:
            far.append((v, d))
            far_min = min(far_min, b)
    return near, far, far_min, lookup
