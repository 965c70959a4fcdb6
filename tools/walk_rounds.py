#!/usr/bin/env python3
"""Census of the walk stage of a dense bottom-up sweep, on the CPU (DESIGN §3.3 m cites it; nothing here touches a GPU).

For one search of the benchmark's seeded R-MAT graph and one of its levels, taken as a dense bottom-up sweep over every
unvisited vertex with edges, it counts

  open            unvisited vertices with edges when the sweep starts
  walkers         open vertices whose two adjacency heads both miss the frontier (they go on to their CSR row)
  length 2        walkers whose row IS its two heads (nothing to walk: BuildHeadsKernel flags them)
  rounds now      WalkRow rounds per 512-vertex step of the step-by-step loop: the largest number of walkers any lane holds
  rounds packed   the same walkers 64 to a round (the per-wave queue): walkers / 64 / steps that hold an open vertex, a quotient
                  and not a count of started rounds; with and without the length-2 rows

The model: heads are the two largest-degree entries among the first 512 of a row (ties to the larger id, as the kernel's
key); a step is 512 consecutive vertices WITH edges, which is what the relabelled numbering gives a wave (hubs first changes
which vertices share a step, not how many walkers a step holds on average); lane = position in the step mod 64.  Rows are
deduplicated in this graph, so "second largest" needs no rule for repeated entries.

  python tools/walk_rounds.py --scale 24            # the two rows of the table (several GB of host memory, minutes)
  python tools/walk_rounds.py --scale 18 --source max --level 2
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gr_oracle as o  # noqa: E402

HEAD_SCAN = 512
STEP = 512
MASK = np.uint64(0xFFFFFFFF)


def splitmix64(x):
    """as gunrockinst_amd.devgraph draws the benchmark's sources: the output is also the next state"""
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def heads(ro, ci, deg, chunk=1 << 20):
    """(h1, h2) per vertex, -1 where the row has no such entry"""
    n = deg.size
    h1 = np.full(n, -1, np.int64)
    h2 = np.full(n, -1, np.int64)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        lo, hi = int(ro[a]), int(ro[b])
        if hi == lo:
            continue
        cols = ci[lo:hi].astype(np.int64)
        rows = np.repeat(np.arange(a, b), deg[a:b])
        pos = np.arange(lo, hi) - ro[rows]
        key = ((deg[cols] + 1).astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
        key[pos >= HEAD_SCAN] = 0
        live = np.nonzero(deg[a:b] > 0)[0]
        starts = (ro[a:b][live] - lo).astype(np.int64)
        k1 = np.maximum.reduceat(key, starts)
        first = np.zeros(b - a, np.uint64)
        first[live] = k1
        key[key == first[rows - a]] = 0
        k2 = np.maximum.reduceat(key, starts)
        h1[a + live] = np.where(k1 > 0, (k1 & MASK).astype(np.int64), -1)
        h2[a + live] = np.where(k2 > 0, (k2 & MASK).astype(np.int64), -1)
    return h1, h2


def levels_until(ro, ci, deg, src, level):
    """visited and frontier masks when the sweep that finds `level` starts (frontier = the vertices of level - 1)"""
    n = deg.size
    visited = np.zeros(n, bool)
    frontier = np.zeros(n, bool)
    visited[src] = frontier[src] = True
    for _ in range(level - 1):
        f = np.nonzero(frontier)[0]
        idx = np.concatenate([np.arange(ro[v], ro[v + 1]) for v in f]) if f.size < 64 else \
            np.repeat(ro[f], deg[f]) + (np.arange(int(deg[f].sum())) - np.repeat(np.cumsum(deg[f]) - deg[f], deg[f]))
        nxt = np.zeros(n, bool)
        nxt[ci[idx]] = True
        nxt &= ~visited
        visited |= nxt
        frontier = nxt
    return visited, frontier


def census(ro, ci, deg, h1, h2, src, level):
    visited, frontier = levels_until(ro, ci, deg, src, level)
    with_edges = np.nonzero(deg > 0)[0]              # the step numbering: rank among the vertices with edges
    open_ = ~visited[with_edges]
    a, b = h1[with_edges], h2[with_edges]
    miss = open_ & (a >= 0) & (b >= 0) & ~frontier[np.maximum(a, 0)] & ~frontier[np.maximum(b, 0)]
    walkers = np.nonzero(miss)[0]                    # ranks
    len2 = deg[with_edges[walkers]] == 2
    steps = (with_edges.size + STEP - 1) // STEP
    live_steps = np.unique(np.nonzero(open_)[0] // STEP).size
    per_lane = np.zeros((steps, 64), np.int64)
    np.add.at(per_lane, (walkers // STEP, walkers % 64), 1)
    rounds_now = per_lane.max(axis=1).sum()
    f = np.nonzero(frontier)[0]
    return {"source": int(src), "source_degree": int(deg[src]), "level": level, "frontier_vertices": int(f.size),
            "frontier_edges": int(deg[f].sum()), "open": int(open_.sum()), "walkers": int(walkers.size),
            "walkers_length_2": int(len2.sum()), "steps_with_open": int(live_steps),
            "rounds_per_step_now": round(float(rounds_now) / live_steps, 2),
            "rounds_per_step_packed": round(walkers.size / 64.0 / live_steps, 2),
            "rounds_per_step_packed_without_length_2": round((walkers.size - int(len2.sum())) / 64.0 / live_steps, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edge-factor", type=int, default=8)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x6772)
    ap.add_argument("--source", default=None, help="'max', a vertex id, or 'deg:D' = the first of the 64 seeded sources of degree D (the result names its id)")
    ap.add_argument("--level", type=int, default=None)
    args = ap.parse_args()
    g = o.rmat_seeded(args.scale, args.edge_factor << args.scale, seed=args.seed)
    ro = g.row_offsets.astype(np.int64)
    ci = g.col_indices
    deg = np.diff(ro)
    h1, h2 = heads(ro, ci, deg)
    seeded, x = [], args.seed
    while len(seeded) < 64:
        x = splitmix64(x)
        if deg[x % g.nodes] > 0:
            seeded.append(int(x % g.nodes))

    def pick(spec):
        if spec == "max":
            return int(np.argmax(deg))
        if spec.startswith("deg:"):
            want = int(spec[4:])
            return next(s for s in seeded if deg[s] == want)
        return int(spec)

    jobs = [(args.source, args.level)] if args.source else [("deg:12", 3), ("max", 2)]
    for spec, level in jobs:
        print(census(ro, ci, deg, h1, h2, pick(spec), level or 2))


if __name__ == "__main__":
    main()
