#!/usr/bin/env python3
"""Census of what a hub slice of the frontier bitmap would answer, on the CPU (DESIGN §3.3 n cites it; nothing here touches a GPU).

For the benchmark's seeded R-MAT graph and a hub tier of the H vertices of largest degree (ties to the smaller id; the
relabelled copy takes "degree >= T" with the smallest T that leaves at most H vertices, which is the same set up to the ties at T),
it counts, over every vertex with edges,

  first head      the share whose first adjacency head is a hub
  second head     the share of those with a second head whose second head is a hub
  column entries  the share of all CSR entries that name a hub

Heads are taken as tools/walk_rounds.py takes them: the two largest-degree entries among the first 512 of a row.  A probe of a
hub id is one the dense bottom-up sweeps answer from LDS when hub_slice = relabel_hubs = H; H / 8 bytes of LDS hold the slice.

  python tools/hub_census.py --scale 24                      # H = 32768, 65536, 131072 (several GB of host memory, minutes)
  python tools/hub_census.py --scale 22 --hubs 65536
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import gr_oracle as o  # noqa: E402
from walk_rounds import heads  # noqa: E402


def census(ci, deg, h1, h2, hubs):
    order = np.argsort(-deg, kind="stable")          # largest degree first, ties to the smaller id
    is_hub = np.zeros(deg.size, bool)
    is_hub[order[:hubs]] = True
    is_hub &= deg > 0
    live = deg > 0
    a, b = h1[live], h2[live]
    second = b >= 0
    hub_entries = 0
    for lo in range(0, ci.size, 1 << 26):
        hub_entries += int(is_hub[ci[lo:lo + (1 << 26)]].sum())
    return {"hubs": int(is_hub.sum()), "lds_bytes": (hubs + 7) // 8, "vertices_with_edges": int(live.sum()),
            "first_head_is_hub": round(float(is_hub[a].mean()), 3),
            "second_head_is_hub": round(float(is_hub[b[second]].mean()), 3) if second.any() else None,
            "column_entries_that_are_hubs": round(hub_entries / max(1, ci.size), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edge-factor", type=int, default=8)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x6772)
    ap.add_argument("--hubs", type=int, action="append", default=None, help="hub tier size, repeatable (default 32768 65536 131072)")
    args = ap.parse_args()
    g = o.rmat_seeded(args.scale, args.edge_factor << args.scale, seed=args.seed)
    ro = g.row_offsets.astype(np.int64)
    deg = np.diff(ro)
    h1, h2 = heads(ro, g.col_indices, deg)
    for hubs in args.hubs or [32768, 65536, 131072]:
        row = census(g.col_indices, deg, h1, h2, hubs)
        row["scale"] = args.scale
        print(row)


if __name__ == "__main__":
    main()
