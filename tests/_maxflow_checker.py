"""CPU checker for the maximum flow and the minimum cuts (grx_maxflow_*).

The CSR is a directed multigraph with int32 capacities (None: 1 each): self-loops are ignored, parallel arcs add up.  The M canonical
pairs are the distinct {a < b} with an arc either way (capacity 0 included), sorted by (a, b), with cap_ab and cap_ba summed in 64
bits.  Three independent forms that must agree on everything that has one value (the flow value and the two residual reaches):
  by_dinic      Dinic in plain Python over the canonical pairs
  by_scipy      scipy.sparse.csgraph.maximum_flow on the merged int32 matrix ("dinic" or "edmonds_karp"); residual = capacity - flow
                as a sparse difference (the flow matrix is antisymmetric, so the difference carries the reverse residuals)
  by_networkx   networkx.maximum_flow_value and networkx.minimum_cut, whose sink side is the set that can reach sink: side 2
side[v] is 0 (reachable from src in the residual graph of a maximum flow), 2 (sink reachable from v) or 1; cut[p] has bit 0 for
positive capacity from a side-0 end to an end that is not side 0 and bit 1 for positive capacity from an end that is not side 2 to a
side-2 end.  The per-pair flow is not unique: validate_flow / expected_arc_flow check it by its rules."""
from collections import deque

import numpy as np

INT_MAX = 2 ** 31 - 1


class Malformed(ValueError):
    """a negative capacity, or a pair whose two capacities do not fit one int32 together (init's -2)"""


def arcs_of(nodes, row_offsets, col_indices, capacities=None):
    """(u, v, cap) per CSR entry as int64"""
    ro = np.asarray(row_offsets, np.int64)
    v = np.asarray(col_indices, np.int64)
    u = np.repeat(np.arange(nodes, dtype=np.int64), np.diff(ro)) if nodes else np.zeros(0, np.int64)
    cap = np.ones(v.shape[0], np.int64) if capacities is None else np.asarray(capacities, np.int64)
    return u, v, cap


def pairs_of(nodes, row_offsets, col_indices, capacities=None):
    """(a, b, cap_ab, cap_ba) as int32; Malformed by init's two rules"""
    u, v, cap = arcs_of(nodes, row_offsets, col_indices, capacities)
    if cap.shape[0] and int(cap.min()) < 0:
        raise Malformed("a negative capacity")
    keep = u != v
    u, v, cap = u[keep], v[keep], cap[keep]
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    keys, inverse = np.unique(lo * max(nodes, 1) + hi, return_inverse=True)
    inverse = inverse.reshape(-1)
    cab, cba = np.zeros(keys.shape[0], np.int64), np.zeros(keys.shape[0], np.int64)
    np.add.at(cab, inverse[u < v], cap[u < v])
    np.add.at(cba, inverse[u > v], cap[u > v])
    if keys.shape[0] and int((cab + cba).max()) > INT_MAX:
        raise Malformed("a pair over 2^31 - 1")
    return (keys // max(nodes, 1)).astype(np.int32), (keys % max(nodes, 1)).astype(np.int32), cab.astype(np.int32), cba.astype(np.int32)


def _rows(nodes, a, b):
    """start, arc ids: row v lists the arcs out of v, arc 2p = a -> b and arc 2p + 1 = b -> a of pair p"""
    M = a.shape[0]
    tail = np.empty(2 * M, np.int64)
    tail[0::2], tail[1::2] = a, b
    order = np.argsort(tail, kind="stable")
    start = np.zeros(nodes + 1, np.int64)
    np.cumsum(np.bincount(tail, minlength=nodes), out=start[1:])
    return start, order


def dinic(nodes, a, b, cab, cba, s, t):
    """(value, flow per pair as int64) by Dinic's blocking flows, iterative"""
    M = a.shape[0]
    head = np.empty(2 * M, np.int64)
    head[0::2], head[1::2] = b, a
    res = np.empty(2 * M, np.int64)
    res[0::2], res[1::2] = cab, cba
    start, order = _rows(nodes, a, b)
    head, res, start, order = head.tolist(), res.tolist(), start.tolist(), order.tolist()
    value = 0
    while True:
        level = [-1] * nodes
        level[s] = 0
        queue = deque([s])
        while queue:
            x = queue.popleft()
            for k in range(start[x], start[x + 1]):
                e = order[k]
                y = head[e]
                if res[e] > 0 and level[y] < 0:
                    level[y] = level[x] + 1
                    queue.append(y)
        if level[t] < 0:
            break
        at = start[:nodes]
        path = []  # the arcs from s to the current vertex
        x = s
        while True:
            if x == t:
                push = min(res[e] for e in path)
                for e in path:
                    res[e] -= push
                    res[e ^ 1] += push
                value += push
                # back to the tail of the first arc that is now saturated
                for i, e in enumerate(path):
                    if res[e] == 0:
                        del path[i:]
                        break
                x = head[path[-1]] if path else s
                continue
            advanced = False
            while at[x] < start[x + 1]:
                e = order[at[x]]
                y = head[e]
                if res[e] > 0 and level[y] == level[x] + 1:
                    path.append(e)
                    x = y
                    advanced = True
                    break
                at[x] += 1
            if advanced:
                continue
            if x == s:
                break
            level[x] = -1  # a dead end of this phase
            e = path.pop()
            x = head[e ^ 1]
    flow = np.asarray(cab, np.int64) - np.asarray(res[0::2], np.int64)
    return value, flow


def _reach(nodes, start, order, head, ok, root, backward):
    seen = np.zeros(nodes, bool)
    seen[root] = True
    queue = deque([root])
    while queue:
        x = queue.popleft()
        for k in range(start[x], start[x + 1]):
            e = order[k]
            if ok[e ^ 1 if backward else e] and not seen[head[e]]:
                seen[head[e]] = True
                queue.append(head[e])
    return seen


def sides_from_flow(nodes, a, b, cab, cba, flow, s, t):
    """side[] from the residual graph of the per-pair flow"""
    M = a.shape[0]
    head = np.empty(2 * M, np.int64)
    head[0::2], head[1::2] = b, a
    res = np.empty(2 * M, np.int64)
    res[0::2], res[1::2] = np.asarray(cab, np.int64) - flow, np.asarray(cba, np.int64) + flow
    start, order = _rows(nodes, a, b)
    ok = (res > 0).tolist()
    start, order, head = start.tolist(), order.tolist(), head.tolist()
    fwd = _reach(nodes, start, order, head, ok, s, False)
    bwd = _reach(nodes, start, order, head, ok, t, True)
    return np.where(fwd, 0, np.where(bwd, 2, 1)).astype(np.uint8)


def cut_of(a, b, cab, cba, side):
    sa, sb = side[a], side[b]
    bit0 = ((sa == 0) & (sb != 0) & (cab > 0)) | ((sb == 0) & (sa != 0) & (cba > 0))
    bit1 = ((sa != 2) & (sb == 2) & (cab > 0)) | ((sb != 2) & (sa == 2) & (cba > 0))
    return (bit0.astype(np.uint8) | (bit1.astype(np.uint8) << 1)).astype(np.uint8)


def cut_capacities(a, b, cab, cba, side):
    """the capacity under cut bit 0 and under cut bit 1"""
    sa, sb = side[a], side[b]
    c, d = np.asarray(cab, np.int64), np.asarray(cba, np.int64)
    return (int(c[(sa == 0) & (sb != 0)].sum() + d[(sb == 0) & (sa != 0)].sum()),
            int(c[(sa != 2) & (sb == 2)].sum() + d[(sb != 2) & (sa == 2)].sum()))


def _result(a, b, cab, cba, value, side):
    cut = cut_of(a, b, cab, cba, side)
    summary = {"value": int(value), "side0": int((side == 0).sum()), "side1": int((side == 1).sum()), "side2": int((side == 2).sum()),
               "cut0": int((cut & 1).sum()), "cut1": int((cut >> 1).sum())}
    return {"value": int(value), "side": side, "cut": cut, "summary": summary}


def by_dinic(nodes, a, b, cab, cba, s, t):
    value, flow = dinic(nodes, a, b, cab, cba, s, t)
    out = _result(a, b, cab, cba, value, sides_from_flow(nodes, a, b, cab, cba, flow, s, t))
    out["flow"] = flow
    return out


def by_scipy(nodes, a, b, cab, cba, s, t, method="dinic"):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order, maximum_flow
    rows, cols = np.concatenate([a, b]).astype(np.int32), np.concatenate([b, a]).astype(np.int32)
    capacity = sp.csr_matrix((np.concatenate([cab, cba]).astype(np.int32), (rows, cols)), shape=(nodes, nodes))
    got = maximum_flow(capacity, s, t, method=method)
    residual = (capacity - got.flow).tocsr()
    residual.data = (residual.data > 0).astype(np.int32)
    residual.eliminate_zeros()
    side = np.full(nodes, 1, np.uint8)
    side[breadth_first_order(residual.T.tocsr(), t, directed=True, return_predecessors=False)] = 2
    side[breadth_first_order(residual, s, directed=True, return_predecessors=False)] = 0
    return _result(a, b, cab, cba, got.flow_value, side)


def by_networkx(nodes, a, b, cab, cba, s, t):
    import networkx as nx
    g = nx.DiGraph()
    g.add_nodes_from(range(nodes))
    for x, y, c, d in zip(a.tolist(), b.tolist(), cab.tolist(), cba.tolist()):
        g.add_edge(x, y, capacity=c)
        g.add_edge(y, x, capacity=d)
    value = nx.maximum_flow_value(g, s, t)
    cut_value, (_, can_reach_sink) = nx.minimum_cut(g, s, t)
    side2 = np.zeros(nodes, bool)
    side2[list(can_reach_sink)] = True
    return {"value": int(value), "cut_value": int(cut_value), "side2": side2}


def solve(nodes, row_offsets, col_indices, capacities, s, t, form="scipy"):
    """(a, b, cap_ab, cap_ba, ref): ref has "value", "side", "cut" and "summary" """
    a, b, cab, cba = pairs_of(nodes, row_offsets, col_indices, capacities)
    ref = by_scipy(nodes, a, b, cab, cba, s, t) if form == "scipy" else by_dinic(nodes, a, b, cab, cba, s, t)
    return a, b, cab, cba, ref


def same(x, y):
    return x["value"] == y["value"] and np.array_equal(x["side"], y["side"]) and np.array_equal(x["cut"], y["cut"]) and x["summary"] == y["summary"]


def forms_disagree(nodes, row_offsets, col_indices, capacities, s, t, edmonds_karp=True, slow_forms=True):
    """the ways in which the forms differ on this case ([]: they agree); slow_forms: plain-Python Dinic and networkx as well"""
    a, b, cab, cba = pairs_of(nodes, row_offsets, col_indices, capacities)
    ref = by_scipy(nodes, a, b, cab, cba, s, t)
    bad = []
    if edmonds_karp and 2 * a.shape[0] <= 1 << 15 and not same(ref, by_scipy(nodes, a, b, cab, cba, s, t, "edmonds_karp")):
        bad.append("scipy edmonds_karp")
    if slow_forms:
        mine = by_dinic(nodes, a, b, cab, cba, s, t)
        if not same(ref, mine):
            bad.append("plain dinic")
        bad += ["dinic flow: " + x for x in validate_flow(nodes, a, b, cab, cba, s, t, ref["value"], mine["flow"])]
        x = by_networkx(nodes, a, b, cab, cba, s, t)
        if x["value"] != ref["value"] or x["cut_value"] != ref["value"] or not np.array_equal(x["side2"], ref["side"] == 2):
            bad.append("networkx")
    caps = cut_capacities(a, b, cab, cba, ref["side"])
    if caps != (ref["value"], ref["value"]):
        bad.append("cut capacities %r" % (caps,))
    return bad


def validate_flow(nodes, a, b, cab, cba, s, t, value, flow):
    """the rules of flow[]: bounds, conservation, the net outflow of src and the net inflow of sink"""
    flow = np.asarray(flow, np.int64)
    bad = []
    if flow.shape[0] != a.shape[0]:
        return ["flow has %d entries for %d pairs" % (flow.shape[0], a.shape[0])]
    if np.any(flow > cab) or np.any(flow < -np.asarray(cba, np.int64)):
        bad.append("flow outside [-cap_ba, cap_ab]")
    net = np.zeros(nodes, np.int64)
    np.add.at(net, a, flow)
    np.subtract.at(net, b, flow)
    inner = np.ones(nodes, bool)
    inner[[s, t]] = False
    if np.any(net[inner] != 0):
        bad.append("flow not conserved at %d vertices" % int((net[inner] != 0).sum()))
    if int(net[s]) != value or int(net[t]) != -value:
        bad.append("src sends %d, sink takes %d, value %d" % (int(net[s]), -int(net[t]), value))
    return bad


def expected_arc_flow(nodes, row_offsets, col_indices, capacities, a, b, flow):
    """arc_flow[] as the table defines it from flow[] and the input"""
    u, v, cap = arcs_of(nodes, row_offsets, col_indices, capacities)
    out = np.zeros(u.shape[0], np.int64)
    idx = np.flatnonzero(u != v)
    if idx.shape[0] == 0:
        return out.astype(np.int32)
    uu, vv, cc = u[idx], v[idx], cap[idx]
    pair = np.searchsorted(a.astype(np.int64) * nodes + b, np.minimum(uu, vv) * nodes + np.maximum(uu, vv))
    f = np.asarray(flow, np.int64)[pair]
    direction = np.where(uu < vv, np.maximum(f, 0), np.maximum(-f, 0))  # the pair's net flow u -> v
    order = np.argsort(uu * nodes + vv, kind="stable")  # groups of one direction of one pair, in CSR order
    key = (uu * nodes + vv)[order]
    c = cc[order]
    before = np.cumsum(c) - c
    first = np.r_[True, key[1:] != key[:-1]]
    before -= np.maximum.accumulate(np.where(first, before, 0))
    got = np.clip(direction[order] - before, 0, c)
    out[idx[order]] = got
    return out.astype(np.int32)


def mismatches(problem, nodes, row_offsets, col_indices, capacities, s, t, a, b, cab, cba, ref, arc_flow=True):
    """compares what the handle holds after an Enact with the checker's `ref`: [] or the list of differences"""
    bad = []
    pa, pb, pab, pba = problem.pairs()
    for name, x, y in (("a", pa, a), ("b", pb, b), ("cap_ab", pab, cab), ("cap_ba", pba, cba)):
        if x.dtype != np.int32 or not np.array_equal(x, y):
            bad.append("pairs: " + name)
    if bad:
        return bad
    got = problem.extract()
    if got["value"] != ref["value"]:
        bad.append("value %d, expected %d" % (got["value"], ref["value"]))
    if got["side"].dtype != np.uint8 or not np.array_equal(got["side"], ref["side"]):
        bad.append("side differs at %d vertices" % int((got["side"] != ref["side"]).sum()))
    if got["cut"].dtype != np.uint8 or not np.array_equal(got["cut"], ref["cut"]):
        bad.append("cut differs at %d pairs" % int((got["cut"] != ref["cut"]).sum()))
    if problem.summary() != ref["summary"]:
        bad.append("summary %r, expected %r" % (problem.summary(), ref["summary"]))
    if got["flow"].dtype != np.int32:
        bad.append("flow dtype")
    bad += validate_flow(nodes, a, b, cab, cba, s, t, got["value"], got["flow"])
    caps = cut_capacities(a, b, cab, cba, got["side"])
    if caps != (got["value"], got["value"]):
        bad.append("cut capacities %r, value %d" % (caps, got["value"]))
    if arc_flow:
        arcs = problem.arc_flow()
        if arcs.dtype != np.int32 or not np.array_equal(arcs, expected_arc_flow(nodes, row_offsets, col_indices, capacities, a, b, got["flow"])):
            bad.append("arc_flow is not the flow handed out in CSR order")
    return bad


def csr_from_arcs(nodes, rows, cols, caps=None, shuffle=None):
    """(ro, ci, cap) int32 from arcs; shuffle: a Generator that puts every row in a random order"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    caps = None if caps is None else np.asarray(caps, np.int64)
    if shuffle is not None and rows.shape[0]:
        perm = shuffle.permutation(rows.shape[0])
        rows, cols, caps = rows[perm], cols[perm], None if caps is None else caps[perm]
    order = np.argsort(rows, kind="stable")
    ro = np.zeros(nodes + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=nodes), out=ro[1:])
    return ro, cols[order].astype(np.int32), None if caps is None else caps[order].astype(np.int32)


def rmat_case(scale):
    """the pinned recipe: (nodes, ro, ci, cap, src, sink)"""
    from oracle import gr_oracle as o
    g = o.rmat_seeded(scale, 8 << scale, undirected=False)
    cap = np.random.default_rng(scale).integers(0, 17, size=g.edges).astype(np.int32)
    src = int(np.argmax(np.diff(g.row_offsets)))
    indegree = np.bincount(g.col_indices, minlength=g.nodes)
    sink = next(int(v) for v in np.argsort(-indegree, kind="stable") if int(v) != src)
    return g.nodes, np.asarray(g.row_offsets, np.int32), np.asarray(g.col_indices, np.int32), cap, src, sink
