"""Maximum bipartite matching and the Dulmage-Mendelsohn decomposition in plain Python and numpy, written from the definitions.

A matrix is (shape, ro, ci): a CSR pattern of shape (rows, cols), duplicates and unsorted rows allowed.

  hopcroft_karp   a maximum matching: phases of a breadth-first layering from the unmatched rows and a depth-first search for a
                  maximal set of shortest disjoint augmenting paths
  parts           row_part / col_part from ANY maximum matching: HORIZONTAL = reached from an unmatched column by a path that
                  alternates (unmatched edge column -> row, matched edge row -> column), VERTICAL = the same from an unmatched
                  row, SQUARE = the rest
  cover           König: the rows outside the vertical part and the columns inside it
  blocks          the strongly connected components (iterative Tarjan) of the square part with every matched pair contracted:
                  vertex = square row, arc r -> mate_col[c] per entry (r, c) with c in the square part; id = the smallest row
  validate        a matching is one: mates mutual, every pair an entry; returns its size
"""
import numpy as np

HORIZONTAL, SQUARE, VERTICAL = 0, 1, 2


def read_pattern(path):
    """(shape, ro, ci) of a Matrix Market coordinate file as it stands: every listed entry, the diagonal too, and the mirror of
    every off-diagonal one when the file says symmetric"""
    with open(path) as f:
        header = f.readline().lower().split()
        line = f.readline()
        while line.startswith("%"):
            line = f.readline()
        rows, cols, count = (int(x) for x in line.split()[:3])
        data = np.loadtxt(f, usecols=(0, 1), dtype=np.int64, ndmin=2)
    assert data.shape[0] == count
    r, c = data[:, 0] - 1, data[:, 1] - 1
    if "symmetric" in header:
        off = r != c
        r, c = np.concatenate([r, c[off]]), np.concatenate([c, r[off]])
    return from_pairs((rows, cols), r, c)


def from_pairs(shape, r, c):
    """(shape, ro, ci) with the entries of a row in the order given"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    order = np.argsort(r, kind="stable")
    ro = np.zeros(shape[0] + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=shape[0]), out=ro[1:])
    return (int(shape[0]), int(shape[1])), ro, c[order].astype(np.int32)


def take_rows(matrix, count):
    """the first `count` rows"""
    (rows, cols), ro, ci = matrix
    return (count, cols), ro[:count + 1].copy(), ci[:ro[count]].copy()


def take_cols(matrix, count):
    """the first `count` columns"""
    (rows, cols), ro, ci = matrix
    r = np.repeat(np.arange(rows), np.diff(ro))
    keep = ci < count
    return from_pairs((rows, count), r[keep], ci[keep])


def transpose(matrix):
    (rows, cols), ro, ci = matrix
    return from_pairs((cols, rows), ci, np.repeat(np.arange(rows), np.diff(ro)))


def hopcroft_karp(matrix):
    """(mate_row, mate_col) of a maximum matching, int32 with -1 for unmatched"""
    (rows, cols), ro, ci = matrix
    ro, ci = ro.tolist(), ci.tolist()
    mate_row, mate_col = [-1] * rows, [-1] * cols
    INF = rows + cols + 5
    while True:
        # layers: dist[r] over rows, from the unmatched ones
        dist = [INF] * rows
        queue = [r for r in range(rows) if mate_row[r] < 0]
        for r in queue:
            dist[r] = 0
        reach = INF
        at = 0
        while at < len(queue):
            r = queue[at]
            at += 1
            if dist[r] >= reach:
                continue
            for i in range(ro[r], ro[r + 1]):
                m = mate_col[ci[i]]
                if m < 0:
                    reach = min(reach, dist[r] + 1)
                elif dist[m] == INF:
                    dist[m] = dist[r] + 1
                    queue.append(m)
        if reach == INF:
            break
        # disjoint shortest paths, depth first with an explicit stack
        cursor = [ro[r] for r in range(rows)]
        for start in range(rows):
            if mate_row[start] >= 0:
                continue
            stack = [start]
            while stack:
                r = stack[-1]
                if cursor[r] == ro[r + 1]:
                    dist[r] = INF
                    stack.pop()
                    continue
                c = ci[cursor[r]]
                cursor[r] += 1
                m = mate_col[c]
                if m < 0:
                    if dist[r] + 1 != reach:
                        continue
                    # flip the path on the stack: row stack[k] takes the column it was looking at
                    for k in range(len(stack) - 1, -1, -1):
                        rk = stack[k]
                        ck = ci[cursor[rk] - 1]
                        mate_row[rk], mate_col[ck] = ck, rk
                    for rk in stack:
                        dist[rk] = INF
                    stack = []
                elif dist[m] == dist[r] + 1:
                    stack.append(m)
    return np.array(mate_row, np.int32).reshape(rows), np.array(mate_col, np.int32).reshape(cols)


def validate(matrix, mate_row, mate_col):
    """the size of the matching; raises when it is none"""
    (rows, cols), ro, ci = matrix
    mate_row, mate_col = np.asarray(mate_row), np.asarray(mate_col)
    assert mate_row.shape == (rows,) and mate_col.shape == (cols,)
    size = 0
    for r in range(rows):
        c = int(mate_row[r])
        if c < 0:
            assert c == -1
            continue
        assert 0 <= c < cols and mate_col[c] == r, "row %d: mates are not mutual" % r
        assert c in ci[ro[r]:ro[r + 1]], "pair (%d, %d) is no entry" % (r, c)
        size += 1
    for c in range(cols):
        r = int(mate_col[c])
        assert r == -1 or (0 <= r < rows and mate_row[r] == c), "column %d: mates are not mutual" % c
    return size


def _reach(adj_ro, adj_ci, mate_u, mate_w, n_w):
    """(reached u, reached w) by alternating paths from the unmatched u over u's adjacency"""
    seen_u, seen_w = np.zeros(len(mate_u), bool), np.zeros(n_w, bool)
    stack = [u for u in range(len(mate_u)) if mate_u[u] < 0]
    seen_u[stack] = True
    while stack:
        u = stack.pop()
        for w in adj_ci[adj_ro[u]:adj_ro[u + 1]].tolist():
            if seen_w[w]:
                continue
            seen_w[w] = True
            m = int(mate_w[w])
            if m >= 0 and not seen_u[m]:
                seen_u[m] = True
                stack.append(m)
    return seen_u, seen_w


def parts(matrix, mate_row, mate_col):
    """(row_part, col_part) as int32 from a maximum matching"""
    (rows, cols), ro, ci = matrix
    _, t_ro, t_ci = transpose(matrix)
    h_cols, h_rows = _reach(t_ro, t_ci, mate_col, mate_row, rows)
    v_rows, v_cols = _reach(ro, ci, mate_row, mate_col, cols)
    assert not (h_rows & v_rows).any() and not (h_cols & v_cols).any(), "the matching is not maximum"
    row_part, col_part = np.full(rows, SQUARE, np.int32), np.full(cols, SQUARE, np.int32)
    row_part[h_rows], col_part[h_cols] = HORIZONTAL, HORIZONTAL
    row_part[v_rows], col_part[v_cols] = VERTICAL, VERTICAL
    return row_part, col_part


def cover(row_part, col_part):
    """(row_cover, col_cover) as uint8"""
    return (row_part != VERTICAL).astype(np.uint8), (col_part == VERTICAL).astype(np.uint8)


def blocks(matrix, mate_row, mate_col, row_part, col_part):
    """(row_block, col_block, count): int32, the smallest row of the block, -1 outside the square part"""
    (rows, cols), ro, ci = matrix
    square = row_part == SQUARE
    succ = {}
    for r in np.flatnonzero(square).tolist():
        succ[r] = [int(mate_col[c]) for c in ci[ro[r]:ro[r + 1]].tolist() if col_part[c] == SQUARE]
    index, low, on_stack, comp = {}, {}, set(), {}
    order, counter, count = [], 0, 0
    for root in succ:
        if root in index:
            continue
        work = [(root, 0)]
        index[root] = low[root] = counter
        counter += 1
        order.append(root)
        on_stack.add(root)
        while work:
            v, i = work.pop()
            if i < len(succ[v]):
                work.append((v, i + 1))
                w = succ[v][i]
                if w not in index:
                    index[w] = low[w] = counter
                    counter += 1
                    order.append(w)
                    on_stack.add(w)
                    work.append((w, 0))
                elif w in on_stack:
                    low[v] = min(low[v], index[w])
            else:
                if work:
                    parent = work[-1][0]
                    low[parent] = min(low[parent], low[v])
                if low[v] == index[v]:
                    members = []
                    while True:
                        w = order.pop()
                        on_stack.discard(w)
                        members.append(w)
                        if w == v:
                            break
                    count += 1
                    for w in members:
                        comp[w] = min(members)
    row_block, col_block = np.full(rows, -1, np.int32), np.full(cols, -1, np.int32)
    for r, b in comp.items():
        row_block[r] = b
        col_block[mate_row[r]] = b
    return row_block, col_block, count


def decompose(matrix, matching=None):
    """everything, from `matching` = (mate_row, mate_col) or from hopcroft_karp's"""
    mate_row, mate_col = hopcroft_karp(matrix) if matching is None else matching
    size = validate(matrix, mate_row, mate_col)
    row_part, col_part = parts(matrix, mate_row, mate_col)
    row_cover, col_cover = cover(row_part, col_part)
    row_block, col_block, count = blocks(matrix, mate_row, mate_col, row_part, col_part)
    part_sizes = [int((row_part == p).sum()) for p in range(3)] + [int((col_part == p).sum()) for p in range(3)]
    return {"size": size, "mate_row": mate_row, "mate_col": mate_col, "row_part": row_part, "col_part": col_part, "part_sizes": part_sizes,
            "row_cover": row_cover, "col_cover": col_cover, "row_block": row_block, "col_block": col_block, "blocks": count}
