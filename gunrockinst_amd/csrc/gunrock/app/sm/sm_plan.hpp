// app/sm/sm_plan.hpp -- the host side of subgraph matching: from a pattern to what the kernels search by.  No HIP call.
//
// A pattern H has q vertices (2 .. 6), a list of pairs (duplicates and both orientations are one edge), an optional int32 label per
// vertex (-1: a wildcard) and the flag `induced`.  BuildPlan refuses what is no pattern and gives
//   aut          |Aut(H)|: the label-preserving automorphisms, the wildcard a label of its own, by brute force over the q! <= 720
//                permutations
//   cons         the symmetry-breaking constraints f(lo) < f(hi) of Grochow and Kellis: while the group A (at first Aut(H)) moves a
//                vertex, v = the smallest moved one, f(v) < f(u) for every other u of v's orbit under A, A = the stabiliser of v.
//                Under them every occurrence has exactly one embedding.
//   order        the matching order: every vertex behind the first has an earlier neighbour
//   level[l]     for the vertex order[l]: its label and degree, `must` / `mustnot` (the earlier levels it has to be / must not be
//                adjacent to; mustnot only when induced), `parent` (the earliest level of must: the anchor tree T), and `lt` / `gt`
//                (the earlier levels whose image has to be greater / smaller than this one's: a constraint sits at the level where
//                its later end is bound; both 0 without `symmetry`)
// PlanLevels is what a kernel takes by value.
#pragma once

#include <algorithm>

namespace gunrock {
namespace app {
namespace sm {

constexpr int kMinQ = 2, kMaxQ = 6;
constexpr int kMaxPairs = kMaxQ * (kMaxQ - 1) / 2;
constexpr int kWildcard = -1;

enum { ORDER_RULE = 0, ORDER_REVERSE = 1, ORDER_ID = 2 };

struct Level {
    int plabel = kWildcard;
    int min_degree = 0;
    int parent = -1;
    unsigned must = 0, mustnot = 0, lt = 0, gt = 0;
};

struct PlanLevels {
    int q = 0;
    Level level[kMaxQ];
};

struct Plan {
    int q = 0, induced = 0, edges = 0;
    int aut = 1;
    int constraints = 0;
    int cons_lo[kMaxPairs], cons_hi[kMaxPairs];  // f(cons_lo[i]) < f(cons_hi[i])
    int order[kMaxQ], pos[kMaxQ];                // pos[order[l]] = l
    int plabel[kMaxQ], degree[kMaxQ];
    unsigned adj[kMaxQ];  // bit u of adj[v]: v -- u
    PlanLevels levels;
};

// v before u in the order rule's key: the larger degree, labelled before wildcard, the smaller id
inline bool KeyBefore(const Plan &p, int v, int u)
{
    if (p.degree[v] != p.degree[u]) return p.degree[v] > p.degree[u];
    const bool lv = p.plabel[v] != kWildcard, lu = p.plabel[u] != kWildcard;
    if (lv != lu) return lv;
    return v < u;
}

inline int PopCount(unsigned x)
{
    int c = 0;
    for (; x; x &= x - 1) ++c;
    return c;
}

// rule ORDER_RULE: the first by the key, then always the vertex with the most earlier neighbours, ties by the key.  ORDER_REVERSE:
// the last by the key, then the vertex with the fewest (but one) earlier neighbours, ties by the reversed key.  ORDER_ID: 0, 1, ..
// when that is a connected order, else ORDER_RULE.
inline void MatchingOrder(Plan &p, int rule)
{
    const int q = p.q;
    if (rule == ORDER_ID) {
        bool connected = true;
        for (int v = 1; v < q; ++v) connected = connected && (p.adj[v] & ((1u << v) - 1u)) != 0;
        if (connected) {
            for (int v = 0; v < q; ++v) p.order[v] = v;
            return;
        }
        rule = ORDER_RULE;
    }
    const bool reverse = rule == ORDER_REVERSE;
    unsigned placed = 0;
    for (int l = 0; l < q; ++l) {
        int best = -1, best_back = 0;
        for (int v = 0; v < q; ++v) {
            if (placed >> v & 1u) continue;
            const int back = PopCount(p.adj[v] & placed);
            if (l > 0 && back == 0) continue;
            bool better = best < 0;
            if (!better && back != best_back) better = reverse ? back < best_back : back > best_back;
            else if (!better) better = reverse ? KeyBefore(p, best, v) : KeyBefore(p, v, best);
            if (better) best = v, best_back = back;
        }
        p.order[l] = best;  // (connected: there is one)
        placed |= 1u << best;
    }
}

// 0, or -1 for what is no pattern: q outside 2 .. 6, an endpoint out of range, a self-loop, a label below -1, a disconnected H.
// `plabels` may be NULL: all wildcards.  Nothing of *out is meaningful behind a refusal.
inline int BuildPlan(int q, int npairs, const int *a, const int *b, const int *plabels, bool induced, bool symmetry, int order_rule, Plan *out)
{
    Plan p;
    if (q < kMinQ || q > kMaxQ || npairs < 0 || (npairs > 0 && (!a || !b))) return -1;
    if (order_rule < ORDER_RULE || order_rule > ORDER_ID) return -1;
    p.q = q;
    p.induced = induced ? 1 : 0;
    for (int v = 0; v < kMaxQ; ++v) {
        p.adj[v] = 0;
        p.plabel[v] = kWildcard;
        p.degree[v] = 0;
        p.order[v] = p.pos[v] = 0;
    }
    for (int i = 0; i < kMaxPairs; ++i) p.cons_lo[i] = p.cons_hi[i] = 0;
    for (int v = 0; v < q; ++v) {
        p.plabel[v] = plabels ? plabels[v] : kWildcard;
        if (p.plabel[v] < kWildcard) return -1;
    }
    for (int i = 0; i < npairs; ++i) {
        if (a[i] < 0 || a[i] >= q || b[i] < 0 || b[i] >= q || a[i] == b[i]) return -1;
        p.adj[a[i]] |= 1u << b[i];
        p.adj[b[i]] |= 1u << a[i];
    }
    unsigned seen = 1u;  // connected: everything is reached from vertex 0
    for (int round = 0; round < q; ++round)
        for (int v = 0; v < q; ++v)
            if (seen >> v & 1u) seen |= p.adj[v];
    if (seen != (1u << q) - 1u) return -1;
    for (int v = 0; v < q; ++v) {
        p.degree[v] = PopCount(p.adj[v]);
        p.edges += p.degree[v];
    }
    p.edges /= 2;

    // Aut(H) by brute force
    int perms[720][kMaxQ];
    int count = 0;
    int perm[kMaxQ] = {0, 1, 2, 3, 4, 5};
    do {
        bool keeps = true;
        for (int v = 0; v < q && keeps; ++v) {
            keeps = p.plabel[perm[v]] == p.plabel[v];
            for (int u = 0; u < v && keeps; ++u) keeps = (p.adj[v] >> u & 1u) == (p.adj[perm[v]] >> perm[u] & 1u);
        }
        if (keeps) {
            for (int v = 0; v < q; ++v) perms[count][v] = perm[v];
            ++count;
        }
    } while (std::next_permutation(perm, perm + q));
    p.aut = count;

    // the constraints: A = perms[0 .. count)
    while (count > 1) {
        int v = q;
        for (int i = 0; i < count; ++i)
            for (int u = 0; u < v; ++u)
                if (perms[i][u] != u) v = u;
        unsigned orbit = 0;
        for (int i = 0; i < count; ++i) orbit |= 1u << perms[i][v];
        for (int u = 0; u < q; ++u)
            if (u != v && (orbit >> u & 1u)) {
                p.cons_lo[p.constraints] = v;
                p.cons_hi[p.constraints] = u;
                ++p.constraints;
            }
        int kept = 0;
        for (int i = 0; i < count; ++i)
            if (perms[i][v] == v) {
                for (int u = 0; u < q; ++u) perms[kept][u] = perms[i][u];
                ++kept;
            }
        count = kept;
    }

    MatchingOrder(p, order_rule);
    for (int l = 0; l < q; ++l) p.pos[p.order[l]] = l;
    p.levels.q = q;
    for (int l = 0; l < q; ++l) {
        Level &lv = p.levels.level[l];
        const int v = p.order[l];
        lv.plabel = p.plabel[v];
        lv.min_degree = p.degree[v];
        for (int k = 0; k < l; ++k) {
            if (p.adj[v] >> p.order[k] & 1u) lv.must |= 1u << k;
            else if (induced) lv.mustnot |= 1u << k;
        }
        for (int k = l - 1; k >= 0; --k)
            if (lv.must >> k & 1u) lv.parent = k;
    }
    if (symmetry)
        for (int i = 0; i < p.constraints; ++i) {
            const int lo = p.pos[p.cons_lo[i]], hi = p.pos[p.cons_hi[i]];
            if (lo > hi) p.levels.level[lo].lt |= 1u << hi;  // f(lo) is bound later: below the image of level hi
            else p.levels.level[hi].gt |= 1u << lo;
        }
    *out = p;
    return 0;
}

}  // namespace sm
}  // namespace app
}  // namespace gunrock
