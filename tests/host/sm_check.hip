// tests/host/sm_check.hip -- the plan of subgraph matching (app/sm/sm_plan.hpp), without a GPU: |Aut(H)| and the symmetry-breaking
// constraints of the named patterns, the matching orders, the masks of a house, every refusal, and -- by a host search over the
// plan's levels on a fixed 10-vertex graph -- that for every connected pattern of up to 5 vertices the constrained count times aut
// is the unconstrained count, which is the count of a search that knows nothing of the plan.  Built with -Xarch_host
// -fsanitize=address,undefined by tests/test_sm_host.py; makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <gunrock/app/sm/sm_plan.hpp>

using namespace gunrock::app::sm;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

namespace {

struct Pattern {
    int q;
    std::vector<int> a, b;
};

Pattern Make(int q, std::initializer_list<std::pair<int, int>> pairs)
{
    Pattern p{q, {}, {}};
    for (auto e : pairs) {
        p.a.push_back(e.first);
        p.b.push_back(e.second);
    }
    return p;
}

int Build(const Pattern &p, const int *plabels, bool induced, bool symmetry, int order, Plan *plan)
{
    return BuildPlan(p.q, static_cast<int>(p.a.size()), p.a.data(), p.b.data(), plabels, induced, symmetry, order, plan);
}

bool HasConstraint(const Plan &plan, int lo, int hi)
{
    for (int i = 0; i < plan.constraints; ++i)
        if (plan.cons_lo[i] == lo && plan.cons_hi[i] == hi) return true;
    return false;
}

// the fixed graph: the Petersen graph and four chords (triangles, 4-cycles, a vertex of degree 5)
constexpr int kN = 10;
bool g_adj[kN][kN];
int g_label[kN] = {0, 1, 2, 0, 1, 2, 0, 1, 2, 0};

void MakeGraph()
{
    const int edges[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 0}, {0, 5}, {1, 6}, {2, 7}, {3, 8}, {4, 9}, {5, 7}, {7, 9}, {9, 6}, {6, 8}, {8, 5},
                            {0, 2}, {1, 3}, {5, 6}, {0, 7}};
    for (auto &e : edges) g_adj[e[0]][e[1]] = g_adj[e[1]][e[0]] = true;
}

int Degree(int v)
{
    int d = 0;
    for (int u = 0; u < kN; ++u) d += g_adj[v][u];
    return d;
}

// the search the kernels run, on the host: level by level over the plan's masks
long long Search(const PlanLevels &plan, int level, int *image)
{
    if (level == plan.q) return 1;
    const Level &lv = plan.level[level];
    long long found = 0;
    for (int c = 0; c < kN; ++c) {
        bool ok = (lv.plabel == kWildcard || g_label[c] == lv.plabel) && Degree(c) >= lv.min_degree;
        for (int j = 0; j < level && ok; ++j) {
            ok = c != image[j];
            if (lv.must >> j & 1u) ok = ok && g_adj[c][image[j]];
            if (lv.mustnot >> j & 1u) ok = ok && !g_adj[c][image[j]];
            if (lv.lt >> j & 1u) ok = ok && c < image[j];
            if (lv.gt >> j & 1u) ok = ok && c > image[j];
        }
        if (!ok) continue;
        image[level] = c;
        found += Search(plan, level + 1, image);
    }
    return found;
}

// ... and one that knows nothing of the plan: pattern vertices in id order, every injective map tested against the definition
long long Plain(const Pattern &p, const int *plabels, bool induced, int v, int *image)
{
    if (v == p.q) {
        bool padj[kMaxQ][kMaxQ] = {};
        for (size_t i = 0; i < p.a.size(); ++i) padj[p.a[i]][p.b[i]] = padj[p.b[i]][p.a[i]] = true;
        for (int i = 0; i < p.q; ++i)
            for (int j = 0; j < i; ++j) {
                if (padj[i][j] && !g_adj[image[i]][image[j]]) return 0;
                if (induced && !padj[i][j] && g_adj[image[i]][image[j]]) return 0;
            }
        return 1;
    }
    long long found = 0;
    for (int c = 0; c < kN; ++c) {
        bool ok = !plabels || plabels[v] == kWildcard || plabels[v] == g_label[c];
        for (int j = 0; j < v && ok; ++j) ok = image[j] != c;
        if (!ok) continue;
        image[v] = c;
        found += Plain(p, plabels, induced, v + 1, image);
    }
    return found;
}

}  // namespace

int main()
{
    Plan plan;

    // |Aut(H)| and the constraints of the named patterns
    const Pattern wedge = Make(3, {{0, 1}, {1, 2}}), triangle = Make(3, {{0, 1}, {1, 2}, {0, 2}}), p4 = Make(4, {{0, 1}, {1, 2}, {2, 3}}),
                  claw = Make(4, {{0, 1}, {0, 2}, {0, 3}}), c4 = Make(4, {{0, 1}, {1, 2}, {2, 3}, {3, 0}}),
                  paw = Make(4, {{0, 1}, {1, 2}, {0, 2}, {2, 3}}), diamond = Make(4, {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}}),
                  k4 = Make(4, {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}}), c5 = Make(5, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 0}}),
                  house = Make(5, {{0, 1}, {0, 2}, {1, 2}, {1, 3}, {2, 4}, {3, 4}}), bull = Make(5, {{0, 1}, {1, 2}, {0, 2}, {1, 3}, {2, 4}}),
                  c6 = Make(6, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 0}});
    const struct {
        const Pattern *p;
        int aut, constraints;
    } named[] = {{&wedge, 2, 1}, {&triangle, 6, 3}, {&p4, 2, 1}, {&claw, 6, 3}, {&c4, 8, 4}, {&paw, 2, 1},
                 {&diamond, 4, 2}, {&k4, 24, 6}, {&c5, 10, 5}, {&house, 2, 1}, {&bull, 2, 1}, {&c6, 12, 6}};
    for (auto &x : named) {
        CHECK(Build(*x.p, nullptr, false, true, ORDER_RULE, &plan) == 0);
        CHECK(plan.aut == x.aut && plan.constraints == x.constraints && plan.q == x.p->q);
    }
    CHECK(Build(wedge, nullptr, false, true, 0, &plan) == 0 && plan.constraints == 1 && HasConstraint(plan, 0, 2));
    CHECK(Build(p4, nullptr, false, true, 0, &plan) == 0 && plan.constraints == 1 && HasConstraint(plan, 0, 3));
    CHECK(Build(paw, nullptr, false, true, 0, &plan) == 0 && plan.constraints == 1 && HasConstraint(plan, 0, 1));
    CHECK(Build(diamond, nullptr, false, true, 0, &plan) == 0 && plan.constraints == 2 && HasConstraint(plan, 0, 1) && HasConstraint(plan, 2, 3));
    CHECK(Build(k4, nullptr, false, true, 0, &plan) == 0);
    for (int lo = 0; lo < 4; ++lo)
        for (int hi = lo + 1; hi < 4; ++hi) CHECK(HasConstraint(plan, lo, hi));  // six constraints: the total order 0 < 1 < 2 < 3
    // duplicates and both orientations are one edge; labels cut the group down, the wildcard a label of its own
    const Pattern twice = Make(3, {{0, 1}, {1, 0}, {1, 2}, {1, 2}, {2, 1}});
    CHECK(Build(twice, nullptr, false, true, 0, &plan) == 0 && plan.aut == 2 && plan.edges == 2);
    const int l001[] = {0, 0, 1}, lw[] = {0, -1, 1}, l1w1[] = {1, -1, 1};
    CHECK(Build(triangle, l001, false, true, 0, &plan) == 0 && plan.aut == 2 && HasConstraint(plan, 0, 1));
    CHECK(Build(triangle, lw, false, true, 0, &plan) == 0 && plan.aut == 1 && plan.constraints == 0);
    CHECK(Build(wedge, l1w1, false, true, 0, &plan) == 0 && plan.aut == 2);

    // the house under the rule: order 1, 2, 0, 3, 4; its masks not induced and induced; its one constraint 1 < 2 sits at level 1
    CHECK(Build(house, nullptr, false, true, ORDER_RULE, &plan) == 0);
    const int house_order[] = {1, 2, 0, 3, 4};
    for (int l = 0; l < 5; ++l) CHECK(plan.order[l] == house_order[l] && plan.pos[house_order[l]] == l);
    const unsigned must[] = {0, 1, 3, 1, 10}, parent[] = {0, 0, 0, 0, 1}, degree[] = {3, 3, 2, 2, 2};
    for (int l = 0; l < 5; ++l) {
        CHECK(plan.levels.level[l].must == must[l] && plan.levels.level[l].mustnot == 0 && plan.levels.level[l].min_degree == static_cast<int>(degree[l]));
        if (l > 0) CHECK(plan.levels.level[l].parent == static_cast<int>(parent[l]));
        CHECK(plan.levels.level[l].lt == 0 && plan.levels.level[l].gt == (l == 1 ? 1u : 0u));
    }
    CHECK(HasConstraint(plan, 1, 2));
    CHECK(Build(house, nullptr, true, true, ORDER_RULE, &plan) == 0);
    const unsigned mustnot[] = {0, 0, 0, 6, 5};
    for (int l = 0; l < 5; ++l) CHECK(plan.levels.level[l].must == must[l] && plan.levels.level[l].mustnot == mustnot[l]);
    CHECK(Build(house, nullptr, true, false, ORDER_RULE, &plan) == 0 && plan.aut == 2 && plan.constraints == 1);
    for (int l = 0; l < 5; ++l) CHECK(plan.levels.level[l].lt == 0 && plan.levels.level[l].gt == 0);  // no symmetry: no lt / gt
    CHECK(Build(house, nullptr, false, true, ORDER_ID, &plan) == 0);
    for (int l = 0; l < 5; ++l) CHECK(plan.order[l] == l);
    CHECK(plan.levels.level[2].lt == 0 && plan.levels.level[2].gt == 2u);  // 1 < 2 at level 2, against level 1
    const Pattern late = Make(3, {{0, 2}, {1, 2}});  // ascending ids are no connected order: the rule instead
    CHECK(Build(late, nullptr, false, true, ORDER_ID, &plan) == 0 && plan.order[0] == 2 && plan.order[1] == 0 && plan.order[2] == 1);
    CHECK(plan.levels.level[2].lt == 0 && plan.levels.level[2].gt == 2u);  // 0 < 1: level 2 above level 1

    // every refusal
    const Pattern far = Make(4, {{0, 1}, {2, 3}}), loop = Make(3, {{0, 1}, {1, 1}, {1, 2}}), out = Make(3, {{0, 1}, {1, 3}}),
                  negative = Make(3, {{0, 1}, {-1, 2}}), one = Make(1, {}), seven = Make(7, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}}),
                  none = Make(2, {});
    const int below[] = {0, -2, 0};
    plan.q = 99;
    CHECK(Build(far, nullptr, false, true, 0, &plan) == -1 && Build(loop, nullptr, false, true, 0, &plan) == -1);
    CHECK(Build(out, nullptr, false, true, 0, &plan) == -1 && Build(negative, nullptr, false, true, 0, &plan) == -1);
    CHECK(Build(one, nullptr, false, true, 0, &plan) == -1 && Build(seven, nullptr, false, true, 0, &plan) == -1);
    CHECK(Build(none, nullptr, false, true, 0, &plan) == -1 && Build(wedge, below, false, true, 0, &plan) == -1);
    CHECK(BuildPlan(3, -1, nullptr, nullptr, nullptr, false, true, 0, &plan) == -1 && BuildPlan(3, 2, nullptr, nullptr, nullptr, false, true, 0, &plan) == -1);
    CHECK(Build(wedge, nullptr, false, true, 3, &plan) == -1 && Build(wedge, nullptr, false, true, -1, &plan) == -1);
    CHECK(plan.q == 99);  // a refusal writes nothing

    // every connected pattern of 2 .. 5 vertices (every edge subset that is one): every order is connected; on the fixed graph
    // constrained x aut == unconstrained under every order, induced and not; the unconstrained count is the plain search's
    MakeGraph();
    long long patterns = 0, nonzero = 0;
    for (int q = 2; q <= 5; ++q) {
        std::vector<std::pair<int, int>> slots;
        for (int i = 0; i < q; ++i)
            for (int j = i + 1; j < q; ++j) slots.push_back({i, j});
        for (unsigned bits = 1; bits < (1u << slots.size()); ++bits) {
            Pattern p{q, {}, {}};
            for (size_t s = 0; s < slots.size(); ++s)
                if (bits >> s & 1u) {
                    p.a.push_back(slots[s].first);
                    p.b.push_back(slots[s].second);
                }
            if (Build(p, nullptr, false, true, ORDER_RULE, &plan)) continue;  // disconnected
            ++patterns;
            const int labels[] = {static_cast<int>(bits % 3), -1, static_cast<int>(bits / 3 % 3), 0, -1};
            for (int labelled = 0; labelled < (q <= 4 ? 2 : 1); ++labelled)
                for (int induced = 0; induced < 2; ++induced) {
                    const int *pl = labelled ? labels : nullptr;
                    long long want = -1;
                    int plain_image[kMaxQ];
                    for (int order = ORDER_RULE; order <= (q <= 4 ? ORDER_ID : ORDER_RULE); ++order) {
                        Plan with, without;
                        int image[kMaxQ];
                        CHECK(Build(p, pl, induced != 0, true, order, &with) == 0 && Build(p, pl, induced != 0, false, order, &without) == 0);
                        unsigned placed = 0;
                        for (int l = 0; l < q; ++l) {  // a permutation in which every vertex behind the first has an earlier neighbour
                            CHECK(with.order[l] >= 0 && with.order[l] < q && !(placed >> with.order[l] & 1u));
                            CHECK(l == 0 || (with.adj[with.order[l]] & placed) != 0);
                            CHECK(l == 0 || (with.levels.level[l].must != 0 && with.levels.level[l].parent >= 0 && with.levels.level[l].parent < l));
                            placed |= 1u << with.order[l];
                        }
                        const long long constrained = Search(with.levels, 0, image), all = Search(without.levels, 0, image);
                        CHECK(constrained * with.aut == all && with.aut == without.aut);
                        if (want < 0) want = all;
                        CHECK(all == want);  // the order never changes a count
                        nonzero += all > 0;
                    }
                    if (q <= 4 || bits % 7 == 0) CHECK(Plain(p, pl, induced != 0, 0, plain_image) == want);
                }
        }
    }
    CHECK(patterns == 1 + 4 + 38 + 728 && nonzero > 1000);  // the connected labelled graphs on 2, 3, 4 and 5 vertices

    std::printf("sm host checks passed\n");
    return 0;
}
