// lib/sm_app.hip -- subgraph-matching entry points of libgunrock.so.
//  * grx_sm_*: SmProblem / SmEnactor phases as separate C calls (the reference snapshot's app/sm is a stub; the calls are shaped like
//    grx_clique_*).  A handle takes one graph and any number of patterns, one at a time; Extract gives one 64-bit count per vertex,
//    the occurrences and the embeddings.
#include <gunrock/gunrock_mi355x.h>

#include <vector>

#include <gunrock/app/handle_runner.hpp>
#include <gunrock/app/sm/sm_enactor.hpp>
#include <gunrock/app/sm/sm_problem.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::sm;

static_assert(GRX_SM_AUTO == SM_AUTO && GRX_SM_GROUP8 == SM_GROUP8 && GRX_SM_WAVE == SM_WAVE, "the header's strategies are the kernels' strategies");
static_assert(GRX_SM_TOO_LARGE == kTooLarge && GRX_SM_NOT_CERTIFIED == kNotCertified, "the header's codes are the enactor's");
static_assert(GRX_SM_MAX_Q == kMaxQ && GRX_SM_MAX_CONSTRAINTS == kMaxPairs, "the header's sizes are the plan's");
static_assert(sizeof(long long) == sizeof(Count), "counts are 64-bit");

namespace {

struct SmStats {
    long long items = 0, regime[2] = {0, 0}, streamed = 0, bisections = 0, occurrences = 0, embeddings = 0, pairs = 0, longest = 0, launches = 0;
    double bound = 0, kernel_ms = 0, kind_ms[MS_COUNT] = {0, 0, 0, 0}, build_ms = 0;
};

struct SmRunner {
    InitState state;
    bool finished = false;  // the last Enact ran to its end: there is a result to extract
    // the pattern as it was given, and its plan under the options in force
    bool has_pattern = false, has_plabels = false, induced = false;
    int q = 0;
    std::vector<int> pa, pb;
    int plabels[kMaxQ] = {0, 0, 0, 0, 0, 0};
    Plan plan;
    SmOptions options;

    virtual ~SmRunner() {}
    virtual int Init(const Csr<int, int, int> &g, const int *labels) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, const int *d_labels) = 0;
    virtual void NewPlan() = 0;
    virtual hipError_t Reset() = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(SmStats &s) = 0;
    virtual hipError_t Extract(long long *count, long long *occurrences, long long *embeddings) = 0;
    virtual void DeviceResults(long long **d_count, int **d_degrees) = 0;

    // a refused pattern installs nothing: the one before it stays
    int SetPattern(int q_, int npairs, const int *a, const int *b, const int *labels, bool induced_)
    {
        Plan next;
        if (BuildPlan(q_, npairs, a, b, labels, induced_, options.symmetry != 0, options.order, &next)) return -1;
        q = q_;
        pa.assign(a, a + npairs);
        pb.assign(b, b + npairs);
        has_plabels = labels != nullptr;
        for (int v = 0; v < q_; ++v) plabels[v] = labels ? labels[v] : kWildcard;
        induced = induced_;
        plan = next;
        has_pattern = true;
        finished = false;
        NewPlan();
        return 0;
    }
    // 0 taken, -1 out of range, 1 unknown; a new "symmetry" or "order" plans the pattern in force again
    int SetOption(const char *name, double value)
    {
        const int symmetry = options.symmetry, order = options.order;
        const int rc = options.Set(name, value);
        if (rc == 0 && has_pattern && (symmetry != options.symmetry || order != options.order)) {
            BuildPlan(q, static_cast<int>(pa.size()), pa.data(), pb.data(), has_plabels ? plabels : nullptr, induced, options.symmetry != 0, options.order, &plan);
            finished = false;
            NewPlan();
        }
        return rc;
    }
};

template <bool INSTR>
struct SmRunnerT : SmRunner {
    typedef SmProblem<false> Problem;
    Problem problem;
    SmEnactor<INSTR> enactor;
    EventPair timer;
    explicit SmRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g, const int *labels) override
    {
        const hipError_t rc = problem.Init(false, g, labels, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, const int *d_labels) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci, d_labels);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    void NewPlan() override { enactor.bound_known = false; }
    hipError_t Reset() override
    {
        if (!state.ready) return hipErrorNotReady;
        finished = false;
        return problem.Reset();
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready || !has_pattern) return static_cast<int>(hipErrorNotReady);
        finished = false;
        const hipError_t rc = timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, plan, options, max_grid_size); });
        if (rc) return static_cast<int>(rc);
        if (enactor.code) return enactor.code;
        finished = true;
        return 0;
    }
    void Stats(SmStats &s) override
    {
        s.items = enactor.items[0] + enactor.items[1];
        s.regime[0] = enactor.items[0];
        s.regime[1] = enactor.items[1];
        s.streamed = enactor.streamed;
        s.bisections = enactor.bisections;
        s.occurrences = enactor.occurrences;
        s.embeddings = enactor.embeddings;
        s.pairs = problem.pairs;
        s.longest = problem.longest_row;
        s.launches = enactor.host.launches;
        s.bound = enactor.bound;
        s.kernel_ms = enactor.host.kernel_ms;
        for (int i = 0; i < MS_COUNT; ++i) s.kind_ms[i] = enactor.kind_ms[i];
        s.build_ms = problem.build_ms;
    }
    hipError_t Extract(long long *count, long long *occurrences, long long *embeddings) override
    {
        if (!state.ready || !finished) return hipErrorNotReady;
        if (occurrences) *occurrences = enactor.occurrences;
        if (embeddings) *embeddings = enactor.embeddings;
        return problem.Read(count, reinterpret_cast<const long long *>(problem.data_slices[0]->d_count.p), static_cast<size_t>(problem.nodes));
    }
    void DeviceResults(long long **d_count, int **d_degrees) override
    {
        if (d_count) *d_count = state.ready ? reinterpret_cast<long long *>(problem.data_slices[0]->d_count.p) : nullptr;
        if (d_degrees) *d_degrees = state.ready ? reinterpret_cast<int *>(problem.data_slices[0]->d_deg.p) : nullptr;
    }
};

}  // namespace

struct grx_sm {
    std::unique_ptr<SmRunner> runner;
};

extern "C" {

int grx_sm_create(grx_sm **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_sm{MakeRunner<SmRunner, SmRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_sm_init(grx_sm *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *labels)
{
    if (!p || !row_offsets || nodes < 0 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph, labels);
}

int grx_sm_init_device(grx_sm *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, const int *d_labels)
{
    if (!p || !d_row_offsets || nodes < 0 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_labels);
}

int grx_sm_set_pattern(grx_sm *p, int q, int num_pairs, const int *a, const int *b, const int *pattern_labels, int induced)
{
    if (!p) return -1;
    return p->runner->SetPattern(q, num_pairs, a, b, pattern_labels, induced != 0);
}

int grx_sm_pattern_info(grx_sm *p, int *q, int *aut, int *order, int *num_constraints, int *lower, int *higher)
{
    if (!p) return -1;
    const SmRunner &r = *p->runner;
    if (!r.has_pattern) return static_cast<int>(hipErrorNotReady);
    if (q) *q = r.plan.q;
    if (aut) *aut = r.plan.aut;
    if (num_constraints) *num_constraints = r.plan.constraints;
    for (int i = 0; i < kMaxQ; ++i)
        if (order) order[i] = i < r.plan.q ? r.plan.order[i] : -1;
    for (int i = 0; i < kMaxPairs; ++i) {
        if (lower) lower[i] = i < r.plan.constraints ? r.plan.cons_lo[i] : -1;
        if (higher) higher[i] = i < r.plan.constraints ? r.plan.cons_hi[i] : -1;
    }
    return 0;
}

int grx_sm_set_option(grx_sm *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_sm_reset(grx_sm *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_sm_enact(grx_sm *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_sm_stats(grx_sm *p, long long *items, long long *regime_items, long long *candidates, long long *bisections, long long *occurrences,
                 long long *embeddings, long long *pairs, long long *longest_row, long long *kernel_launches, double *bound, double *kernel_ms,
                 double *bin_ms, double *group8_ms, double *wave_ms, double *finish_ms, double *build_ms)
{
    if (!p) return -1;
    SmStats s;
    p->runner->Stats(s);
    if (items) *items = s.items;
    if (regime_items) regime_items[0] = s.regime[0], regime_items[1] = s.regime[1];
    if (candidates) *candidates = s.streamed;
    if (bisections) *bisections = s.bisections;
    if (occurrences) *occurrences = s.occurrences;
    if (embeddings) *embeddings = s.embeddings;
    if (pairs) *pairs = s.pairs;
    if (longest_row) *longest_row = s.longest;
    if (kernel_launches) *kernel_launches = s.launches;
    if (bound) *bound = s.bound;
    if (kernel_ms) *kernel_ms = s.kernel_ms;
    double *kinds[MS_COUNT] = {bin_ms, group8_ms, wave_ms, finish_ms};
    for (int i = 0; i < MS_COUNT; ++i)
        if (kinds[i]) *kinds[i] = s.kind_ms[i];
    if (build_ms) *build_ms = s.build_ms;
    return 0;
}

int grx_sm_extract(grx_sm *p, long long *h_count, long long *occurrences, long long *embeddings)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_count, occurrences, embeddings));
}

int grx_sm_device_results(grx_sm *p, long long **d_count, int **d_degrees)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_count, d_degrees);
    return 0;
}

void grx_sm_destroy(grx_sm *p) { delete p; }

}  // extern "C"
