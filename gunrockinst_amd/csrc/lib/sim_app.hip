// lib/sim_app.hip -- vertex-similarity entry points of libgunrock.so.
//  * grx_sim_*: SimProblem / SimEnactor phases as separate C calls (the reference snapshot has no similarity; the calls are shaped
//    like grx_c4_*).  Two Enacts on one handle: pairs / pairs_device score given pairs, topk / topk_device give the k most similar
//    vertices of given sources; each has its extract.
#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/sim/sim_enactor.hpp>
#include <gunrock/app/sim/sim_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::sim;

static_assert(GRX_SIM_AUTO == SIM_AUTO && GRX_SIM_LANE == SIM_LANE && GRX_SIM_WAVE == SIM_WAVE && GRX_SIM_BLOCK == SIM_BLOCK && GRX_SIM_GLOBAL == SIM_GLOBAL,
              "the header's strategies are the kernels' strategies");
static_assert(GRX_SIM_COMMON == SIM_COMMON && GRX_SIM_JACCARD == SIM_JACCARD && GRX_SIM_OVERLAP == SIM_OVERLAP && GRX_SIM_SORENSEN == SIM_SORENSEN,
              "the header's metrics are the kernels' metrics");
static_assert(GRX_SIM_TOO_LARGE == kSimTooLarge && GRX_SIM_MAX_K == kMaxK, "the header's refusal and cap are the enactor's");

namespace {

struct SimStats {
    long long simple_edges = 0, wedges = 0, walked = 0, pairs[2] = {0, 0}, sources[3] = {0, 0, 0}, regime_wedges[3] = {0, 0, 0}, candidates = 0,
              probes = 0, launches = 0;
    double kernel_ms = 0, build_ms = 0;
};

struct SimRunner {
    InitState state;
    virtual ~SimRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual int Pairs(long long pairs, const int *u, const int *v, bool on_device, int max_grid_size, float *ms) = 0;
    virtual int Topk(long long sources, const int *ids, bool on_device, int k, int max_grid_size, float *ms) = 0;
    virtual void Stats(SimStats &s) = 0;
    virtual hipError_t ExtractPairs(int *common, long long *num, long long *den, double *score) = 0;
    virtual hipError_t ExtractTopk(int *ids, int *common, long long *num, long long *den, double *score, int *count, int *candidates) = 0;
    virtual void DeviceResults(int **pair_common, long long **pair_num, long long **pair_den, int **ids, int **common, long long **num, long long **den,
                               int **count, int **candidates) = 0;
};

template <bool INSTR>
struct SimRunnerT : SimRunner {
    typedef SimProblem<false> Problem;
    Problem problem;
    SimEnactor<INSTR> enactor;
    EventPair timer;
    explicit SimRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g) override
    {
        const hipError_t rc = problem.Init(false, g, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetOption(const char *name, double value) override { return enactor.options.Set(name, value); }
    hipError_t Reset() override
    {
        if (!state.ready) return hipErrorNotReady;
        return problem.Reset();
    }
    // what an Enact left: a HIP error, the refusal, a bad id, or 0
    int Code(hipError_t rc) const
    {
        if (rc) return static_cast<int>(rc);
        if (enactor.refused) return kSimTooLarge;
        return enactor.bad_id ? -1 : 0;
    }
    int Pairs(long long pairs, const int *u, const int *v, bool on_device, int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        problem.pairs = -1;
        if (!on_device && pairs > 0 && SimOptions::PairsFit(pairs)) {
            if (hipError_t rc = problem.Stage(pairs, u, v)) return static_cast<int>(rc);
            u = problem.data_slices[0]->staged_u.p;
            v = problem.data_slices[0]->staged_v.p;
        }
        return Code(timer.Timed(problem.graph_slices[0]->stream, ms,
                                [&]() { return enactor.template EnactPairs<Problem>(&problem, pairs, u, v, max_grid_size); }));
    }
    int Topk(long long sources, const int *ids, bool on_device, int k, int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        problem.sources = -1;
        if (!on_device && sources > 0 && SimOptions::TopkFits(sources, k)) {
            if (hipError_t rc = problem.Stage(sources, ids, nullptr)) return static_cast<int>(rc);
            ids = problem.data_slices[0]->staged_u.p;
        }
        return Code(timer.Timed(problem.graph_slices[0]->stream, ms,
                                [&]() { return enactor.template EnactTopk<Problem>(&problem, sources, ids, k, max_grid_size); }));
    }
    void Stats(SimStats &s) override
    {
        s.simple_edges = problem.simple_edges;
        s.wedges = problem.wedges;
        s.walked = enactor.walked;
        for (int i = 0; i < 2; ++i) s.pairs[i] = enactor.regime_pairs[i];
        for (int i = 0; i < 3; ++i) {
            s.sources[i] = enactor.regime_sources[i];
            s.regime_wedges[i] = enactor.regime_wedges[i];
        }
        s.candidates = enactor.candidates;
        s.probes = enactor.probes;
        s.launches = enactor.host.launches;
        s.kernel_ms = enactor.host.kernel_ms;
        s.build_ms = problem.build_ms;
    }
    hipError_t ExtractPairs(int *common, long long *num, long long *den, double *score) override
    {
        if (!state.ready || problem.pairs < 0) return hipErrorNotReady;
        return problem.ExtractPairs(common, num, den, score);
    }
    hipError_t ExtractTopk(int *ids, int *common, long long *num, long long *den, double *score, int *count, int *candidates) override
    {
        if (!state.ready || problem.sources < 0) return hipErrorNotReady;
        return problem.ExtractTopk(ids, common, num, den, score, count, candidates);
    }
    void DeviceResults(int **pair_common, long long **pair_num, long long **pair_den, int **ids, int **common, long long **num, long long **den,
                       int **count, int **candidates) override
    {
        typename Problem::DataSlice *ds = state.ready ? problem.data_slices[0] : nullptr;
        const bool pairs = ds && problem.pairs > 0, topk = ds && problem.sources > 0;
        if (pair_common) *pair_common = pairs ? ds->pair_common.p : nullptr;
        if (pair_num) *pair_num = pairs ? ds->pair_num.p : nullptr;
        if (pair_den) *pair_den = pairs ? ds->pair_den.p : nullptr;
        if (ids) *ids = topk ? ds->ids.p : nullptr;
        if (common) *common = topk ? ds->common.p : nullptr;
        if (num) *num = topk ? ds->num.p : nullptr;
        if (den) *den = topk ? ds->den.p : nullptr;
        if (count) *count = topk ? ds->count.p : nullptr;
        if (candidates) *candidates = topk ? ds->candidates.p : nullptr;
    }
};

}  // namespace

struct grx_sim {
    std::unique_ptr<SimRunner> runner;
};

extern "C" {

int grx_sim_create(grx_sim **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_sim{MakeRunner<SimRunner, SimRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_sim_init(grx_sim *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_sim_init_device(grx_sim *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices);
}

int grx_sim_set_option(grx_sim *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_sim_reset(grx_sim *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_sim_pairs(grx_sim *p, long long num_pairs, const int *h_u, const int *h_v, int max_grid_size, float *elapsed_ms)
{
    if (!p || num_pairs < 0 || (num_pairs > 0 && (!h_u || !h_v))) return -1;
    return p->runner->Pairs(num_pairs, h_u, h_v, false, max_grid_size, elapsed_ms);
}

int grx_sim_pairs_device(grx_sim *p, long long num_pairs, const int *d_u, const int *d_v, int max_grid_size, float *elapsed_ms)
{
    if (!p || num_pairs < 0 || (num_pairs > 0 && (!d_u || !d_v))) return -1;
    return p->runner->Pairs(num_pairs, d_u, d_v, true, max_grid_size, elapsed_ms);
}

int grx_sim_topk(grx_sim *p, long long num_sources, const int *h_sources, int k, int max_grid_size, float *elapsed_ms)
{
    if (!p || num_sources < 0 || (num_sources > 0 && !h_sources) || !SimOptions::ValidK(k)) return -1;
    return p->runner->Topk(num_sources, h_sources, false, k, max_grid_size, elapsed_ms);
}

int grx_sim_topk_device(grx_sim *p, long long num_sources, const int *d_sources, int k, int max_grid_size, float *elapsed_ms)
{
    if (!p || num_sources < 0 || (num_sources > 0 && !d_sources) || !SimOptions::ValidK(k)) return -1;
    return p->runner->Topk(num_sources, d_sources, true, k, max_grid_size, elapsed_ms);
}

int grx_sim_stats(grx_sim *p, long long *simple_edges, long long *wedges, long long *wedges_walked, long long *regime_pairs, long long *regime_sources,
                  long long *regime_wedges, long long *candidates, long long *table_probes, long long *kernel_launches, double *kernel_ms,
                  double *build_ms)
{
    if (!p) return -1;
    SimStats s;
    p->runner->Stats(s);
    if (simple_edges) *simple_edges = s.simple_edges;
    if (wedges) *wedges = s.wedges;
    if (wedges_walked) *wedges_walked = s.walked;
    for (int i = 0; i < 2; ++i)
        if (regime_pairs) regime_pairs[i] = s.pairs[i];
    for (int i = 0; i < 3; ++i) {
        if (regime_sources) regime_sources[i] = s.sources[i];
        if (regime_wedges) regime_wedges[i] = s.regime_wedges[i];
    }
    if (candidates) *candidates = s.candidates;
    if (table_probes) *table_probes = s.probes;
    if (kernel_launches) *kernel_launches = s.launches;
    if (kernel_ms) *kernel_ms = s.kernel_ms;
    if (build_ms) *build_ms = s.build_ms;
    return 0;
}

int grx_sim_extract_pairs(grx_sim *p, int *h_common, long long *h_num, long long *h_den, double *h_score)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->ExtractPairs(h_common, h_num, h_den, h_score));
}

int grx_sim_extract_topk(grx_sim *p, int *h_ids, int *h_common, long long *h_num, long long *h_den, double *h_score, int *h_count, int *h_candidates)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->ExtractTopk(h_ids, h_common, h_num, h_den, h_score, h_count, h_candidates));
}

int grx_sim_device_results(grx_sim *p, int **d_pair_common, long long **d_pair_num, long long **d_pair_den, int **d_ids, int **d_common,
                           long long **d_num, long long **d_den, int **d_count, int **d_candidates)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_pair_common, d_pair_num, d_pair_den, d_ids, d_common, d_num, d_den, d_count, d_candidates);
    return 0;
}

void grx_sim_destroy(grx_sim *p) { delete p; }

}  // extern "C"
