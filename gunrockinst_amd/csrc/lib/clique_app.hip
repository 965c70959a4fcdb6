// lib/clique_app.hip -- k-clique counting entry points of libgunrock.so.
//  * grx_clique_*: CliqueProblem / CliqueEnactor phases as separate C calls (the reference snapshot has no clique counting; the calls
//    are shaped like grx_tc_*).  Extract gives one 64-bit count per vertex and the total.
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/clique/clique_enactor.hpp>
#include <gunrock/app/clique/clique_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::clique;

static_assert(GRX_CLIQUE_AUTO == CLIQUE_AUTO && GRX_CLIQUE_BITMAP == CLIQUE_BITMAP && GRX_CLIQUE_LIST == CLIQUE_LIST,
              "the header's strategies are the kernels' strategies");
static_assert(GRX_CLIQUE_OVERFLOW == kCliqueOverflow, "the header's refusal is the enactor's");
static_assert(sizeof(long long) == sizeof(Count), "counts are 64-bit");

namespace {

struct CliqueStats {
    long long oriented = 0, longest = 0, rows[2] = {0, 0}, edges[2] = {0, 0}, bit_ands = 0, list_lookups = 0, launches = 0;
    double bound = 0, kernel_ms = 0, build_ms = 0;
};

struct CliqueRunner {
    InitState state;
    bool finished = false;  // the last Enact ran to its end: there is a result to extract
    virtual ~CliqueRunner() {}
    virtual int Init(const Csr<int, int, int> &g, const int *rank) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, const int *d_rank) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual int Enact(int k, int max_grid_size, float *ms) = 0;
    virtual void Stats(CliqueStats &s) = 0;
    virtual hipError_t Extract(long long *cliques, long long *total) = 0;
    virtual void DeviceResults(long long **d_cliques, int **d_degrees) = 0;
};

template <bool INSTR>
struct CliqueRunnerT : CliqueRunner {
    typedef CliqueProblem<false> Problem;
    Problem problem;
    CliqueEnactor<INSTR> enactor;
    EventPair timer;
    explicit CliqueRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g, const int *rank) override
    {
        const hipError_t rc = problem.Init(false, g, rank, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, const int *d_rank) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci, d_rank);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetOption(const char *name, double value) override
    {
        const long long v = static_cast<long long>(value);
        if (!std::strcmp(name, "strategy")) {
            if (v < CLIQUE_AUTO || v > CLIQUE_LIST) return -1;
            enactor.strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "bitmap_rows")) {
            if (v < kBitmapRowsMin || v > kBitmapRowsMax) return -1;
            enactor.bitmap_rows = static_cast<int>(v);
        } else if (!std::strcmp(name, "count_limit")) {
            if (!(value >= 1.0 && value <= kCountLimit)) return -1;
            enactor.count_limit = value;
        } else {
            return 1;
        }
        return 0;
    }
    hipError_t Reset() override
    {
        if (!state.ready) return hipErrorNotReady;
        finished = false;
        return problem.Reset();
    }
    int Enact(int k, int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        finished = false;
        const hipError_t rc = timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, k, max_grid_size); });
        if (rc) return static_cast<int>(rc);
        if (enactor.refused) return kCliqueOverflow;
        finished = true;
        return 0;
    }
    void Stats(CliqueStats &s) override
    {
        s.oriented = problem.oriented_edges;
        s.longest = problem.max_out_row;
        for (int i = 0; i < 2; ++i) {
            s.rows[i] = enactor.regime_rows[i];
            s.edges[i] = enactor.regime_edges[i];
        }
        s.bit_ands = enactor.bit_ands;
        s.list_lookups = enactor.list_lookups;
        s.launches = enactor.host.launches;
        s.bound = enactor.bound;
        s.kernel_ms = enactor.host.kernel_ms;
        s.build_ms = problem.build_ms;
    }
    hipError_t Extract(long long *cliques, long long *total) override
    {
        if (!state.ready || !finished) return hipErrorNotReady;
        const hipError_t rc = problem.Extract(cliques);
        if (total) *total = problem.total;
        return rc;
    }
    void DeviceResults(long long **d_cliques, int **d_degrees) override
    {
        if (d_cliques) *d_cliques = state.ready ? reinterpret_cast<long long *>(problem.data_slices[0]->d_cliques.p) : nullptr;
        if (d_degrees) *d_degrees = state.ready ? reinterpret_cast<int *>(problem.data_slices[0]->d_degrees.p) : nullptr;
    }
};

}  // namespace

struct grx_clique {
    std::unique_ptr<CliqueRunner> runner;
};

extern "C" {

int grx_clique_create(grx_clique **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_clique{MakeRunner<CliqueRunner, CliqueRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_clique_init(grx_clique *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *rank)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph, rank);
}

int grx_clique_init_device(grx_clique *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, const int *d_rank)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_rank);
}

int grx_clique_set_option(grx_clique *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_clique_reset(grx_clique *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_clique_enact(grx_clique *p, int k, int max_grid_size, float *elapsed_ms)
{
    if (!p || k < kMinK || k > kMaxK) return -1;
    return p->runner->Enact(k, max_grid_size, elapsed_ms);
}

int grx_clique_stats(grx_clique *p, long long *oriented_edges, long long *max_out_row, long long *regime_rows, long long *regime_edges,
                     long long *bit_ands, long long *list_lookups, double *bound, long long *kernel_launches, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    CliqueStats s;
    p->runner->Stats(s);
    if (oriented_edges) *oriented_edges = s.oriented;
    if (max_out_row) *max_out_row = s.longest;
    for (int i = 0; i < 2; ++i) {
        if (regime_rows) regime_rows[i] = s.rows[i];
        if (regime_edges) regime_edges[i] = s.edges[i];
    }
    if (bit_ands) *bit_ands = s.bit_ands;
    if (list_lookups) *list_lookups = s.list_lookups;
    if (bound) *bound = s.bound;
    if (kernel_launches) *kernel_launches = s.launches;
    if (kernel_ms) *kernel_ms = s.kernel_ms;
    if (build_ms) *build_ms = s.build_ms;
    return 0;
}

int grx_clique_extract(grx_clique *p, long long *h_cliques, long long *total)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_cliques, total));
}

int grx_clique_device_results(grx_clique *p, long long **d_cliques, int **d_degrees)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_cliques, d_degrees);
    return 0;
}

void grx_clique_destroy(grx_clique *p) { delete p; }

}  // extern "C"
