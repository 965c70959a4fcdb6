// lib/c4_app.hip -- 4-cycle (butterfly) counting entry points of libgunrock.so.
//  * grx_c4_*: C4Problem / C4Enactor phases as separate C calls (the reference snapshot has no 4-cycle counting; the calls are
//    shaped like grx_clique_*, the per-edge ones like grx_truss_*).  Extract gives one 64-bit count per vertex and the total,
//    extract_edges one per canonical pair.
#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/c4/c4_enactor.hpp>
#include <gunrock/app/c4/c4_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::c4;

static_assert(GRX_C4_AUTO == C4_AUTO && GRX_C4_LANE == C4_LANE && GRX_C4_WAVE == C4_WAVE && GRX_C4_BLOCK == C4_BLOCK && GRX_C4_GLOBAL == C4_GLOBAL,
              "the header's strategies are the kernels' strategies");
static_assert(GRX_C4_OVERFLOW == kC4Overflow, "the header's refusal is the enactor's");
static_assert(sizeof(long long) == sizeof(Count), "counts are 64-bit");

namespace {

struct C4Stats {
    long long simple_edges = 0, wedges = 0, vertices[4] = {0, 0, 0, 0}, regime_wedges[4] = {0, 0, 0, 0}, probes = 0, launches = 0;
    double bound = 0, kernel_ms = 0, build_ms = 0;
};

struct C4Runner {
    InitState state;
    bool finished = false;  // the last Enact ran to its end: there is a result to extract
    virtual ~C4Runner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(C4Stats &s) = 0;
    virtual hipError_t Extract(long long *cycles, long long *total) = 0;
    virtual hipError_t Edges(int *src, int *dst, long long *count) = 0;
    virtual int ExtractEdges(long long *edge_cycles) = 0;
    virtual void DeviceResults(long long **d_cycles, long long **d_edge_cycles, int **d_src, int **d_dst) = 0;
};

template <bool INSTR>
struct C4RunnerT : C4Runner {
    typedef C4Problem<false> Problem;
    Problem problem;
    C4Enactor<INSTR> enactor;
    EventPair timer;
    explicit C4RunnerT(int device) : enactor(false)
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
        finished = false;
        return problem.Reset();
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        finished = false;
        const hipError_t rc = timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
        if (rc) return static_cast<int>(rc);
        if (enactor.refused) return kC4Overflow;
        finished = true;
        return 0;
    }
    void Stats(C4Stats &s) override
    {
        s.simple_edges = problem.simple_edges;
        s.wedges = problem.wedges;
        for (int i = 0; i < 4; ++i) {
            s.vertices[i] = enactor.regime_vertices[i];
            s.regime_wedges[i] = enactor.regime_wedges[i];
        }
        s.probes = enactor.probes;
        s.launches = enactor.host.launches;
        s.bound = state.ready ? problem.bound : 0;
        s.kernel_ms = enactor.host.kernel_ms;
        s.build_ms = problem.build_ms;
    }
    hipError_t Extract(long long *cycles, long long *total) override
    {
        if (!state.ready || !finished) return hipErrorNotReady;
        const hipError_t rc = problem.Extract(cycles);
        if (total) *total = problem.total;
        return rc;
    }
    hipError_t Edges(int *src, int *dst, long long *count) override
    {
        if (!state.ready) return hipErrorNotReady;
        *count = problem.simple_edges;
        return problem.Edges(src, dst);
    }
    int ExtractEdges(long long *edge_cycles) override
    {
        if (!state.ready || !finished) return static_cast<int>(hipErrorNotReady);
        if (!enactor.with_edges) return -1;
        return static_cast<int>(problem.ExtractEdges(edge_cycles));
    }
    void DeviceResults(long long **d_cycles, long long **d_edge_cycles, int **d_src, int **d_dst) override
    {
        typename Problem::DataSlice *ds = state.ready ? problem.data_slices[0] : nullptr;
        if (d_cycles) *d_cycles = ds ? reinterpret_cast<long long *>(ds->d_cycles.p) : nullptr;
        if (d_edge_cycles) *d_edge_cycles = ds && finished && enactor.with_edges ? reinterpret_cast<long long *>(ds->d_edge_cycles.p) : nullptr;
        if (d_src) *d_src = ds ? ds->d_src : nullptr;
        if (d_dst) *d_dst = ds ? ds->d_dst : nullptr;
    }
};

}  // namespace

struct grx_c4 {
    std::unique_ptr<C4Runner> runner;
};

extern "C" {

int grx_c4_create(grx_c4 **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_c4{MakeRunner<C4Runner, C4RunnerT>(instrument != 0, device)};
    return 0;
}

int grx_c4_init(grx_c4 *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_c4_init_device(grx_c4 *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices);
}

int grx_c4_set_option(grx_c4 *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_c4_reset(grx_c4 *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_c4_enact(grx_c4 *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_c4_stats(grx_c4 *p, long long *simple_edges, long long *wedges, long long *regime_vertices, long long *regime_wedges, long long *table_probes,
                 double *bound, long long *kernel_launches, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    C4Stats s;
    p->runner->Stats(s);
    if (simple_edges) *simple_edges = s.simple_edges;
    if (wedges) *wedges = s.wedges;
    for (int i = 0; i < 4; ++i) {
        if (regime_vertices) regime_vertices[i] = s.vertices[i];
        if (regime_wedges) regime_wedges[i] = s.regime_wedges[i];
    }
    if (table_probes) *table_probes = s.probes;
    if (bound) *bound = s.bound;
    if (kernel_launches) *kernel_launches = s.launches;
    if (kernel_ms) *kernel_ms = s.kernel_ms;
    if (build_ms) *build_ms = s.build_ms;
    return 0;
}

int grx_c4_extract(grx_c4 *p, long long *h_cycles, long long *total)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_cycles, total));
}

int grx_c4_edges(grx_c4 *p, int *h_src, int *h_dst)
{
    if (!p) return -1;
    long long count = 0;  // M <= the entries of the CSR: an int
    const hipError_t rc = p->runner->Edges(h_src, h_dst, &count);
    return rc ? -static_cast<int>(rc) : static_cast<int>(count);
}

int grx_c4_extract_edges(grx_c4 *p, long long *h_edge_cycles)
{
    if (!p) return -1;
    return p->runner->ExtractEdges(h_edge_cycles);
}

int grx_c4_device_results(grx_c4 *p, long long **d_cycles, long long **d_edge_cycles, int **d_src, int **d_dst)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_cycles, d_edge_cycles, d_src, d_dst);
    return 0;
}

void grx_c4_destroy(grx_c4 *p) { delete p; }

}  // extern "C"
