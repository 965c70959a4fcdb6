// lib/mst_app.hip -- minimum spanning forest entry points of libgunrock.so.
//  * grx_mst_*: MSTProblem / MSTEnactor phases as separate C calls (the reference has no C entry point for MST; its driver is
//    tests/mst/test_mst.cu).  Extract follows MSTProblem::Extract(h_mst_output) (mst_problem.cuh:218): a 0/1 flag per CSR entry.
#include <gunrock/gunrock_mi355x.h>

#include <vector>

#include <gunrock/app/mst/mst_enactor.hpp>
#include <gunrock/app/mst/mst_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::mst;

namespace {

struct MstRunner {
    InitState state;  // (MST reads `state.ready` only: its handle may be initialised again)
    virtual ~MstRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_w) = 0;
    virtual hipError_t Reset() = 0;
    virtual hipError_t Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long &rounds, long long &scanned, long long &launches, double &kernel_ms) = 0;
    virtual int Trace(int max_rounds, long long *entries, double *ms) = 0;
    virtual hipError_t Extract(int *selected, long long *total_weight, int *forest_edges) = 0;
    virtual int *DeviceSelected() = 0;
};

template <bool INSTR>
struct MstRunnerT : MstRunner {
    typedef MSTProblem<true> Problem;
    Problem problem;
    MSTEnactor<INSTR> enactor;
    EventPair timer;
    explicit MstRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g) override
    {
        const hipError_t rc = problem.Init(false, g, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_w) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci, d_w);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    hipError_t Reset() override { return state.ready ? problem.Reset() : hipErrorNotReady; }
    hipError_t Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return hipErrorNotReady;
        return timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
    }
    void Stats(long long &rounds, long long &scanned, long long &launches, double &kernel_ms) override
    {
        rounds = enactor.rounds;
        scanned = enactor.edges_scanned;
        launches = enactor.launches;
        kernel_ms = enactor.kernel_ms;
    }
    int Trace(int max_rounds, long long *entries, double *ms) override
    {
        return CopyTrace(enactor.trace.size(), max_rounds, Column(entries, [&](int i) { return enactor.trace[i].entries; }),
                         Column(ms, [&](int i) { return enactor.trace[i].ms; }));
    }
    hipError_t Extract(int *selected, long long *total_weight, int *forest_edges) override
    {
        if (!state.ready) return hipErrorNotReady;
        const hipError_t rc = problem.Extract(selected);
        if (total_weight) *total_weight = problem.total_weight;
        if (forest_edges) *forest_edges = static_cast<int>(problem.forest_edges);
        return rc;
    }
    int *DeviceSelected() override { return state.ready ? problem.data_slices[0]->d_selected : nullptr; }
};

}  // namespace

struct grx_mst {
    std::unique_ptr<MstRunner> runner;
};

extern "C" {

int grx_mst_create(grx_mst **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_mst{MakeRunner<MstRunner, MstRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_mst_init(grx_mst *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *edge_values)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && (!col_indices || !edge_values)) return -1;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices, edge_values);
    return p->runner->Init(wrap.graph);
}

int grx_mst_init_device(grx_mst *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_edge_values)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && (!d_col_indices || !d_edge_values)) return -1;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_edge_values);
}

int grx_mst_reset(grx_mst *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_mst_enact(grx_mst *p, int max_grid_size, float *elapsed_ms)
{
    return p ? static_cast<int>(p->runner->Enact(max_grid_size, elapsed_ms)) : -1;
}

int grx_mst_stats(grx_mst *p, long long *rounds, long long *edges_scanned, long long *kernel_launches, double *kernel_ms)
{
    if (!p) return -1;
    long long r = 0, s = 0, l = 0;
    double k = 0;
    p->runner->Stats(r, s, l, k);
    if (rounds) *rounds = r;
    if (edges_scanned) *edges_scanned = s;
    if (kernel_launches) *kernel_launches = l;
    if (kernel_ms) *kernel_ms = k;
    return 0;
}

int grx_mst_round_trace(grx_mst *p, int max_rounds, long long *entries, double *ms)
{
    if (!p || max_rounds < 0) return -1;
    return p->runner->Trace(max_rounds, entries, ms);
}

int grx_mst_extract(grx_mst *p, int *h_selected, long long *total_weight, int *forest_edges)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_selected, total_weight, forest_edges));
}

int grx_mst_device_results(grx_mst *p, int **d_selected)
{
    if (!p || !d_selected) return -1;
    *d_selected = p->runner->DeviceSelected();
    return 0;
}

void grx_mst_destroy(grx_mst *p) { delete p; }

}  // extern "C"
