// lib/tc_app.hip -- triangle counting / clustering coefficient entry points of libgunrock.so.
//  * grx_tc_*: TCProblem / TCEnactor phases as separate C calls (the reference snapshot has no TC; the calls are shaped like
//    grx_mis_*).  Extract gives one 64-bit count per vertex and the total.
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/tc/tc_enactor.hpp>
#include <gunrock/app/tc/tc_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::tc;

static_assert(GRX_TC_AUTO == TC_AUTO && GRX_TC_LANE == TC_LANE && GRX_TC_LDS == TC_LDS && GRX_TC_GLOBAL == TC_GLOBAL,
              "the header's strategies are the kernels' strategies");
static_assert(sizeof(long long) == sizeof(Count), "counts are 64-bit");

namespace {

struct TcRunner {
    InitState state;
    virtual ~TcRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual hipError_t Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long &oriented, long long &longest, long long &probed, long long &launches, long long *regime_rows, double &kernel_ms,
                       double &build_ms) = 0;
    virtual hipError_t Extract(long long *triangles, long long *total) = 0;
    virtual hipError_t Clustering(double *coeff, double *transitivity) = 0;
    virtual void DeviceResults(long long **d_triangles, int **d_degrees) = 0;
};

template <bool INSTR>
struct TcRunnerT : TcRunner {
    typedef TCProblem<false> Problem;
    Problem problem;
    TCEnactor<INSTR> enactor;
    EventPair timer;
    explicit TcRunnerT(int device) : enactor(false)
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
    int SetOption(const char *name, double value) override
    {
        const long long v = static_cast<long long>(value);
        if (!std::strcmp(name, "strategy")) {
            if (v < TC_AUTO || v > TC_GLOBAL) return -1;
            enactor.strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "lds_entries")) {
            if (v < 1) return -1;
            enactor.lds_entries = static_cast<int>(v < kLdsEntriesMax ? v : kLdsEntriesMax);
        } else if (!std::strcmp(name, "lane_max_row")) {
            if (v < 0) return -1;
            enactor.lane_max_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else {
            return 1;
        }
        return 0;
    }
    hipError_t Reset() override { return state.ready ? problem.Reset() : hipErrorNotReady; }
    hipError_t Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return hipErrorNotReady;
        return timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
    }
    void Stats(long long &oriented, long long &longest, long long &probed, long long &launches, long long *regime_rows, double &kernel_ms,
               double &build_ms) override
    {
        oriented = problem.oriented_edges;
        longest = problem.max_out_row;
        probed = enactor.entries_probed;
        launches = enactor.host.launches;
        if (regime_rows)
            for (int i = 0; i < 3; ++i) regime_rows[i] = enactor.regime_rows[i];
        kernel_ms = enactor.host.kernel_ms;
        build_ms = problem.build_ms;
    }
    hipError_t Extract(long long *triangles, long long *total) override
    {
        if (!state.ready) return hipErrorNotReady;
        const hipError_t rc = problem.Extract(triangles);
        if (total) *total = problem.total;
        return rc;
    }
    hipError_t Clustering(double *coeff, double *transitivity) override
    {
        if (!state.ready) return hipErrorNotReady;
        return problem.Clustering(coeff, transitivity);
    }
    void DeviceResults(long long **d_triangles, int **d_degrees) override
    {
        if (d_triangles) *d_triangles = state.ready ? reinterpret_cast<long long *>(problem.data_slices[0]->d_triangles.p) : nullptr;
        if (d_degrees) *d_degrees = state.ready ? reinterpret_cast<int *>(problem.data_slices[0]->d_degrees.p) : nullptr;
    }
};

}  // namespace

struct grx_tc {
    std::unique_ptr<TcRunner> runner;
};

extern "C" {

int grx_tc_create(grx_tc **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_tc{MakeRunner<TcRunner, TcRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_tc_init(grx_tc *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_tc_init_device(grx_tc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices);
}

int grx_tc_set_option(grx_tc *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_tc_reset(grx_tc *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_tc_enact(grx_tc *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Enact(max_grid_size, elapsed_ms));
}

int grx_tc_stats(grx_tc *p, long long *oriented_edges, long long *max_out_row, long long *entries_probed, long long *kernel_launches,
                 long long *regime_rows, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    long long o = 0, r = 0, e = 0, l = 0;
    double k = 0, b = 0;
    p->runner->Stats(o, r, e, l, regime_rows, k, b);
    if (oriented_edges) *oriented_edges = o;
    if (max_out_row) *max_out_row = r;
    if (entries_probed) *entries_probed = e;
    if (kernel_launches) *kernel_launches = l;
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_tc_extract(grx_tc *p, long long *h_triangles, long long *total)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_triangles, total));
}

int grx_tc_clustering(grx_tc *p, double *h_coeff, double *transitivity)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Clustering(h_coeff, transitivity));
}

int grx_tc_device_results(grx_tc *p, long long **d_triangles, int **d_degrees)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_triangles, d_degrees);
    return 0;
}

void grx_tc_destroy(grx_tc *p) { delete p; }

}  // extern "C"
