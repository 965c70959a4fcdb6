// lib/truss_app.hip -- per-edge triangle support and k-truss entry points of libgunrock.so.
//  * grx_truss_*: TrussProblem / TrussEnactor phases as separate C calls (the reference snapshot has no k-truss; the calls are
//    shaped like grx_kcore_*).  Every per-edge array is indexed by the canonical edge id (grx_truss_edges).
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/truss/truss_enactor.hpp>
#include <gunrock/app/truss/truss_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::truss;

static_assert(GRX_TRUSS_AUTO == TRUSS_AUTO && GRX_TRUSS_ROUNDS == TRUSS_ROUNDS, "the header's schedules are the enactor's schedules");

namespace {

struct TrussRunner {
    InitState state;
    virtual ~TrussRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual hipError_t Enact(int k_limit, int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double *ms) = 0;
    virtual int LevelTrace(int max_levels, int *k, long long *edges, double *ms) = 0;
    virtual hipError_t Edges(int *src, int *dst, long long *count) = 0;
    virtual hipError_t Support(int *support, long long *total) = 0;
    virtual hipError_t Extract(int *truss, int *max_truss) = 0;
    virtual hipError_t Classes(int max_entries, long long *sizes, int *count) = 0;
    virtual hipError_t Members(int k, unsigned char *mask, long long *edges, long long *vertices) = 0;
    virtual hipError_t VertexTruss(int *out) = 0;
    virtual void DeviceResults(int **d_truss, int **d_support, int **d_src, int **d_dst) = 0;
};

template <bool INSTR>
struct TrussRunnerT : TrussRunner {
    typedef TrussProblem<false> Problem;
    Problem problem;
    TrussEnactor<INSTR> enactor;
    EventPair timer;
    explicit TrussRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g) override
    {
        problem.wave_min_row = enactor.loop.wave_min_row;
        const hipError_t rc = problem.Init(false, g, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) override
    {
        problem.wave_min_row = enactor.loop.wave_min_row;
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetOption(const char *name, double value) override
    {
        return enactor.loop.Set(name, value, TRUSS_ROUNDS);  // (no option of its own, and no DEVICE_LOOP schedule)
    }
    hipError_t Reset() override { return state.ready ? problem.Reset() : hipErrorNotReady; }
    hipError_t Enact(int k_limit, int max_grid_size, float *ms) override
    {
        if (!state.ready) return hipErrorNotReady;
        return timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, k_limit, max_grid_size); });
    }
    void Stats(long long *out, double *ms) override
    {
        out[0] = problem.simple_edges;
        out[1] = problem.triangles;
        out[2] = problem.max_support;
        out[3] = enactor.levels;
        out[4] = enactor.rounds;
        out[5] = enactor.edges_peeled;
        out[6] = problem.support_entries;
        out[7] = enactor.entries_read;
        out[8] = enactor.step.launches;
        out[9] = enactor.step.readbacks;
        ms[0] = enactor.step.kernel_ms;
        ms[1] = problem.build_ms;
        ms[2] = problem.support_ms;
    }
    int LevelTrace(int max_levels, int *k, long long *edges, double *ms) override
    {
        return CopyTrace(enactor.trace_k.size(), max_levels, Column(k, [&](int i) { return enactor.trace_k[i]; }),
                         Column(edges, [&](int i) { return enactor.trace_edges[i]; }), Column(ms, [&](int i) { return enactor.trace_ms[i]; }));
    }
    hipError_t Edges(int *src, int *dst, long long *count) override
    {
        if (!state.ready) return hipErrorNotReady;
        *count = problem.simple_edges;
        return problem.Edges(src, dst);
    }
    hipError_t Support(int *support, long long *total) override
    {
        if (!state.ready) return hipErrorNotReady;
        if (total) *total = problem.triangles;
        return problem.Support(support);
    }
    hipError_t Extract(int *truss_out, int *max_truss) override
    {
        if (!state.ready || !problem.enacted) return hipErrorNotReady;
        const hipError_t rc = problem.Extract(truss_out);
        if (max_truss) *max_truss = problem.max_truss;
        return rc;
    }
    hipError_t Classes(int max_entries, long long *sizes, int *count) override
    {
        if (!state.ready || !problem.enacted) return hipErrorNotReady;
        return problem.Classes(max_entries, sizes, count);
    }
    hipError_t Members(int k, unsigned char *mask, long long *edges, long long *vertices) override
    {
        if (!state.ready || !problem.enacted) return hipErrorNotReady;
        return problem.Members(k, mask, edges, vertices);
    }
    hipError_t VertexTruss(int *out) override
    {
        if (!state.ready || !problem.enacted) return hipErrorNotReady;
        return problem.VertexTruss(out);
    }
    void DeviceResults(int **d_truss, int **d_support, int **d_src, int **d_dst) override
    {
        typename Problem::DataSlice *ds = state.ready ? problem.data_slices[0] : nullptr;
        if (d_truss) *d_truss = ds ? ds->d_truss : nullptr;
        if (d_support) *d_support = ds ? ds->d_support : nullptr;
        if (d_src) *d_src = ds ? ds->d_src : nullptr;
        if (d_dst) *d_dst = ds ? ds->d_dst : nullptr;
    }
};

}  // namespace

struct grx_truss {
    std::unique_ptr<TrussRunner> runner;
};

extern "C" {

int grx_truss_create(grx_truss **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_truss{MakeRunner<TrussRunner, TrussRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_truss_init(grx_truss *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_truss_init_device(grx_truss *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices);
}

int grx_truss_set_option(grx_truss *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_truss_reset(grx_truss *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_truss_enact(grx_truss *p, int k_limit, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Enact(k_limit, max_grid_size, elapsed_ms));
}

int grx_truss_stats(grx_truss *p, long long *simple_edges, long long *triangles, long long *max_support, long long *levels, long long *rounds,
                    long long *edges_peeled, long long *support_entries, long long *peel_entries, long long *kernel_launches,
                    long long *readbacks, double *kernel_ms, double *build_ms, double *support_ms)
{
    if (!p) return -1;
    long long v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double ms[3] = {0, 0, 0};
    p->runner->Stats(v, ms);
    long long *out[10] = {simple_edges, triangles, max_support, levels, rounds, edges_peeled, support_entries, peel_entries, kernel_launches,
                          readbacks};
    for (int i = 0; i < 10; ++i)
        if (out[i]) *out[i] = v[i];
    if (kernel_ms) *kernel_ms = ms[0];
    if (build_ms) *build_ms = ms[1];
    if (support_ms) *support_ms = ms[2];
    return 0;
}

int grx_truss_level_trace(grx_truss *p, int max_levels, int *k, long long *edges, double *ms)
{
    if (!p) return -1;
    return p->runner->LevelTrace(max_levels, k, edges, ms);
}

int grx_truss_edges(grx_truss *p, int *h_src, int *h_dst)
{
    if (!p) return -1;
    long long count = 0;  // M <= the entries of the CSR: an int
    const hipError_t rc = p->runner->Edges(h_src, h_dst, &count);
    return rc ? -static_cast<int>(rc) : static_cast<int>(count);
}

int grx_truss_support(grx_truss *p, int *h_support, long long *total_triangles)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Support(h_support, total_triangles));
}

int grx_truss_extract(grx_truss *p, int *h_truss, int *max_truss)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_truss, max_truss));
}

int grx_truss_classes(grx_truss *p, int max_entries, long long *h_sizes)
{
    if (!p) return -1;
    int count = 0;
    const hipError_t rc = p->runner->Classes(max_entries, h_sizes, &count);
    return rc ? -static_cast<int>(rc) : count;
}

int grx_truss_members(grx_truss *p, int k, unsigned char *h_mask, long long *edges, long long *vertices)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Members(k, h_mask, edges, vertices));
}

int grx_truss_vertex_truss(grx_truss *p, int *h_vertex_truss)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->VertexTruss(h_vertex_truss));
}

int grx_truss_device_results(grx_truss *p, int **d_truss, int **d_support, int **d_src, int **d_dst)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_truss, d_support, d_src, d_dst);
    return 0;
}

void grx_truss_destroy(grx_truss *p) { delete p; }

}  // extern "C"
