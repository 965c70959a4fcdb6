// lib/kcore_app.hip -- k-core decomposition entry points of libgunrock.so.
//  * grx_kcore_*: KcoreProblem / KcoreEnactor phases as separate C calls (the reference snapshot has no k-core; the calls are
//    shaped like grx_tc_*).  Extract gives one int32 core number per vertex and the degeneracy.
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/kcore/kcore_enactor.hpp>
#include <gunrock/app/kcore/kcore_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::kcore;

static_assert(GRX_KCORE_AUTO == KCORE_AUTO && GRX_KCORE_ROUNDS == KCORE_ROUNDS && GRX_KCORE_DEVICE_LOOP == KCORE_DEVICE_LOOP,
              "the header's schedules are the enactor's schedules");

namespace {

struct KcoreRunner {
    InitState state;
    virtual ~KcoreRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual hipError_t Enact(int k_limit, int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms, double &build_ms) = 0;
    virtual int LevelTrace(int max_levels, int *k, long long *vertices, double *ms) = 0;
    virtual hipError_t Extract(int *core, int *degeneracy) = 0;
    virtual hipError_t Shells(int max_entries, long long *sizes, int *count) = 0;
    virtual hipError_t Members(int k, unsigned char *mask, long long *vertices, long long *edges) = 0;
    virtual void DeviceResults(int **d_core, int **d_degrees) = 0;
};

template <bool INSTR>
struct KcoreRunnerT : KcoreRunner {
    typedef KcoreProblem<false> Problem;
    Problem problem;
    KcoreEnactor<INSTR> enactor;
    EventPair timer;
    explicit KcoreRunnerT(int device) : enactor(false)
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
        const int shared = enactor.loop.Set(name, value, KCORE_DEVICE_LOOP);
        if (shared != 1) return shared;
        if (std::strcmp(name, "compact_below")) return 1;
        if (!(value >= 0.0 && value <= 1.0)) return -1;
        enactor.compact_below = value;
        return 0;
    }
    hipError_t Reset() override { return state.ready ? problem.Reset() : hipErrorNotReady; }
    hipError_t Enact(int k_limit, int max_grid_size, float *ms) override
    {
        if (!state.ready) return hipErrorNotReady;
        return timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, k_limit, max_grid_size); });
    }
    void Stats(long long *out, double &kernel_ms, double &build_ms) override
    {
        out[0] = problem.simple_edges;
        out[1] = problem.max_degree;
        out[2] = enactor.levels;
        out[3] = enactor.rounds;
        out[4] = enactor.vertices_peeled;
        out[5] = enactor.entries_read;
        out[6] = enactor.compactions;
        out[7] = enactor.step.launches;
        kernel_ms = enactor.step.kernel_ms;
        build_ms = problem.build_ms;
    }
    int LevelTrace(int max_levels, int *k, long long *vertices, double *ms) override
    {
        return CopyTrace(enactor.trace_k.size(), max_levels, Column(k, [&](int i) { return enactor.trace_k[i]; }),
                         Column(vertices, [&](int i) { return enactor.trace_vertices[i]; }), Column(ms, [&](int i) { return enactor.trace_ms[i]; }));
    }
    hipError_t Extract(int *core, int *degeneracy) override
    {
        if (!state.ready) return hipErrorNotReady;
        const hipError_t rc = problem.Extract(core);
        if (degeneracy) *degeneracy = problem.degeneracy;
        return rc;
    }
    hipError_t Shells(int max_entries, long long *sizes, int *count) override
    {
        if (!state.ready) return hipErrorNotReady;
        return problem.Shells(max_entries, sizes, count);
    }
    hipError_t Members(int k, unsigned char *mask, long long *vertices, long long *edges) override
    {
        if (!state.ready) return hipErrorNotReady;
        return problem.Members(k, enactor.loop.wave_min_row, mask, vertices, edges);
    }
    void DeviceResults(int **d_core, int **d_degrees) override
    {
        if (d_core) *d_core = state.ready ? problem.data_slices[0]->d_core : nullptr;
        if (d_degrees) *d_degrees = state.ready ? problem.data_slices[0]->d_degrees : nullptr;
    }
};

}  // namespace

struct grx_kcore {
    std::unique_ptr<KcoreRunner> runner;
};

extern "C" {

int grx_kcore_create(grx_kcore **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_kcore{MakeRunner<KcoreRunner, KcoreRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_kcore_init(grx_kcore *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_kcore_init_device(grx_kcore *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices);
}

int grx_kcore_set_option(grx_kcore *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_kcore_reset(grx_kcore *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_kcore_enact(grx_kcore *p, int k_limit, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Enact(k_limit, max_grid_size, elapsed_ms));
}

int grx_kcore_stats(grx_kcore *p, long long *simple_edges, long long *max_degree, long long *levels, long long *rounds,
                    long long *vertices_peeled, long long *entries_read, long long *compactions, long long *kernel_launches, double *kernel_ms,
                    double *build_ms)
{
    if (!p) return -1;
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double k = 0, b = 0;
    p->runner->Stats(v, k, b);
    long long *out[8] = {simple_edges, max_degree, levels, rounds, vertices_peeled, entries_read, compactions, kernel_launches};
    for (int i = 0; i < 8; ++i)
        if (out[i]) *out[i] = v[i];
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_kcore_level_trace(grx_kcore *p, int max_levels, int *k, long long *vertices, double *ms)
{
    if (!p) return -1;
    return p->runner->LevelTrace(max_levels, k, vertices, ms);
}

int grx_kcore_extract(grx_kcore *p, int *h_core, int *degeneracy)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_core, degeneracy));
}

int grx_kcore_shells(grx_kcore *p, int max_entries, long long *h_sizes)
{
    if (!p) return -1;
    int count = 0;
    const hipError_t rc = p->runner->Shells(max_entries, h_sizes, &count);
    return rc ? -static_cast<int>(rc) : count;
}

int grx_kcore_members(grx_kcore *p, int k, unsigned char *h_mask, long long *vertices, long long *edges)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Members(k, h_mask, vertices, edges));
}

int grx_kcore_device_results(grx_kcore *p, int **d_core, int **d_degrees)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_core, d_degrees);
    return 0;
}

void grx_kcore_destroy(grx_kcore *p) { delete p; }

}  // extern "C"
