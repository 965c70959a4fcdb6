// lib/scc_app.hip -- strongly connected components entry points of libgunrock.so.
//  * grx_scc_*: SccProblem / SccEnactor phases as separate C calls (the reference snapshot has no SCC; the calls are shaped like
//    grx_kcore_*).  Extract gives one int32 per vertex, the smallest id of its component, and the number of components.
#include <gunrock/gunrock_mi355x.h>

#include <climits>
#include <cstring>

#include <gunrock/app/handle_runner.hpp>
#include <gunrock/app/scc/scc_enactor.hpp>
#include <gunrock/app/scc/scc_problem.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::scc;

static_assert(GRX_SCC_PHASE_TRIM == PHASE_TRIM && GRX_SCC_PHASE_PIVOT == PHASE_PIVOT && GRX_SCC_PHASE_COLOUR == PHASE_COLOUR,
              "the header's phase kinds are the enactor's");
static_assert(GRX_SCC_AUTO == SCC_AUTO && GRX_SCC_ROUNDS == SCC_ROUNDS && GRX_SCC_DEVICE_LOOP == SCC_DEVICE_LOOP,
              "the header's schedules are the enactor's schedules");

namespace {

struct SccRunner {
    InitState state;
    virtual ~SccRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_iro, int *d_ici) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual hipError_t Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms, double &build_ms) = 0;
    virtual int PhaseTrace(int max_phases, int *kind, long long *vertices, double *ms) = 0;
    virtual hipError_t Extract(int *comp, long long *components) = 0;
    virtual hipError_t Summary(long long *components, long long *trivial, long long *largest, int *largest_root) = 0;
    virtual hipError_t Sizes(int *size) = 0;
    virtual hipError_t Condensation(long long max_edges, int *from, int *to, long long *count) = 0;
    virtual void DeviceResults(int **d_comp, int **d_iro, int **d_ici) = 0;
};

template <bool INSTR>
struct SccRunnerT : SccRunner {
    typedef SccProblem<false> Problem;
    Problem problem;
    SccEnactor<INSTR> enactor;
    EventPair timer;
    explicit SccRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g) override
    {
        const hipError_t rc = problem.Init(false, g, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_iro, int *d_ici) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci, d_iro, d_ici);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetOption(const char *name, double value) override
    {
        const int shared = enactor.loop.Set(name, value, SCC_DEVICE_LOOP);
        if (shared != 1) return shared;
        const long long v = Whole(value);
        if (!std::strcmp(name, "pivot_phase")) {
            if (v < 0 || v > 1) return -1;
            enactor.pivot_phase = static_cast<int>(v);
        } else if (!std::strcmp(name, "trim")) {
            if (v < 0 || v > 1) return -1;
            enactor.trim = static_cast<int>(v);
        } else if (!std::strcmp(name, "pair_trim")) {
            if (v < 0 || v > 1) return -1;
            enactor.pair_trim = static_cast<int>(v);
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
    void Stats(long long *out, double &kernel_ms, double &build_ms) override
    {
        out[0] = enactor.trimmed;
        out[1] = enactor.trim_rounds;
        out[2] = enactor.pivot_component;
        out[3] = enactor.colour_rounds;
        out[4] = enactor.sweeps;
        out[5] = enactor.bfs_levels;
        out[6] = enactor.entries_read;
        out[7] = enactor.step.launches;
        kernel_ms = enactor.step.kernel_ms;
        build_ms = problem.build_ms;
    }
    int PhaseTrace(int max_phases, int *kind, long long *vertices, double *ms) override
    {
        return CopyTrace(enactor.trace_kind.size(), max_phases, Column(kind, [&](int i) { return enactor.trace_kind[i]; }),
                         Column(vertices, [&](int i) { return enactor.trace_vertices[i]; }), Column(ms, [&](int i) { return enactor.trace_ms[i]; }));
    }
    hipError_t Extract(int *comp, long long *components) override { return state.ready ? problem.Extract(comp, components) : hipErrorNotReady; }
    hipError_t Summary(long long *components, long long *trivial, long long *largest, int *largest_root) override
    {
        return state.ready ? problem.Summary(components, trivial, largest, largest_root) : hipErrorNotReady;
    }
    hipError_t Sizes(int *size) override { return state.ready ? problem.Sizes(size) : hipErrorNotReady; }
    hipError_t Condensation(long long max_edges, int *from, int *to, long long *count) override
    {
        return state.ready ? problem.Condensation(max_edges, from, to, count) : hipErrorNotReady;
    }
    void DeviceResults(int **d_comp, int **d_iro, int **d_ici) override
    {
        if (d_comp) *d_comp = state.ready ? problem.data_slices[0]->d_comp : nullptr;
        if (d_iro) *d_iro = state.ready ? problem.data_slices[0]->d_iro : nullptr;
        if (d_ici) *d_ici = state.ready ? problem.data_slices[0]->d_ici : nullptr;
    }
};

}  // namespace

struct grx_scc {
    std::unique_ptr<SccRunner> runner;
};

extern "C" {

int grx_scc_create(grx_scc **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_scc{MakeRunner<SccRunner, SccRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_scc_init(grx_scc *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_scc_init_device(grx_scc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_inv_row_offsets, int *d_inv_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (d_inv_row_offsets ? (edges > 0 && !d_inv_col_indices) : d_inv_col_indices != nullptr) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_inv_row_offsets, d_inv_col_indices);
}

int grx_scc_set_option(grx_scc *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_scc_reset(grx_scc *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_scc_enact(grx_scc *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Enact(max_grid_size, elapsed_ms));
}

int grx_scc_stats(grx_scc *p, long long *trimmed, long long *trim_rounds, long long *pivot_component, long long *colour_rounds, long long *sweeps,
                  long long *bfs_levels, long long *entries_read, long long *kernel_launches, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double k = 0, b = 0;
    p->runner->Stats(v, k, b);
    long long *out[8] = {trimmed, trim_rounds, pivot_component, colour_rounds, sweeps, bfs_levels, entries_read, kernel_launches};
    for (int i = 0; i < 8; ++i)
        if (out[i]) *out[i] = v[i];
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_scc_phase_trace(grx_scc *p, int max_phases, int *kind, long long *vertices, double *ms)
{
    if (!p) return -1;
    return p->runner->PhaseTrace(max_phases, kind, vertices, ms);
}

int grx_scc_extract(grx_scc *p, int *h_comp, long long *components)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_comp, components));
}

int grx_scc_summary(grx_scc *p, long long *components, long long *trivial, long long *largest, int *largest_root)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Summary(components, trivial, largest, largest_root));
}

int grx_scc_sizes(grx_scc *p, int *h_size)
{
    if (!p || !h_size) return -1;
    return static_cast<int>(p->runner->Sizes(h_size));
}

int grx_scc_condensation(grx_scc *p, int max_edges, int *h_from, int *h_to)
{
    if (!p || max_edges < 0) return -1;
    long long count = 0;
    const hipError_t rc = p->runner->Condensation(max_edges, h_from, h_to, &count);
    return rc ? -static_cast<int>(rc) : static_cast<int>(count);
}

int grx_scc_device_results(grx_scc *p, int **d_comp, int **d_inv_row_offsets, int **d_inv_col_indices)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_comp, d_inv_row_offsets, d_inv_col_indices);
    return 0;
}

void grx_scc_destroy(grx_scc *p) { delete p; }

}  // extern "C"
