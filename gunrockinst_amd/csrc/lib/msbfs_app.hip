// lib/msbfs_app.hip -- multi-source BFS entry points of libgunrock.so.
//  * grx_msbfs_*: MsbfsProblem / MsbfsEnactor phases as separate C calls (the reference snapshot has no MS-BFS; the calls are
//    shaped like grx_scc_*).  The results are integers: depth[source][vertex] (int32, optional), per source the vertices reached, the
//    sum of their depths and the eccentricity, per vertex the sources that reach it and the sum of their distances.
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/handle_runner.hpp>
#include <gunrock/app/msbfs/msbfs_enactor.hpp>
#include <gunrock/app/msbfs/msbfs_problem.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::msbfs;

static_assert(GRX_MSBFS_AUTO == MSBFS_AUTO && GRX_MSBFS_PUSH == MSBFS_PUSH && GRX_MSBFS_PULL == MSBFS_PULL && GRX_MSBFS_ALTERNATE == MSBFS_ALTERNATE,
              "the header's directions are the enactor's");
static_assert(GRX_MSBFS_INVERSE_AUTO == INVERSE_AUTO && GRX_MSBFS_INVERSE_NONE == INVERSE_NONE && GRX_MSBFS_INVERSE_SELF == INVERSE_SELF &&
                  GRX_MSBFS_INVERSE_BUILD == INVERSE_BUILD,
              "the header's inverse choices are the problem's");
static_assert(GRX_MSBFS_LEVEL_PUSH == LEVEL_PUSH && GRX_MSBFS_LEVEL_PULL == LEVEL_PULL, "the header's level kinds are the enactor's");
static_assert(GRX_MSBFS_DEPTHS_NOT_STORED == kDepthsNotStored && GRX_MSBFS_INVERSE_NOT_SYMMETRIC == kInverseNotSymmetric,
              "the header's codes are the problem's");

namespace {

struct MsbfsRunner {
    InitState state;
    virtual ~MsbfsRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_iro, int *d_ici) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int Reset(const int *sources, int count, bool store_depths) = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms, double &build_ms) = 0;
    virtual int LevelTrace(int max_levels, int *batch, int *level, int *kind, long long *frontier, long long *edges, double *ms) = 0;
    virtual int ExtractDepths(int first, int count, int *h_depth) = 0;
    virtual int SourceSummary(long long *reached, long long *dist_sum, int *ecc) = 0;
    virtual int VertexSummary(int *sources_reaching, long long *in_dist_sum) = 0;
    virtual void DeviceResults(int **d_depth, long long **d_reached, long long **d_dist_sum, int **d_ecc, int **d_sources_reaching,
                               long long **d_in_dist_sum) = 0;
};

template <bool INSTR>
struct MsbfsRunnerT : MsbfsRunner {
    typedef MsbfsProblem<false> Problem;
    Problem problem;
    MsbfsEnactor<INSTR> enactor;
    EventPair timer;
    explicit MsbfsRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    bool HasSources() const { return state.ready && !problem.sources.empty(); }
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
        const long long v = static_cast<long long>(value);
        if (!std::strcmp(name, "direction")) {
            if (v < MSBFS_AUTO || v > MSBFS_ALTERNATE) return -1;
            enactor.direction = static_cast<int>(v);
        } else if (!std::strcmp(name, "inverse")) {
            if (v < INVERSE_AUTO || v > INVERSE_BUILD) return -1;
            problem.inverse = static_cast<int>(v);
        } else if (!std::strcmp(name, "alpha")) {
            if (!(value > 0)) return -1;
            enactor.alpha = value;
        } else if (!std::strcmp(name, "beta")) {
            if (!(value > 0)) return -1;
            enactor.beta = value;
        } else if (!std::strcmp(name, "wave_min_row")) {
            if (v < 1) return -1;
            enactor.wave_min_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else {
            return 1;
        }
        return 0;
    }
    int Reset(const int *sources, int count, bool store_depths) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        for (int i = 0; i < count; ++i)
            if (sources[i] < 0 || sources[i] >= problem.nodes) return -1;
        bool refused = false;
        const hipError_t rc = problem.Reset(sources, count, store_depths, &refused);
        return refused ? kInverseNotSymmetric : static_cast<int>(rc);
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!HasSources()) return static_cast<int>(hipErrorNotReady);
        bool refused = false;
        const hipError_t rc = timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size, &refused); });
        return refused ? kInverseNotSymmetric : static_cast<int>(rc);
    }
    void Stats(long long *out, double &kernel_ms, double &build_ms) override
    {
        out[0] = enactor.batches;
        out[1] = enactor.levels;
        out[2] = enactor.push_levels;
        out[3] = enactor.pull_levels;
        out[4] = enactor.entries_read;
        out[5] = enactor.step.launches;
        kernel_ms = enactor.step.kernel_ms;
        build_ms = problem.build_ms;
    }
    int LevelTrace(int max_levels, int *batch, int *level, int *kind, long long *frontier, long long *edges, double *ms) override
    {
        return CopyTrace(enactor.trace_kind.size(), max_levels, Column(batch, [&](int i) { return enactor.trace_batch[i]; }),
                         Column(level, [&](int i) { return enactor.trace_level[i]; }), Column(kind, [&](int i) { return enactor.trace_kind[i]; }),
                         Column(frontier, [&](int i) { return enactor.trace_frontier[i]; }), Column(edges, [&](int i) { return enactor.trace_edges[i]; }),
                         Column(ms, [&](int i) { return enactor.trace_ms[i]; }));
    }
    int ExtractDepths(int first, int count, int *h_depth) override
    {
        if (!HasSources()) return static_cast<int>(hipErrorNotReady);
        if (!problem.store_depths) return kDepthsNotStored;
        if (first < 0 || count < 0 || static_cast<size_t>(first) + static_cast<size_t>(count) > problem.sources.size()) return -1;
        return static_cast<int>(problem.ExtractDepths(first, count, h_depth));
    }
    int SourceSummary(long long *reached, long long *dist_sum, int *ecc) override
    {
        return HasSources() ? static_cast<int>(problem.SourceSummary(reached, dist_sum, ecc)) : static_cast<int>(hipErrorNotReady);
    }
    int VertexSummary(int *sources_reaching, long long *in_dist_sum) override
    {
        return HasSources() ? static_cast<int>(problem.VertexSummary(sources_reaching, in_dist_sum)) : static_cast<int>(hipErrorNotReady);
    }
    void DeviceResults(int **d_depth, long long **d_reached, long long **d_dist_sum, int **d_ecc, int **d_sources_reaching, long long **d_in_dist_sum) override
    {
        const bool have = HasSources();
        typename Problem::DataSlice *ds = have ? problem.data_slices[0] : nullptr;
        if (d_depth) *d_depth = have && problem.store_depths ? ds->d_depth : nullptr;
        if (d_reached) *d_reached = have ? reinterpret_cast<long long *>(ds->d_reached.p) : nullptr;
        if (d_dist_sum) *d_dist_sum = have ? reinterpret_cast<long long *>(ds->d_dist_sum.p) : nullptr;
        if (d_ecc) *d_ecc = have ? ds->d_ecc : nullptr;
        if (d_sources_reaching) *d_sources_reaching = have ? ds->d_sources_reaching : nullptr;
        if (d_in_dist_sum) *d_in_dist_sum = have ? reinterpret_cast<long long *>(ds->d_in_dist_sum.p) : nullptr;
    }
};

}  // namespace

struct grx_msbfs {
    std::unique_ptr<MsbfsRunner> runner;
};

extern "C" {

int grx_msbfs_create(grx_msbfs **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_msbfs{MakeRunner<MsbfsRunner, MsbfsRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_msbfs_init(grx_msbfs *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_msbfs_init_device(grx_msbfs *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_inv_row_offsets, int *d_inv_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (d_inv_row_offsets ? (edges > 0 && !d_inv_col_indices) : d_inv_col_indices != nullptr) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_inv_row_offsets, d_inv_col_indices);
}

int grx_msbfs_set_option(grx_msbfs *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_msbfs_reset(grx_msbfs *p, const int *sources, int count, int store_depths)
{
    if (!p || !sources || count < 1) return -1;
    return p->runner->Reset(sources, count, store_depths != 0);
}

int grx_msbfs_enact(grx_msbfs *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_msbfs_stats(grx_msbfs *p, long long *batches, long long *levels, long long *push_levels, long long *pull_levels, long long *entries_read,
                    long long *kernel_launches, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    long long v[6] = {0, 0, 0, 0, 0, 0};
    double k = 0, b = 0;
    p->runner->Stats(v, k, b);
    long long *out[6] = {batches, levels, push_levels, pull_levels, entries_read, kernel_launches};
    for (int i = 0; i < 6; ++i)
        if (out[i]) *out[i] = v[i];
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_msbfs_level_trace(grx_msbfs *p, int max_levels, int *batch, int *level, int *kind, long long *frontier, long long *edges, double *ms)
{
    if (!p) return -1;
    return p->runner->LevelTrace(max_levels, batch, level, kind, frontier, edges, ms);
}

int grx_msbfs_extract_depths(grx_msbfs *p, int first_source, int source_count, int *h_depth)
{
    if (!p || !h_depth) return -1;
    return p->runner->ExtractDepths(first_source, source_count, h_depth);
}

int grx_msbfs_source_summary(grx_msbfs *p, long long *reached, long long *dist_sum, int *ecc)
{
    if (!p) return -1;
    return p->runner->SourceSummary(reached, dist_sum, ecc);
}

int grx_msbfs_vertex_summary(grx_msbfs *p, int *sources_reaching, long long *in_dist_sum)
{
    if (!p) return -1;
    return p->runner->VertexSummary(sources_reaching, in_dist_sum);
}

int grx_msbfs_device_results(grx_msbfs *p, int **d_depth, long long **d_reached, long long **d_dist_sum, int **d_ecc, int **d_sources_reaching,
                             long long **d_in_dist_sum)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_depth, d_reached, d_dist_sum, d_ecc, d_sources_reaching, d_in_dist_sum);
    return 0;
}

void grx_msbfs_destroy(grx_msbfs *p) { delete p; }

}  // extern "C"
