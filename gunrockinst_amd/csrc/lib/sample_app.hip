// lib/sample_app.hip -- neighbourhood-sampling entry points of libgunrock.so.
//  * grx_sample_*: SampleProblem / SampleEnactor phases as separate C calls (the reference snapshot has no sampling; the calls are
//    shaped like grx_rw_*).  set_fanouts gives the hops, Reset the seeds; sizes / extract give the sampled subgraph.
#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/sample/sample_enactor.hpp>
#include <gunrock/app/sample/sample_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::sample;

static_assert(GRX_SAMPLE_AUTO == SAMPLE_AUTO && GRX_SAMPLE_LANE == SAMPLE_LANE && GRX_SAMPLE_GROUP == SAMPLE_GROUP,
              "the header's strategies are the kernels' strategies");
static_assert(GRX_SAMPLE_TOO_LARGE == kSampleTooLarge, "the header's refusal is the enactor's");
static_assert(sizeof(long long) == sizeof(unsigned long long) && sizeof(long long) == 8, "offsets are 64-bit");

namespace {

struct SampleStats {
    int hops = 0;
    const long long *expanded = nullptr, *sampled = nullptr, *copied = nullptr;
    long long long_rows = 0, launches = 0, readbacks = 0;
    double kernel_ms = 0, build_ms = 0;
    const double *phase_ms = nullptr;
};

struct SampleRunner {
    InitState state;
    bool started = false;   // a Reset gave seeds
    bool finished = false;  // the last Enact ran to its end: there is a result to extract
    virtual ~SampleRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_w) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int SetFanouts(int hops, const int *fanouts) = 0;
    virtual int Reset(int num_seeds, const int *h_seeds) = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(SampleStats &s) = 0;
    virtual int Sizes(long long *vertices, long long *edges, long long *vertex_ptr, long long *edge_ptr) = 0;
    virtual int Extract(int *vertices, long long *offsets, int *cols, int *eids) = 0;
    virtual void DeviceResults(int **d_vertices, long long **d_offsets, int **d_cols, int **d_eids) = 0;
};

template <bool INSTR>
struct SampleRunnerT : SampleRunner {
    typedef SampleProblem<false> Problem;
    Problem problem;
    SampleEnactor<INSTR> enactor;
    EventPair timer;
    explicit SampleRunnerT(int device) : enactor(false)
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
    int SetOption(const char *name, double value) override { return enactor.options.Set(name, value, state.ready && problem.weights); }
    int SetFanouts(int hops, const int *fanouts) override { return enactor.options.SetFanouts(hops, fanouts); }
    int Reset(int num_seeds, const int *h_seeds) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        if (!DistinctVertices(h_seeds, num_seeds, problem.nodes)) return -1;
        finished = false;
        started = false;
        const hipError_t rc = problem.Reset(num_seeds, h_seeds);
        started = rc == hipSuccess;
        return static_cast<int>(rc);
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready || !started || enactor.options.fanouts.empty()) return static_cast<int>(hipErrorNotReady);
        finished = false;
        const hipError_t rc = timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
        if (rc) return static_cast<int>(rc);
        if (enactor.refused) return kSampleTooLarge;
        finished = true;
        return 0;
    }
    void Stats(SampleStats &s) override
    {
        s.hops = enactor.hops;
        s.expanded = enactor.rows_expanded;
        s.sampled = enactor.rows_sampled;
        s.copied = enactor.rows_copied;
        s.long_rows = enactor.long_rows;
        s.launches = enactor.host.launches;
        s.readbacks = enactor.host.readbacks;
        s.kernel_ms = enactor.host.kernel_ms;
        s.phase_ms = enactor.phase_ms;
        s.build_ms = problem.build_ms;
    }
    int Sizes(long long *vertices, long long *edges, long long *vertex_ptr, long long *edge_ptr) override
    {
        if (!state.ready || !finished) return static_cast<int>(hipErrorNotReady);
        if (vertices) *vertices = problem.num_vertices;
        if (edges) *edges = problem.num_edges;
        if (vertex_ptr) std::copy(enactor.vertex_ptr.begin(), enactor.vertex_ptr.end(), vertex_ptr);
        if (edge_ptr) std::copy(enactor.edge_ptr.begin(), enactor.edge_ptr.end(), edge_ptr);
        return 0;
    }
    int Extract(int *vertices, long long *offsets, int *cols, int *eids) override
    {
        if (!state.ready || !finished) return static_cast<int>(hipErrorNotReady);
        if (eids && !enactor.with_eids) return -1;
        return static_cast<int>(problem.Extract(vertices, offsets, cols, eids));
    }
    void DeviceResults(int **d_vertices, long long **d_offsets, int **d_cols, int **d_eids) override
    {
        typename Problem::DataSlice *ds = state.ready && finished ? problem.data_slices[0] : nullptr;
        if (d_vertices) *d_vertices = ds ? ds->d_vertices : nullptr;
        if (d_offsets) *d_offsets = ds ? ds->d_offsets : nullptr;
        if (d_cols) *d_cols = ds && problem.num_edges ? ds->d_cols : nullptr;
        if (d_eids) *d_eids = ds && problem.num_edges && enactor.with_eids ? ds->d_eids : nullptr;
    }
};

}  // namespace

struct grx_sample {
    std::unique_ptr<SampleRunner> runner;
};

extern "C" {

int grx_sample_create(grx_sample **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_sample{MakeRunner<SampleRunner, SampleRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_sample_init(grx_sample *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices, weights);
    return p->runner->Init(wrap.graph);
}

int grx_sample_init_device(grx_sample *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_weights);
}

int grx_sample_set_option(grx_sample *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_sample_set_fanouts(grx_sample *p, int hops, const int *fanouts)
{
    if (!p) return -1;
    return p->runner->SetFanouts(hops, fanouts);
}

int grx_sample_reset(grx_sample *p, int num_seeds, const int *h_seeds)
{
    if (!p || num_seeds < 1 || !h_seeds) return -1;
    return p->runner->Reset(num_seeds, h_seeds);
}

int grx_sample_enact(grx_sample *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_sample_stats(grx_sample *p, int *hops, long long *rows_expanded, long long *rows_sampled, long long *rows_copied, long long *long_rows,
                     long long *kernel_launches, long long *readbacks, double *kernel_ms, double *phase_ms, double *build_ms)
{
    if (!p) return -1;
    SampleStats s;
    p->runner->Stats(s);
    if (hops) *hops = s.hops;
    for (int h = 0; h < s.hops; ++h) {
        if (rows_expanded) rows_expanded[h] = s.expanded[h];
        if (rows_sampled) rows_sampled[h] = s.sampled[h];
        if (rows_copied) rows_copied[h] = s.copied[h];
    }
    if (long_rows) *long_rows = s.long_rows;
    if (kernel_launches) *kernel_launches = s.launches;
    if (readbacks) *readbacks = s.readbacks;
    if (kernel_ms) *kernel_ms = s.kernel_ms;
    if (phase_ms)
        for (int k = 0; k < PHASES; ++k) phase_ms[k] = s.phase_ms[k];
    if (build_ms) *build_ms = s.build_ms;
    return 0;
}

int grx_sample_sizes(grx_sample *p, long long *vertices, long long *edges, long long *vertex_ptr, long long *edge_ptr)
{
    if (!p) return -1;
    return p->runner->Sizes(vertices, edges, vertex_ptr, edge_ptr);
}

int grx_sample_extract(grx_sample *p, int *h_vertices, long long *h_offsets, int *h_cols, int *h_eids)
{
    if (!p) return -1;
    return p->runner->Extract(h_vertices, h_offsets, h_cols, h_eids);
}

int grx_sample_device_results(grx_sample *p, int **d_vertices, long long **d_offsets, int **d_cols, int **d_eids)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_vertices, d_offsets, d_cols, d_eids);
    return 0;
}

void grx_sample_destroy(grx_sample *p) { delete p; }

}  // extern "C"
