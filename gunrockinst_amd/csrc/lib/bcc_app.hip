// lib/bcc_app.hip -- biconnected components, articulation points and bridges entry points of libgunrock.so.
//  * grx_bcc_*: BccProblem / BccEnactor phases as separate C calls (the reference snapshot has no BCC; the calls are shaped like
//    grx_scc_* and grx_truss_*).  Every per-edge array is indexed by the canonical edge id (grx_bcc_edges).
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/bcc/bcc_enactor.hpp>
#include <gunrock/app/bcc/bcc_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::bcc;

static_assert(GRX_BCC_AUTO == BCC_AUTO && GRX_BCC_ROUNDS == BCC_ROUNDS && GRX_BCC_DEVICE_LOOP == BCC_DEVICE_LOOP,
              "the header's schedules are the enactor's schedules");
static_assert(GRX_BCC_PHASE_FOREST == PHASE_FOREST && GRX_BCC_PHASE_SIZES == PHASE_SIZES && GRX_BCC_PHASE_NUMBER == PHASE_NUMBER &&
                  GRX_BCC_PHASE_LOWHIGH == PHASE_LOWHIGH && GRX_BCC_PHASE_LINK == PHASE_LINK && GRX_BCC_PHASE_LABEL == PHASE_LABEL,
              "the header's phase kinds are the enactor's");

namespace {

struct BccRunner {
    InitState state;
    virtual ~BccRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual hipError_t Reset() = 0;
    virtual hipError_t Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms, double &build_ms) = 0;
    virtual int PhaseTrace(int max_phases, int *kind, long long *items, double *ms) = 0;
    virtual hipError_t Edges(int *src, int *dst, long long *count) = 0;
    virtual hipError_t Extract(int *bcc_out, unsigned char *bridge, unsigned char *art, int *tecc, int *block_size) = 0;
    virtual hipError_t GetSummary(Summary *out) = 0;
    virtual hipError_t BlockCut(long long max_edges, int *vertex, int *block, long long *count) = 0;
    virtual void DeviceResults(void **out) = 0;
};

template <bool INSTR>
struct BccRunnerT : BccRunner {
    typedef BccProblem<false> Problem;
    Problem problem;
    BccEnactor<INSTR> enactor;
    EventPair timer;
    explicit BccRunnerT(int device) : enactor(false)
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
        return enactor.loop.Set(name, value, BCC_DEVICE_LOOP);  // (no option of its own)
    }
    bool Done() const { return state.ready && problem.enacted; }
    hipError_t Reset() override { return state.ready ? problem.Reset() : hipErrorNotReady; }
    hipError_t Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return hipErrorNotReady;
        return timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
    }
    void Stats(long long *out, double &kernel_ms, double &build_ms) override
    {
        out[0] = problem.simple_edges;
        out[1] = enactor.trees;
        out[2] = enactor.levels;
        out[3] = enactor.entries_read;
        out[4] = enactor.step.launches;
        out[5] = enactor.step.readbacks;
        kernel_ms = enactor.step.kernel_ms;
        build_ms = problem.build_ms;
    }
    int PhaseTrace(int max_phases, int *kind, long long *items, double *ms) override
    {
        return CopyTrace(enactor.trace_items.size(), max_phases, Column(kind, [&](int i) { return i; }),
                         Column(items, [&](int i) { return enactor.trace_items[i]; }), Column(ms, [&](int i) { return enactor.trace_ms[i]; }));
    }
    hipError_t Edges(int *src, int *dst, long long *count) override
    {
        if (!state.ready) return hipErrorNotReady;
        *count = problem.simple_edges;
        return problem.Edges(src, dst);
    }
    hipError_t Extract(int *bcc_out, unsigned char *bridge, unsigned char *art, int *tecc, int *block_size) override
    {
        return Done() ? problem.Extract(bcc_out, bridge, art, tecc, block_size) : hipErrorNotReady;
    }
    hipError_t GetSummary(Summary *out) override
    {
        if (!Done()) return hipErrorNotReady;
        *out = problem.summary;
        return hipSuccess;
    }
    hipError_t BlockCut(long long max_edges, int *vertex, int *block, long long *count) override
    {
        return Done() ? problem.BlockCut(max_edges, vertex, block, count) : hipErrorNotReady;
    }
    void DeviceResults(void **out) override
    {
        typename Problem::DataSlice *ds = state.ready ? problem.data_slices[0] : nullptr;
        void *p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (ds) {
            void *have[8] = {ds->d_bcc, ds->d_tecc, ds->d_bridge, ds->d_art, ds->d_src, ds->d_dst, ds->d_parent, ds->d_level};
            for (int i = 0; i < 8; ++i) p[i] = have[i];
        }
        for (int i = 0; i < 8; ++i) out[i] = p[i];
    }
};

}  // namespace

struct grx_bcc {
    std::unique_ptr<BccRunner> runner;
};

extern "C" {

int grx_bcc_create(grx_bcc **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_bcc{MakeRunner<BccRunner, BccRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_bcc_init(grx_bcc *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_bcc_init_device(grx_bcc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices);
}

int grx_bcc_set_option(grx_bcc *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_bcc_reset(grx_bcc *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_bcc_enact(grx_bcc *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Enact(max_grid_size, elapsed_ms));
}

int grx_bcc_stats(grx_bcc *p, long long *simple_edges, long long *trees, long long *levels, long long *entries_read, long long *kernel_launches,
                  long long *readbacks, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    long long v[6] = {0, 0, 0, 0, 0, 0};
    double k = 0, b = 0;
    p->runner->Stats(v, k, b);
    long long *out[6] = {simple_edges, trees, levels, entries_read, kernel_launches, readbacks};
    for (int i = 0; i < 6; ++i)
        if (out[i]) *out[i] = v[i];
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_bcc_phase_trace(grx_bcc *p, int max_phases, int *kind, long long *items, double *ms)
{
    if (!p) return -1;
    return p->runner->PhaseTrace(max_phases, kind, items, ms);
}

int grx_bcc_edges(grx_bcc *p, int *h_src, int *h_dst)
{
    if (!p) return -1;
    long long count = 0;  // M <= the entries of the CSR: an int
    const hipError_t rc = p->runner->Edges(h_src, h_dst, &count);
    return rc ? -static_cast<int>(rc) : static_cast<int>(count);
}

int grx_bcc_extract(grx_bcc *p, int *h_bcc, unsigned char *h_bridge, unsigned char *h_articulation, int *h_tecc, int *h_block_size)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_bcc, h_bridge, h_articulation, h_tecc, h_block_size));
}

int grx_bcc_summary(grx_bcc *p, long long *blocks, long long *bridges, long long *articulation_points, long long *largest_block,
                    int *largest_block_id, long long *tecc_components, long long *largest_tecc, int *largest_tecc_root)
{
    if (!p) return -1;
    Summary s;
    const hipError_t rc = p->runner->GetSummary(&s);
    if (rc) return static_cast<int>(rc);
    if (blocks) *blocks = s.blocks;
    if (bridges) *bridges = s.bridges;
    if (articulation_points) *articulation_points = s.articulation_points;
    if (largest_block) *largest_block = s.largest_block;
    if (largest_block_id) *largest_block_id = s.largest_block_id;
    if (tecc_components) *tecc_components = s.tecc_components;
    if (largest_tecc) *largest_tecc = s.largest_tecc;
    if (largest_tecc_root) *largest_tecc_root = s.largest_tecc_root;
    return 0;
}

int grx_bcc_block_cut(grx_bcc *p, int max_edges, int *h_vertex, int *h_block)
{
    if (!p || max_edges < 0) return -1;
    long long count = 0;
    const hipError_t rc = p->runner->BlockCut(max_edges, h_vertex, h_block, &count);
    return rc ? -static_cast<int>(rc) : static_cast<int>(count);
}

int grx_bcc_device_results(grx_bcc *p, int **d_bcc, int **d_tecc, unsigned char **d_bridge, unsigned char **d_articulation, int **d_src,
                           int **d_dst, int **d_parent, int **d_level)
{
    if (!p) return -1;
    void *out[8];
    p->runner->DeviceResults(out);
    if (d_bcc) *d_bcc = static_cast<int *>(out[0]);
    if (d_tecc) *d_tecc = static_cast<int *>(out[1]);
    if (d_bridge) *d_bridge = static_cast<unsigned char *>(out[2]);
    if (d_articulation) *d_articulation = static_cast<unsigned char *>(out[3]);
    if (d_src) *d_src = static_cast<int *>(out[4]);
    if (d_dst) *d_dst = static_cast<int *>(out[5]);
    if (d_parent) *d_parent = static_cast<int *>(out[6]);
    if (d_level) *d_level = static_cast<int *>(out[7]);
    return 0;
}

void grx_bcc_destroy(grx_bcc *p) { delete p; }

}  // extern "C"
