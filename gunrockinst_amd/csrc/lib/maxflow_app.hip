// lib/maxflow_app.hip -- maximum flow and minimum cut entry points of libgunrock.so.
//  * grx_maxflow_*: MaxflowProblem / MaxflowEnactor phases as separate C calls (the reference snapshot has no max-flow; the calls
//    are shaped like grx_bcc_*).  Every per-pair array is indexed by the canonical pair id (grx_maxflow_pairs).
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/handle_runner.hpp>
#include <gunrock/app/maxflow/maxflow_enactor.hpp>
#include <gunrock/app/maxflow/maxflow_problem.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::maxflow;

static_assert(GRX_MAXFLOW_AUTO == MAXFLOW_AUTO && GRX_MAXFLOW_ROUNDS == MAXFLOW_ROUNDS && GRX_MAXFLOW_DEVICE_LOOP == MAXFLOW_DEVICE_LOOP,
              "the header's schedules are the enactor's schedules");
static_assert(GRX_MAXFLOW_PHASE_PREFLOW == PHASE_PREFLOW && GRX_MAXFLOW_PHASE_RETURN == PHASE_RETURN && GRX_MAXFLOW_PHASE_CUT == PHASE_CUT,
              "the header's phase kinds are the enactor's");
static_assert(GRX_MAXFLOW_GAVE_UP == kGaveUp, "the header's code is the enactor's");

namespace {

struct MaxflowRunner {
    InitState state;
    virtual ~MaxflowRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_cap) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int Reset(int src, int sink) = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms, double &build_ms) = 0;
    virtual int PhaseTrace(int max_phases, int *kind, long long *rounds, double *ms) = 0;
    virtual hipError_t Pairs(int *a, int *b, int *cap_ab, int *cap_ba, long long *count) = 0;
    virtual hipError_t Extract(long long *value, int *flow, unsigned char *side, unsigned char *cut) = 0;
    virtual hipError_t ArcFlow(int *arc_flow) = 0;
    virtual hipError_t GetSummary(Summary *out) = 0;
    virtual void DeviceResults(void **out) = 0;
};

template <bool INSTR>
struct MaxflowRunnerT : MaxflowRunner {
    typedef MaxflowProblem<false> Problem;
    Problem problem;
    MaxflowEnactor<INSTR> enactor;
    EventPair timer;
    explicit MaxflowRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g) override
    {
        const hipError_t rc = problem.Init(false, g, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_cap) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci, d_cap);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetOption(const char *name, double value) override
    {
        if (!(value == value)) return -1;  // (NaN)
        const int shared = enactor.loop.Set(name, value, MAXFLOW_DEVICE_LOOP);
        if (shared != 1) return shared;
        const long long v = Whole(value);
        if (!std::strcmp(name, "discharge_steps")) {
            if (v < 1 || v > 1024) return -1;
            enactor.discharge_steps = static_cast<int>(v);
        } else if (!std::strcmp(name, "relabel_interval")) {
            if (value < 0) return -1;
            enactor.relabel_interval = value;
        } else if (!std::strcmp(name, "max_rounds")) {
            if (v < 1 || v > kMaxMaxRounds) return -1;
            enactor.max_rounds = v;
        } else {
            return 1;
        }
        return 0;
    }
    bool Done() const { return state.ready && problem.enacted; }
    int Reset(int src, int sink) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        if (src < 0 || sink < 0 || src >= problem.nodes || sink >= problem.nodes || src == sink) return -1;
        return static_cast<int>(problem.Reset(src, sink));
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        const hipError_t rc =
            timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
        return rc != hipSuccess && enactor.gave_up ? kGaveUp : static_cast<int>(rc);
    }
    void Stats(long long *out, double &kernel_ms, double &build_ms) override
    {
        out[0] = problem.pairs;
        out[1] = enactor.rounds;
        out[2] = enactor.global_relabels;
        out[3] = enactor.pushes;
        out[4] = enactor.relabels;
        out[5] = enactor.entries_read;
        out[6] = enactor.step.launches;
        out[7] = enactor.step.readbacks;
        kernel_ms = enactor.step.kernel_ms;
        build_ms = problem.build_ms;
    }
    int PhaseTrace(int max_phases, int *kind, long long *rounds, double *ms) override
    {
        return CopyTrace(enactor.trace_rounds.size(), max_phases, Column(kind, [&](int i) { return i; }),
                         Column(rounds, [&](int i) { return enactor.trace_rounds[i]; }), Column(ms, [&](int i) { return enactor.trace_ms[i]; }));
    }
    hipError_t Pairs(int *a, int *b, int *cap_ab, int *cap_ba, long long *count) override
    {
        if (!state.ready) return hipErrorNotReady;
        *count = problem.pairs;
        return problem.Pairs(a, b, cap_ab, cap_ba);
    }
    hipError_t Extract(long long *value, int *flow, unsigned char *side, unsigned char *cut) override
    {
        if (!Done()) return hipErrorNotReady;
        if (value) *value = problem.summary.value;
        return problem.Extract(flow, side, cut);
    }
    hipError_t ArcFlow(int *arc_flow) override { return Done() ? problem.ArcFlow(arc_flow) : hipErrorNotReady; }
    hipError_t GetSummary(Summary *out) override
    {
        if (!Done()) return hipErrorNotReady;
        *out = problem.summary;
        return hipSuccess;
    }
    void DeviceResults(void **out) override
    {
        typename Problem::DataSlice *ds = state.ready ? problem.data_slices[0] : nullptr;
        for (int i = 0; i < 7; ++i) out[i] = nullptr;
        if (ds) {
            void *have[7] = {ds->d_flow, ds->d_side, ds->d_cut, ds->d_a, ds->d_b, ds->d_excess, ds->d_height};
            for (int i = 0; i < 7; ++i) out[i] = have[i];
        }
    }
};

}  // namespace

struct grx_maxflow {
    std::unique_ptr<MaxflowRunner> runner;
};

extern "C" {

int grx_maxflow_create(grx_maxflow **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_maxflow{MakeRunner<MaxflowRunner, MaxflowRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_maxflow_init(grx_maxflow *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *capacities)
{
    if (!p || !row_offsets || nodes < 1 || nodes > (1 << 30) || edges < 0) return -1;  // (heights go up to 2 * nodes)
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices, capacities);
    return p->runner->Init(wrap.graph);
}

int grx_maxflow_init_device(grx_maxflow *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_capacities)
{
    if (!p || !d_row_offsets || nodes < 1 || nodes > (1 << 30) || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_capacities);
}

int grx_maxflow_set_option(grx_maxflow *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_maxflow_reset(grx_maxflow *p, int src, int sink) { return p ? p->runner->Reset(src, sink) : -1; }

int grx_maxflow_enact(grx_maxflow *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_maxflow_stats(grx_maxflow *p, long long *pairs, long long *rounds, long long *global_relabels, long long *pushes, long long *relabels,
                      long long *entries_read, long long *kernel_launches, long long *readbacks, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double k = 0, b = 0;
    p->runner->Stats(v, k, b);
    long long *out[8] = {pairs, rounds, global_relabels, pushes, relabels, entries_read, kernel_launches, readbacks};
    for (int i = 0; i < 8; ++i)
        if (out[i]) *out[i] = v[i];
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_maxflow_phase_trace(grx_maxflow *p, int max_phases, int *kind, long long *rounds, double *ms)
{
    if (!p) return -1;
    return p->runner->PhaseTrace(max_phases, kind, rounds, ms);
}

long long grx_maxflow_pairs(grx_maxflow *p, int *h_a, int *h_b, int *h_cap_ab, int *h_cap_ba)
{
    if (!p) return -1;
    long long count = 0;
    const hipError_t rc = p->runner->Pairs(h_a, h_b, h_cap_ab, h_cap_ba, &count);
    return rc ? -static_cast<long long>(rc) : count;
}

int grx_maxflow_extract(grx_maxflow *p, long long *value, int *h_flow, unsigned char *h_side, unsigned char *h_cut)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(value, h_flow, h_side, h_cut));
}

int grx_maxflow_arc_flow(grx_maxflow *p, int *h_arc_flow)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->ArcFlow(h_arc_flow));
}

int grx_maxflow_summary(grx_maxflow *p, long long out[6])
{
    if (!p || !out) return -1;
    Summary s;
    const hipError_t rc = p->runner->GetSummary(&s);
    if (rc) return static_cast<int>(rc);
    out[0] = s.value;
    out[1] = s.side0;
    out[2] = s.side1;
    out[3] = s.side2;
    out[4] = s.cut0;
    out[5] = s.cut1;
    return 0;
}

int grx_maxflow_device_results(grx_maxflow *p, int **d_flow, unsigned char **d_side, unsigned char **d_cut, int **d_a, int **d_b, long long **d_excess,
                               int **d_height)
{
    if (!p) return -1;
    void *out[7];
    p->runner->DeviceResults(out);
    if (d_flow) *d_flow = static_cast<int *>(out[0]);
    if (d_side) *d_side = static_cast<unsigned char *>(out[1]);
    if (d_cut) *d_cut = static_cast<unsigned char *>(out[2]);
    if (d_a) *d_a = static_cast<int *>(out[3]);
    if (d_b) *d_b = static_cast<int *>(out[4]);
    if (d_excess) *d_excess = static_cast<long long *>(out[5]);
    if (d_height) *d_height = static_cast<int *>(out[6]);
    return 0;
}

void grx_maxflow_destroy(grx_maxflow *p) { delete p; }

}  // extern "C"
