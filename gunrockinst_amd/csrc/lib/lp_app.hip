// lib/lp_app.hip -- label-propagation entry points of libgunrock.so.
//  * grx_lp_*: LpProblem / LpEnactor phases as separate C calls (the reference snapshot has no label propagation; the calls are
//    shaped like grx_matching_*).  Per-community arrays are indexed by the dense community id of grx_lp_extract.
#include <gunrock/gunrock_mi355x.h>

#include <cstring>
#include <vector>

#include <gunrock/app/handle_runner.hpp>
#include <gunrock/app/lp/lp_enactor.hpp>
#include <gunrock/app/lp/lp_problem.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::lp;

static_assert(GRX_LP_SYNC == LP_SYNC && GRX_LP_CLASSES == LP_CLASSES, "the header's modes are the enactor's modes");
static_assert(GRX_LP_AUTO == LP_AUTO && GRX_LP_LANE == LP_LANE && GRX_LP_WAVE == LP_WAVE && GRX_LP_BLOCK == LP_BLOCK,
              "the header's strategies are the enactor's strategies");
static_assert(GRX_LP_CONVERGED == LP_CONVERGED && GRX_LP_PERIOD2 == LP_PERIOD2 && GRX_LP_CAPPED == LP_CAPPED, "the header's states are the enactor's");
static_assert(GRX_LP_BAD_CLASSES == kBadClasses, "the header's code is the problem's");

namespace {

struct LpRunner {
    InitState state;
    virtual ~LpRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_w) = 0;
    virtual int SetClasses(const int *classes, int count) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int Reset(const int *labels) = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms, double &build_ms) = 0;
    virtual int RoundTrace(int max_rounds, long long *list, long long *changed) = 0;
    virtual hipError_t Extract(int *labels, int *community, long long *communities) = 0;
    virtual hipError_t Summary(long long *size, long long *internal, long long *volume, long long *total) = 0;
    virtual void DeviceResults(void **out) = 0;
};

template <bool INSTR>
struct LpRunnerT : LpRunner {
    typedef LpProblem<false> Problem;
    Problem problem;
    LpEnactor<INSTR> enactor;
    EventPair timer;
    explicit LpRunnerT(int device) : enactor(false)
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
    int SetClasses(const int *classes, int count) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        if (count < 1 || count > problem.nodes) return -1;
        for (int v = 0; v < problem.nodes; ++v)
            if (classes[v] < 0 || classes[v] >= count) return -1;
        bool improper = false;
        const hipError_t rc = problem.SetClasses(classes, count, &improper);
        if (rc) return static_cast<int>(rc);
        return improper ? kBadClasses : 0;
    }
    int SetOption(const char *name, double value) override
    {
        if (!(value == value)) return -1;  // (NaN)
        const long long v = value >= 9.0e18 ? LLONG_MAX : (value <= -9.0e18 ? LLONG_MIN : static_cast<long long>(value));
        if (!std::strcmp(name, "mode")) {
            if (v < LP_SYNC || v > LP_CLASSES) return -1;
            enactor.mode = static_cast<int>(v);
        } else if (!std::strcmp(name, "strategy")) {
            if (v < LP_AUTO || v > LP_BLOCK) return -1;
            enactor.strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "lane_max_row")) {
            if (v < 0) return -1;
            enactor.lane_max_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "wave_max_row")) {
            if (v < 0) return -1;
            enactor.wave_max_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "table_slots")) {
            if (v < kMinTableSlots || v > kTableSlots || (v & (v - 1))) return -1;
            enactor.table_slots = static_cast<int>(v);
        } else if (!std::strcmp(name, "max_rounds")) {
            if (v < 0 || v > kMaxMaxRounds) return -1;  // (0: back to the default)
            enactor.max_rounds = v;
        } else {
            return 1;
        }
        return 0;
    }
    bool Done() const { return state.ready && problem.enacted; }
    int Reset(const int *labels) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        if (labels)
            for (int v = 0; v < problem.nodes; ++v)
                if (labels[v] < 0 || labels[v] >= problem.nodes) return -1;
        return static_cast<int>(problem.Reset(labels));
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        return static_cast<int>(
            timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); }));
    }
    void Stats(long long *out, double &kernel_ms, double &build_ms) override
    {
        out[0] = problem.pairs;
        out[1] = enactor.rounds;
        out[2] = enactor.state;
        out[3] = enactor.visits;
        out[4] = enactor.entries_read;
        for (int i = 0; i < 3; ++i) out[5 + i] = enactor.regime_rows[i];
        out[8] = enactor.fallback_rows;
        out[9] = enactor.step.launches;
        out[10] = enactor.step.readbacks;
        kernel_ms = enactor.step.kernel_ms;
        build_ms = problem.build_ms;
    }
    int RoundTrace(int max_rounds, long long *list, long long *changed) override
    {
        return CopyTrace(enactor.trace_list.size(), max_rounds, Column(list, [&](int i) { return enactor.trace_list[i]; }),
                         Column(changed, [&](int i) { return enactor.trace_changed[i]; }));
    }
    hipError_t Extract(int *labels, int *community, long long *communities) override
    {
        if (!Done()) return hipErrorNotReady;
        if (communities) *communities = problem.communities;
        return problem.Extract(labels, community);
    }
    hipError_t Summary(long long *size, long long *internal, long long *volume, long long *total) override
    {
        return Done() ? problem.Summary(size, internal, volume, total) : hipErrorNotReady;
    }
    void DeviceResults(void **out) override
    {
        typename Problem::DataSlice *ds = state.ready ? problem.data_slices[0] : nullptr;
        out[0] = ds ? ds->d_labels : nullptr;
        out[1] = ds ? ds->d_community : nullptr;
    }
};

}  // namespace

struct grx_lp {
    std::unique_ptr<LpRunner> runner;
};

extern "C" {

int grx_lp_create(grx_lp **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_lp{MakeRunner<LpRunner, LpRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_lp_init(grx_lp *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices, weights);
    return p->runner->Init(wrap.graph);
}

int grx_lp_init_device(grx_lp *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_weights);
}

int grx_lp_set_classes(grx_lp *p, const int *classes, int num_classes)
{
    if (!p || !classes) return -1;
    return p->runner->SetClasses(classes, num_classes);
}

int grx_lp_set_option(grx_lp *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_lp_reset(grx_lp *p, const int *labels) { return p ? p->runner->Reset(labels) : -1; }

int grx_lp_enact(grx_lp *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_lp_stats(grx_lp *p, long long *pairs, long long *rounds, long long *state, long long *visits, long long *entries_read, long long *regime_rows,
                 long long *fallback_rows, long long *kernel_launches, long long *readbacks, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    long long v[11] = {0};
    double k = 0, b = 0;
    p->runner->Stats(v, k, b);
    if (pairs) *pairs = v[0];
    if (rounds) *rounds = v[1];
    if (state) *state = v[2];
    if (visits) *visits = v[3];
    if (entries_read) *entries_read = v[4];
    if (regime_rows)
        for (int i = 0; i < 3; ++i) regime_rows[i] = v[5 + i];
    if (fallback_rows) *fallback_rows = v[8];
    if (kernel_launches) *kernel_launches = v[9];
    if (readbacks) *readbacks = v[10];
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_lp_round_trace(grx_lp *p, int max_rounds, long long *list, long long *changed)
{
    if (!p) return -1;
    return p->runner->RoundTrace(max_rounds, list, changed);
}

int grx_lp_extract(grx_lp *p, int *h_labels, int *h_community, long long *communities)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_labels, h_community, communities));
}

int grx_lp_summary(grx_lp *p, long long *h_size, long long *h_internal, long long *h_volume, long long *total_weight)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Summary(h_size, h_internal, h_volume, total_weight));
}

int grx_lp_device_results(grx_lp *p, int **d_labels, int **d_community)
{
    if (!p) return -1;
    void *out[2];
    p->runner->DeviceResults(out);
    if (d_labels) *d_labels = static_cast<int *>(out[0]);
    if (d_community) *d_community = static_cast<int *>(out[1]);
    return 0;
}

void grx_lp_destroy(grx_lp *p) { delete p; }

}  // extern "C"
