// lib/wl_app.hip -- colour-refinement entry points of libgunrock.so.
//  * grx_wl_*: WlProblem / WlEnactor phases as separate C calls (the reference snapshot has no colour refinement; the calls are
//    shaped like grx_lp_*).  Per-class arrays are indexed by the dense colour of grx_wl_extract.
#include <gunrock/gunrock_mi355x.h>

#include <cstring>
#include <vector>

#include <gunrock/app/handle_runner.hpp>
#include <gunrock/app/wl/wl_enactor.hpp>
#include <gunrock/app/wl/wl_problem.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::wl;

static_assert(GRX_WL_AUTO == WL_AUTO && GRX_WL_LANE == WL_LANE && GRX_WL_WAVE == WL_WAVE && GRX_WL_BLOCK == WL_BLOCK,
              "the header's strategies are the enactor's strategies");
static_assert(GRX_WL_STABLE == WL_STABLE && GRX_WL_CAPPED == WL_CAPPED, "the header's states are the enactor's");
static_assert(GRX_WL_TOO_LARGE == kTooLarge && GRX_WL_NOT_CERTIFIED == kNotCertified, "the header's codes are the enactor's");

namespace {

struct WlRunner {
    InitState state;
    virtual ~WlRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int Reset(const int *labels) = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms) = 0;
    virtual int RoundTrace(int max_rounds, long long *classes) = 0;
    virtual int Extract(int *colour, long long *size, int *representative, long long *classes) = 0;
    virtual int History(int round, int *colour, long long *classes) = 0;
    virtual void DeviceResults(void **out) = 0;
};

template <bool INSTR>
struct WlRunnerT : WlRunner {
    typedef WlProblem<false> Problem;
    Problem problem;
    WlEnactor<INSTR> enactor;
    EventPair timer;
    explicit WlRunnerT(int device) : enactor(false)
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
    int SetOption(const char *name, double value) override { return enactor.options.Set(name, value); }
    bool Done() const { return state.ready && problem.enacted; }
    int Reset(const int *labels) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        return static_cast<int>(problem.Reset(labels));
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        const hipError_t rc = timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
        return rc ? static_cast<int>(rc) : enactor.code;
    }
    void Stats(long long *out, double &kernel_ms) override
    {
        out[0] = state.ready ? problem.edges : 0;
        out[1] = enactor.rounds;
        out[2] = enactor.state;
        out[3] = enactor.classes;
        out[4] = enactor.repairs;
        out[5] = enactor.certificate_runs;
        for (int i = 0; i < 3; ++i) out[6 + i] = enactor.regime_rows[i];
        for (int i = 0; i < 3; ++i) out[9 + i] = enactor.rung_rows[i];
        out[12] = enactor.step.launches;
        out[13] = enactor.step.readbacks;
        kernel_ms = enactor.step.kernel_ms;
    }
    int RoundTrace(int max_rounds, long long *classes) override
    {
        return CopyTrace(enactor.trace_classes.size(), max_rounds, Column(classes, [&](int i) { return enactor.trace_classes[i]; }));
    }
    int Extract(int *colour, long long *size, int *representative, long long *classes) override
    {
        if (!Done()) return static_cast<int>(hipErrorNotReady);
        if (classes) *classes = problem.classes;
        return static_cast<int>(problem.Extract(colour, size, representative));
    }
    int History(int round, int *colour, long long *classes) override
    {
        if (!Done() || problem.history_rounds < 0) return static_cast<int>(hipErrorNotReady);
        if (round < 0 || round > problem.history_rounds) return -1;
        return static_cast<int>(problem.History(round, colour, classes));
    }
    void DeviceResults(void **out) override
    {
        typename Problem::DataSlice *ds = Done() ? problem.data_slices[0] : nullptr;
        out[0] = ds ? ds->d_dense : nullptr;
        out[1] = ds ? ds->d_size : nullptr;
        out[2] = ds ? ds->d_representative : nullptr;
    }
};

}  // namespace

struct grx_wl {
    std::unique_ptr<WlRunner> runner;
};

extern "C" {

int grx_wl_create(grx_wl **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_wl{MakeRunner<WlRunner, WlRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_wl_init(grx_wl *p, int nodes, int edges, const int *row_offsets, const int *col_indices)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph);
}

int grx_wl_init_device(grx_wl *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices);
}

int grx_wl_set_option(grx_wl *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_wl_reset(grx_wl *p, const int *labels) { return p ? p->runner->Reset(labels) : -1; }

int grx_wl_enact(grx_wl *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_wl_stats(grx_wl *p, long long *entries, long long *rounds, long long *state, long long *classes, long long *repairs,
                 long long *certificate_runs, long long *regime_rows, long long *rung_rows, long long *kernel_launches, long long *readbacks,
                 double *kernel_ms)
{
    if (!p) return -1;
    long long v[14] = {0};
    double k = 0;
    p->runner->Stats(v, k);
    if (entries) *entries = v[0];
    if (rounds) *rounds = v[1];
    if (state) *state = v[2];
    if (classes) *classes = v[3];
    if (repairs) *repairs = v[4];
    if (certificate_runs) *certificate_runs = v[5];
    if (regime_rows)
        for (int i = 0; i < 3; ++i) regime_rows[i] = v[6 + i];
    if (rung_rows)
        for (int i = 0; i < 3; ++i) rung_rows[i] = v[9 + i];
    if (kernel_launches) *kernel_launches = v[12];
    if (readbacks) *readbacks = v[13];
    if (kernel_ms) *kernel_ms = k;
    return 0;
}

int grx_wl_round_trace(grx_wl *p, int max_rounds, long long *classes)
{
    if (!p) return -1;
    return p->runner->RoundTrace(max_rounds, classes);
}

int grx_wl_extract(grx_wl *p, int *h_colour, long long *h_class_size, int *h_representative, long long *classes)
{
    if (!p) return -1;
    return p->runner->Extract(h_colour, h_class_size, h_representative, classes);
}

int grx_wl_history(grx_wl *p, int round, int *h_colour, long long *classes)
{
    if (!p) return -1;
    return p->runner->History(round, h_colour, classes);
}

int grx_wl_device_results(grx_wl *p, int **d_colour, long long **d_class_size, int **d_representative)
{
    if (!p) return -1;
    void *out[3];
    p->runner->DeviceResults(out);
    if (d_colour) *d_colour = static_cast<int *>(out[0]);
    if (d_class_size) *d_class_size = static_cast<long long *>(out[1]);
    if (d_representative) *d_representative = static_cast<int *>(out[2]);
    return 0;
}

void grx_wl_destroy(grx_wl *p) { delete p; }

}  // extern "C"
