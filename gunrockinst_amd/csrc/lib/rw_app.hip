// lib/rw_app.hip -- random-walk entry points of libgunrock.so.
//  * grx_rw_*: RwProblem / RwEnactor phases as separate C calls (the reference snapshot has no random walks; the calls are shaped
//    like grx_c4_*).  Reset takes the start vertices, Extract gives the walks, their lengths, the visits and the steps taken.
#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/rw/rw_enactor.hpp>
#include <gunrock/app/rw/rw_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::rw;

static_assert(GRX_RW_AUTO == RW_AUTO && GRX_RW_LANE == RW_LANE && GRX_RW_TILE == RW_TILE, "the header's strategies are the kernels' strategies");
static_assert(sizeof(long long) == sizeof(unsigned long long) && sizeof(long long) == 8, "visits and steps are 64-bit");

namespace {

struct RwStats {
    long long walks = 0, steps = 0, ended = 0, tries = 0, forced = 0, launches = 0;
    double kernel_ms = 0, build_ms = 0;
};

struct RwRunner {
    InitState state;
    bool started = false;   // a Reset gave start vertices
    bool finished = false;  // the last Enact ran to its end: there is a result to extract
    virtual ~RwRunner() {}
    virtual int Init(const Csr<int, int, int> &g) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_w) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int Reset(int num_walks, const int *h_starts) = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(RwStats &s) = 0;
    virtual int Extract(int *walks, int *lengths, long long *visits, long long *steps) = 0;
    virtual void DeviceResults(int **d_walks, int **d_lengths, long long **d_visits, long long *pitch) = 0;
};

template <bool INSTR>
struct RwRunnerT : RwRunner {
    typedef RwProblem<false> Problem;
    Problem problem;
    RwEnactor<INSTR> enactor;
    EventPair timer;
    explicit RwRunnerT(int device) : enactor(false)
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
    int Reset(int num_walks, const int *h_starts) override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        for (int w = 0; w < num_walks; ++w)
            if (h_starts[w] < 0 || h_starts[w] >= problem.nodes) return -1;
        finished = false;
        started = false;
        const hipError_t rc = problem.Reset(num_walks, h_starts);
        started = rc == hipSuccess;
        return static_cast<int>(rc);
    }
    int Enact(int max_grid_size, float *ms) override
    {
        if (!state.ready || !started) return static_cast<int>(hipErrorNotReady);
        finished = false;
        const hipError_t rc = timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, max_grid_size); });
        if (rc) return static_cast<int>(rc);
        finished = true;
        return 0;
    }
    void Stats(RwStats &s) override
    {
        s.walks = finished ? problem.num_walks : 0;
        s.steps = enactor.steps;
        s.ended = enactor.ended;
        s.tries = enactor.tries;
        s.forced = enactor.forced;
        s.launches = enactor.host.launches;
        s.kernel_ms = enactor.host.kernel_ms;
        s.build_ms = problem.build_ms;
    }
    int Extract(int *walks, int *lengths, long long *visits, long long *steps) override
    {
        if (!state.ready || !finished) return static_cast<int>(hipErrorNotReady);
        if (visits && !enactor.with_visits) return -1;
        if (steps) *steps = enactor.steps;
        return static_cast<int>(problem.Extract(enactor.length, walks, lengths, visits));
    }
    void DeviceResults(int **d_walks, int **d_lengths, long long **d_visits, long long *pitch) override
    {
        typename Problem::DataSlice *ds = state.ready && finished ? problem.data_slices[0] : nullptr;
        if (d_walks) *d_walks = ds ? ds->d_walks : nullptr;
        if (d_lengths) *d_lengths = ds ? ds->d_lengths : nullptr;
        if (d_visits) *d_visits = ds && enactor.with_visits ? reinterpret_cast<long long *>(ds->d_visits.p) : nullptr;
        if (pitch) *pitch = ds ? problem.pitch : 0;
    }
};

}  // namespace

struct grx_rw {
    std::unique_ptr<RwRunner> runner;
};

extern "C" {

int grx_rw_create(grx_rw **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_rw{MakeRunner<RwRunner, RwRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_rw_init(grx_rw *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices, weights);
    return p->runner->Init(wrap.graph);
}

int grx_rw_init_device(grx_rw *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_weights);
}

int grx_rw_set_option(grx_rw *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_rw_reset(grx_rw *p, int num_walks, const int *h_starts)
{
    if (!p || num_walks < 1 || !h_starts) return -1;
    return p->runner->Reset(num_walks, h_starts);
}

int grx_rw_enact(grx_rw *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_rw_stats(grx_rw *p, long long *walks, long long *steps, long long *ended_early, long long *biased_tries, long long *forced_fallbacks,
                 long long *kernel_launches, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    RwStats s;
    p->runner->Stats(s);
    if (walks) *walks = s.walks;
    if (steps) *steps = s.steps;
    if (ended_early) *ended_early = s.ended;
    if (biased_tries) *biased_tries = s.tries;
    if (forced_fallbacks) *forced_fallbacks = s.forced;
    if (kernel_launches) *kernel_launches = s.launches;
    if (kernel_ms) *kernel_ms = s.kernel_ms;
    if (build_ms) *build_ms = s.build_ms;
    return 0;
}

int grx_rw_extract(grx_rw *p, int *h_walks, int *h_lengths, long long *h_visits, long long *steps)
{
    if (!p) return -1;
    return p->runner->Extract(h_walks, h_lengths, h_visits, steps);
}

int grx_rw_device_results(grx_rw *p, int **d_walks, int **d_lengths, long long **d_visits, long long *walks_pitch)
{
    if (!p) return -1;
    p->runner->DeviceResults(d_walks, d_lengths, d_visits, walks_pitch);
    return 0;
}

void grx_rw_destroy(grx_rw *p) { delete p; }

}  // extern "C"
