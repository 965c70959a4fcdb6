// lib/mis_app.hip -- maximal independent set / greedy colouring entry points of libgunrock.so.
//  * grx_mis_*: MISProblem / MISEnactor phases as separate C calls (the reference has no C entry point for MIS; its driver is
//    tests/mis/test_mis.cu).  Extract follows MISProblem::Extract(h_mis_ids) (mis_problem.cuh:106): one int32 per vertex.
#include <gunrock/gunrock_mi355x.h>

#include <vector>

#include <gunrock/app/mis/mis_enactor.hpp>
#include <gunrock/app/mis/mis_problem.hpp>
#include <gunrock/app/handle_runner.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::mis;

static_assert(GRX_MIS_SET == MIS_SET && GRX_MIS_COLOR_ROUNDS == MIS_COLOR_ROUNDS && GRX_MIS_COLOR_FIRST_FIT == MIS_COLOR_FIRST_FIT,
              "the header's modes are the kernels' modes");

namespace {

struct MisRunner {
    InitState state;
    virtual ~MisRunner() {}
    virtual int Init(const Csr<int, int, int> &g, const int *priorities, unsigned seed) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_prio, unsigned seed) = 0;
    virtual void SetTail(bool on) = 0;
    virtual hipError_t Reset() = 0;
    virtual hipError_t Enact(int mode, int max_grid_size, float *ms) = 0;
    virtual void Stats(long long &rounds, long long &tail_sweeps, long long &entries, long long &polls, long long &launches, double &kernel_ms) = 0;
    virtual int Trace(int max_rounds, long long *entries, double *ms) = 0;
    virtual hipError_t Extract(int *ids, long long *summary) = 0;
    virtual int *DeviceIds() = 0;
};

template <bool INSTR>
struct MisRunnerT : MisRunner {
    typedef MISProblem<false> Problem;
    Problem problem;
    MISEnactor<INSTR> enactor;
    EventPair timer;
    explicit MisRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g, const int *priorities, unsigned seed) override
    {
        const hipError_t rc = problem.Init(false, g, priorities, seed, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_prio, unsigned seed) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci, d_prio, seed);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    void SetTail(bool on) override { enactor.use_tail = on; }
    hipError_t Reset() override { return state.ready ? problem.Reset() : hipErrorNotReady; }
    hipError_t Enact(int mode, int max_grid_size, float *ms) override
    {
        if (!state.ready) return hipErrorNotReady;
        return timer.Timed(problem.graph_slices[0]->stream, ms, [&]() { return enactor.template Enact<Problem>(&problem, mode, max_grid_size); });
    }
    void Stats(long long &rounds, long long &tail_sweeps, long long &entries, long long &polls, long long &launches, double &kernel_ms) override
    {
        rounds = enactor.rounds;
        tail_sweeps = enactor.tail_sweeps;
        entries = enactor.entries_read;
        polls = enactor.polls;
        launches = enactor.launches;
        kernel_ms = enactor.kernel_ms;
    }
    int Trace(int max_rounds, long long *entries, double *ms) override
    {
        return CopyTrace(enactor.trace.size(), max_rounds, Column(entries, [&](int i) { return enactor.trace[i].entries; }),
                         Column(ms, [&](int i) { return enactor.trace[i].ms; }));
    }
    hipError_t Extract(int *ids, long long *summary) override
    {
        if (!state.ready) return hipErrorNotReady;
        const hipError_t rc = problem.Extract(ids);
        if (summary) *summary = problem.summary;
        return rc;
    }
    int *DeviceIds() override { return state.ready ? problem.data_slices[0]->d_mis_ids : nullptr; }
};

}  // namespace

struct grx_mis {
    std::unique_ptr<MisRunner> runner;
};

extern "C" {

int grx_mis_create(grx_mis **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_mis{MakeRunner<MisRunner, MisRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_mis_init(grx_mis *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *priorities, unsigned seed)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices);
    return p->runner->Init(wrap.graph, priorities, seed);
}

int grx_mis_init_device(grx_mis *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_priorities, unsigned seed)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_priorities, seed);
}

int grx_mis_set_tail(grx_mis *p, int enable)
{
    if (!p) return -1;
    p->runner->SetTail(enable != 0);
    return 0;
}

int grx_mis_reset(grx_mis *p) { return p ? static_cast<int>(p->runner->Reset()) : -1; }

int grx_mis_enact(grx_mis *p, int mode, int max_grid_size, float *elapsed_ms)
{
    if (!p || mode < GRX_MIS_SET || mode > GRX_MIS_COLOR_FIRST_FIT) return -1;
    return static_cast<int>(p->runner->Enact(mode, max_grid_size, elapsed_ms));
}

int grx_mis_stats(grx_mis *p, long long *rounds, long long *tail_sweeps, long long *entries_read, long long *polls, long long *kernel_launches,
                  double *kernel_ms)
{
    if (!p) return -1;
    long long r = 0, t = 0, e = 0, q = 0, l = 0;
    double k = 0;
    p->runner->Stats(r, t, e, q, l, k);
    if (rounds) *rounds = r;
    if (tail_sweeps) *tail_sweeps = t;
    if (entries_read) *entries_read = e;
    if (polls) *polls = q;
    if (kernel_launches) *kernel_launches = l;
    if (kernel_ms) *kernel_ms = k;
    return 0;
}

int grx_mis_round_trace(grx_mis *p, int max_rounds, long long *vertices, double *ms)
{
    if (!p || max_rounds < 0) return -1;
    return p->runner->Trace(max_rounds, vertices, ms);
}

int grx_mis_extract(grx_mis *p, int *h_ids, long long *summary)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_ids, summary));
}

int grx_mis_device_results(grx_mis *p, int **d_ids)
{
    if (!p || !d_ids) return -1;
    *d_ids = p->runner->DeviceIds();
    return 0;
}

void grx_mis_destroy(grx_mis *p) { delete p; }

}  // extern "C"
