// lib/matching_app.hip -- heavy-edge matching and graph contraction entry points of libgunrock.so.
//  * grx_matching_*: MatchingProblem / MatchingEnactor phases as separate C calls (the reference snapshot has no matching; the
//    calls are shaped like grx_maxflow_*).  Every per-pair array is indexed by the canonical pair id (grx_matching_pairs).
#include <gunrock/gunrock_mi355x.h>

#include <cstring>

#include <gunrock/app/handle_runner.hpp>
#include <gunrock/app/matching/matching_enactor.hpp>
#include <gunrock/app/matching/matching_problem.hpp>
#include <gunrock/csr.hpp>

using namespace gunrock;
using namespace gunrock::app;
using namespace gunrock::app::matching;

static_assert(GRX_MATCHING_AUTO == MATCHING_AUTO && GRX_MATCHING_ROUNDS == MATCHING_ROUNDS && GRX_MATCHING_DEVICE_LOOP == MATCHING_DEVICE_LOOP,
              "the header's schedules are the enactor's schedules");
static_assert(GRX_MATCHING_STEP_WIDE == STEP_WIDE && GRX_MATCHING_STEP_LOOP == STEP_LOOP, "the header's step kinds are the enactor's");
static_assert(GRX_MATCHING_GAVE_UP == kGaveUp && GRX_MATCHING_OVERFLOW == kOverflow, "the header's codes are the enactor's and the problem's");

namespace {

struct MatchingRunner {
    InitState state;
    virtual ~MatchingRunner() {}
    virtual int Init(const Csr<int, int, int> &g, unsigned seed) = 0;
    virtual int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_w, unsigned seed) = 0;
    virtual int SetOption(const char *name, double value) = 0;
    virtual int Reset() = 0;
    virtual int Enact(int max_grid_size, float *ms) = 0;
    virtual void Stats(long long *out, double &kernel_ms, double &build_ms) = 0;
    virtual int RoundTrace(int max_steps, int *kind, long long *rounds, long long *list, long long *matched) = 0;
    virtual hipError_t Pairs(int *src, int *dst, int *weight, long long *count) = 0;
    virtual hipError_t Extract(unsigned char *in, int *mate, int *medge) = 0;
    virtual hipError_t GetSummary(Summary *out) = 0;
    virtual void DeviceResults(void **out) = 0;
    virtual int Contract(const int *vertex_weights, long long *nodes, long long *entries) = 0;
    virtual hipError_t CoarseExtract(int *map, int *ro, int *ci, int *w, int *vweight) = 0;
    virtual int CoarseDevice(void **out) = 0;
};

template <bool INSTR>
struct MatchingRunnerT : MatchingRunner {
    typedef MatchingProblem<false> Problem;
    Problem problem;
    MatchingEnactor<INSTR> enactor;
    EventPair timer;
    explicit MatchingRunnerT(int device) : enactor(false)
    {
        util::GRError(hipSetDevice(device), "hipSetDevice failed", __FILE__, __LINE__);
        timer.Create();
    }
    int Init(const Csr<int, int, int> &g, unsigned seed) override
    {
        const hipError_t rc = problem.Init(false, g, seed, 1);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int InitDevice(int nodes, int edges, int *d_ro, int *d_ci, int *d_w, unsigned seed) override
    {
        const hipError_t rc = problem.InitFromDevice(nodes, edges, d_ro, d_ci, d_w, seed);
        return state.AdmitCode(rc, problem.malformed != 0);
    }
    int SetOption(const char *name, double value) override
    {
        if (!(value == value)) return -1;  // (NaN)
        const int shared = enactor.loop.Set(name, value, MATCHING_DEVICE_LOOP);
        if (shared != 1) return shared;
        const long long v = Whole(value);
        if (!std::strcmp(name, "max_rounds")) {
            if (v < 0 || v > kMaxMaxRounds) return -1;  // (0: back to the derived bound)
            enactor.max_rounds = v;
        } else {
            return 1;
        }
        return 0;
    }
    bool Done() const { return state.ready && problem.enacted; }
    int Reset() override
    {
        if (!state.ready) return static_cast<int>(hipErrorNotReady);
        return static_cast<int>(problem.Reset());
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
        out[2] = enactor.loop_rounds;
        out[3] = enactor.entries_read;
        out[4] = enactor.polls;
        out[5] = enactor.step.launches;
        kernel_ms = enactor.step.kernel_ms;
        build_ms = problem.build_ms;
    }
    int RoundTrace(int max_steps, int *kind, long long *rounds, long long *list, long long *matched) override
    {
        return CopyTrace(enactor.trace_kind.size(), max_steps, Column(kind, [&](int i) { return enactor.trace_kind[i]; }),
                         Column(rounds, [&](int i) { return enactor.trace_rounds[i]; }), Column(list, [&](int i) { return enactor.trace_list[i]; }),
                         Column(matched, [&](int i) { return enactor.trace_matched[i]; }));
    }
    hipError_t Pairs(int *src, int *dst, int *weight, long long *count) override
    {
        if (!state.ready) return hipErrorNotReady;
        *count = problem.pairs;
        return problem.Pairs(src, dst, weight);
    }
    hipError_t Extract(unsigned char *in, int *mate, int *medge) override { return Done() ? problem.Extract(in, mate, medge) : hipErrorNotReady; }
    hipError_t GetSummary(Summary *out) override
    {
        if (!Done()) return hipErrorNotReady;
        *out = problem.summary;
        return hipSuccess;
    }
    void DeviceResults(void **out) override
    {
        typename Problem::DataSlice *ds = state.ready ? problem.data_slices[0] : nullptr;
        for (int i = 0; i < 6; ++i) out[i] = nullptr;
        if (ds) {
            void *have[6] = {ds->d_in, ds->d_mate, ds->d_pp, ds->d_src, ds->d_dst, ds->d_pw};
            for (int i = 0; i < 6; ++i) out[i] = have[i];
        }
    }
    int Contract(const int *vertex_weights, long long *nodes, long long *entries) override
    {
        if (!Done()) return -1;
        // the vertex weights may be the caller's host array or a device array (the vweight of a level before)
        util::DeviceArray<int> d_upload;
        const int *d_vw = vertex_weights;
        if (vertex_weights) {
            hipPointerAttribute_t attr;
            const hipError_t known = hipPointerGetAttributes(&attr, vertex_weights);
            if (known != hipSuccess) (void)hipGetLastError();  // (a plain host pointer is no error here)
            if (known != hipSuccess || attr.type != hipMemoryTypeDevice) {
                const size_t bytes = sizeof(int) * static_cast<size_t>(problem.nodes);
                hipError_t rc = d_upload.Alloc(static_cast<size_t>(problem.nodes));
                if (rc == hipSuccess) rc = hipMemcpy(d_upload, vertex_weights, bytes, hipMemcpyHostToDevice);
                if (rc != hipSuccess) return static_cast<int>(rc);
                d_vw = d_upload;
            }
        }
        bool overflow = false;
        const hipError_t rc = problem.Contract(d_vw, &overflow);
        if (rc) return static_cast<int>(rc);
        if (overflow) return kOverflow;
        if (nodes) *nodes = problem.coarse_nodes;
        if (entries) *entries = problem.coarse_entries;
        return 0;
    }
    hipError_t CoarseExtract(int *map, int *ro, int *ci, int *w, int *vweight) override
    {
        if (!Done() || problem.coarse_nodes < 0) return hipErrorNotReady;
        return problem.CoarseExtract(map, ro, ci, w, vweight);
    }
    int CoarseDevice(void **out) override
    {
        for (int i = 0; i < 5; ++i) out[i] = nullptr;
        if (!Done() || problem.coarse_nodes < 0) return static_cast<int>(hipErrorNotReady);
        typename Problem::DataSlice *ds = problem.data_slices[0];
        void *have[5] = {ds->d_map, ds->d_cro, ds->d_cci, ds->d_cw, ds->d_vweight};
        for (int i = 0; i < 5; ++i) out[i] = have[i];
        return 0;
    }
};

}  // namespace

struct grx_matching {
    std::unique_ptr<MatchingRunner> runner;
};

extern "C" {

int grx_matching_create(grx_matching **out, int instrument, int device)
{
    if (!out) return -1;
    *out = new grx_matching{MakeRunner<MatchingRunner, MatchingRunnerT>(instrument != 0, device)};
    return 0;
}

int grx_matching_init(grx_matching *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights, unsigned seed)
{
    if (!p || !row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    BorrowedCsr<> wrap(nodes, edges, row_offsets, col_indices, weights);
    return p->runner->Init(wrap.graph, seed);
}

int grx_matching_init_device(grx_matching *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights, unsigned seed)
{
    if (!p || !d_row_offsets || nodes < 1 || edges < 0) return -1;
    if (edges > 0 && !d_col_indices) return -1;
    if (int taken = p->runner->state.Taken()) return taken;
    return p->runner->InitDevice(nodes, edges, d_row_offsets, d_col_indices, d_weights, seed);
}

int grx_matching_set_option(grx_matching *p, const char *name, double value)
{
    if (!p || !name) return -1;
    return p->runner->SetOption(name, value);
}

int grx_matching_reset(grx_matching *p) { return p ? p->runner->Reset() : -1; }

int grx_matching_enact(grx_matching *p, int max_grid_size, float *elapsed_ms)
{
    if (!p) return -1;
    return p->runner->Enact(max_grid_size, elapsed_ms);
}

int grx_matching_stats(grx_matching *p, long long *pairs, long long *rounds, long long *loop_rounds, long long *entries_read, long long *polls,
                       long long *kernel_launches, double *kernel_ms, double *build_ms)
{
    if (!p) return -1;
    long long v[6] = {0, 0, 0, 0, 0, 0};
    double k = 0, b = 0;
    p->runner->Stats(v, k, b);
    long long *out[6] = {pairs, rounds, loop_rounds, entries_read, polls, kernel_launches};
    for (int i = 0; i < 6; ++i)
        if (out[i]) *out[i] = v[i];
    if (kernel_ms) *kernel_ms = k;
    if (build_ms) *build_ms = b;
    return 0;
}

int grx_matching_round_trace(grx_matching *p, int max_steps, int *kind, long long *rounds, long long *list, long long *matched)
{
    if (!p) return -1;
    return p->runner->RoundTrace(max_steps, kind, rounds, list, matched);
}

long long grx_matching_pairs(grx_matching *p, int *h_src, int *h_dst, int *h_weight)
{
    if (!p) return -1;
    long long count = 0;
    const hipError_t rc = p->runner->Pairs(h_src, h_dst, h_weight, &count);
    return rc ? -static_cast<long long>(rc) : count;
}

int grx_matching_extract(grx_matching *p, unsigned char *h_in_matching, int *h_mate, int *h_medge)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->Extract(h_in_matching, h_mate, h_medge));
}

int grx_matching_summary(grx_matching *p, long long out[5])
{
    if (!p || !out) return -1;
    Summary s;
    const hipError_t rc = p->runner->GetSummary(&s);
    if (rc) return static_cast<int>(rc);
    out[0] = s.pairs;
    out[1] = s.matched;
    out[2] = s.weight;
    out[3] = s.unmatched;
    out[4] = s.unmatched_with_neighbours;
    return 0;
}

int grx_matching_device_results(grx_matching *p, unsigned char **d_in_matching, int **d_mate, int **d_medge, int **d_src, int **d_dst, int **d_weight)
{
    if (!p) return -1;
    void *out[6];
    p->runner->DeviceResults(out);
    if (d_in_matching) *d_in_matching = static_cast<unsigned char *>(out[0]);
    if (d_mate) *d_mate = static_cast<int *>(out[1]);
    if (d_medge) *d_medge = static_cast<int *>(out[2]);
    if (d_src) *d_src = static_cast<int *>(out[3]);
    if (d_dst) *d_dst = static_cast<int *>(out[4]);
    if (d_weight) *d_weight = static_cast<int *>(out[5]);
    return 0;
}

int grx_matching_contract(grx_matching *p, const int *vertex_weights, long long *coarse_nodes, long long *coarse_entries)
{
    if (!p) return -1;
    return p->runner->Contract(vertex_weights, coarse_nodes, coarse_entries);
}

int grx_matching_coarse_extract(grx_matching *p, int *h_map, int *h_row_offsets, int *h_col_indices, int *h_weights, int *h_vweight)
{
    if (!p) return -1;
    return static_cast<int>(p->runner->CoarseExtract(h_map, h_row_offsets, h_col_indices, h_weights, h_vweight));
}

int grx_matching_coarse_device(grx_matching *p, int **d_map, int **d_row_offsets, int **d_col_indices, int **d_weights, int **d_vweight)
{
    if (!p) return -1;
    void *out[5];
    const int rc = p->runner->CoarseDevice(out);
    if (d_map) *d_map = static_cast<int *>(out[0]);
    if (d_row_offsets) *d_row_offsets = static_cast<int *>(out[1]);
    if (d_col_indices) *d_col_indices = static_cast<int *>(out[2]);
    if (d_weights) *d_weights = static_cast<int *>(out[3]);
    if (d_vweight) *d_vweight = static_cast<int *>(out[4]);
    return rc;
}

void grx_matching_destroy(grx_matching *p) { delete p; }

}  // extern "C"
