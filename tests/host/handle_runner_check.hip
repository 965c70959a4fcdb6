// The host-only pieces of gunrock/app/handle_runner.hpp -- BorrowedCsr, InitState, CopyTrace -- run on their own, without a
// GPU call, so that a host build with the address and undefined-behaviour sanitizers sees every free and every store they
// make (tests/test_handle_runner_host.py compiles and runs this file that way).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <gunrock/app/handle_runner.hpp>

using namespace gunrock;
using namespace gunrock::app;

namespace {

int failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// What a family's init does with a borrowed graph, with the early return a later edit might add.
int SumOrBail(const int *row_offsets, const int *col_indices, const int *edge_values, bool bail)
{
    BorrowedCsr<> wrap(3, 4, row_offsets, col_indices, edge_values);
    if (bail) return -1;
    int sum = 0;
    for (int v = 0; v < wrap.graph.nodes; ++v)
        for (int e = wrap.graph.row_offsets[v]; e < wrap.graph.row_offsets[v + 1]; ++e)
            sum += wrap.graph.column_indices[e] + (wrap.graph.edge_values ? wrap.graph.edge_values[e] : 0);
    return sum;
}

void BorrowedCsrLeavesTheCallersArrays()
{
    const int ro[4] = {0, 2, 3, 4}, ci[4] = {1, 2, 0, 0}, ev[4] = {5, 6, 7, 8};
    int *row_offsets = static_cast<int *>(std::malloc(sizeof(ro)));
    int *col_indices = static_cast<int *>(std::malloc(sizeof(ci)));
    int *edge_values = static_cast<int *>(std::malloc(sizeof(ev)));
    for (int i = 0; i < 4; ++i) {
        row_offsets[i] = ro[i];
        col_indices[i] = ci[i];
        edge_values[i] = ev[i];
    }
    {
        BorrowedCsr<> wrap(3, 4, row_offsets, col_indices);
        CHECK(wrap.graph.nodes == 3 && wrap.graph.edges == 4 && !wrap.graph.pinned);
        CHECK(wrap.graph.row_offsets == row_offsets && wrap.graph.column_indices == col_indices && !wrap.graph.edge_values);
    }
    {
        BorrowedCsr<float> wrap(3, 4, row_offsets, col_indices);  // the PageRank / BC value type
        CHECK(wrap.graph.row_offsets == row_offsets && !wrap.graph.edge_values && !wrap.graph.node_values);
    }
    CHECK(SumOrBail(row_offsets, col_indices, edge_values, false) == 3 + 26);
    CHECK(SumOrBail(row_offsets, col_indices, nullptr, false) == 3);
    CHECK(SumOrBail(row_offsets, col_indices, edge_values, true) == -1);
    // the arrays are still the caller's: readable, and freed exactly once, here
    for (int i = 0; i < 4; ++i) CHECK(row_offsets[i] == ro[i] && col_indices[i] == ci[i] && edge_values[i] == ev[i]);
    std::free(row_offsets);
    std::free(col_indices);
    std::free(edge_values);
}

// A one-graph family's init as its *_app.hip writes it: refuse a second graph, else admit what the problem's Init gave.
int Init(InitState &state, hipError_t rc, bool malformed)
{
    if (int taken = state.Taken()) return taken;
    return state.AdmitCode(rc, malformed);
}

void InitStateGivesTheAbiCodes()
{
    {
        InitState s;
        CHECK(!s.used && !s.ready && s.Taken() == 0);
        CHECK(Init(s, hipErrorInvalidValue, true) == -2);  // a malformed graph
        CHECK(s.used && !s.ready);
        CHECK(Init(s, hipSuccess, false) == -3);  // a handle takes one graph, also after a rejection
        CHECK(s.used && !s.ready);
    }
    {
        InitState s;
        CHECK(Init(s, hipSuccess, false) == 0);
        CHECK(s.used && s.ready);
        CHECK(Init(s, hipSuccess, false) == -3);
        CHECK(s.ready);  // the refusal leaves the first graph in place
    }
    {
        InitState s;
        CHECK(Init(s, hipErrorOutOfMemory, false) == static_cast<int>(hipErrorOutOfMemory));  // not the graph's fault: the error itself
        CHECK(s.used && !s.ready);
    }
    {
        InitState s;  // MST: no refusal, a later init decides
        CHECK(s.AdmitCode(hipErrorInvalidValue, true) == -2 && !s.ready);
        CHECK(s.AdmitCode(hipSuccess, false) == 0 && s.ready);
        CHECK(s.Admit(hipErrorInvalidValue) == hipErrorInvalidValue && !s.ready);
    }
}

void CopyTraceStopsAtMax()
{
    struct Record {
        long long entries;
        double ms;
    };
    const std::vector<Record> trace = {{10, 0.5}, {20, 1.5}, {30, 2.5}};
    auto entries_of = [&](int i) { return trace[i].entries; };
    auto ms_of = [&](int i) { return trace[i].ms; };
    // the sizing call: nothing to write to
    CHECK(CopyTrace(trace.size(), 0, Column(static_cast<long long *>(nullptr), entries_of), Column(static_cast<double *>(nullptr), ms_of)) == 3);
    // two entries into arrays that are two entries long (heap, so that a third store is seen)
    long long *entries = static_cast<long long *>(std::malloc(2 * sizeof(long long)));
    double *ms = static_cast<double *>(std::malloc(2 * sizeof(double)));
    CHECK(CopyTrace(trace.size(), 2, Column(entries, entries_of), Column(ms, ms_of)) == 3);
    CHECK(entries[0] == 10 && entries[1] == 20 && ms[0] == 0.5 && ms[1] == 1.5);
    // one column missing: the other is still written
    entries[0] = entries[1] = -1;
    CHECK(CopyTrace(trace.size(), 2, Column(entries, entries_of), Column(static_cast<double *>(nullptr), ms_of)) == 3);
    CHECK(entries[0] == 10 && entries[1] == 20);
    // max beyond the trace: the trace's length bounds the copy
    entries[0] = entries[1] = -1;
    CHECK(CopyTrace(2, 100, Column(entries, entries_of)) == 2);
    CHECK(entries[0] == 10 && entries[1] == 20);
    // an empty trace
    CHECK(CopyTrace(0, 2, Column(entries, entries_of), Column(ms, ms_of)) == 0);
    CHECK(CopyTrace(0, 0, Column(static_cast<int *>(nullptr), entries_of)) == 0);
    std::free(entries);
    std::free(ms);
}

}  // namespace

int main()
{
    BorrowedCsrLeavesTheCallersArrays();
    InitStateGivesTheAbiCodes();
    CopyTraceStopsAtMax();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("handle_runner host checks passed\n");
    return 0;
}
