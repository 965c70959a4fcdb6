// gunrock/util/device_array.hpp and the slice holder and frontier storage of gunrock/app/problem_base.hpp run on their own, without
// a GPU call: the arrays live in host memory through a counting malloc / free, so that a host build with the address and undefined-behaviour
// sanitizers sees every free they make, and the count of live blocks says whether each happened once
// (tests/test_device_array_host.py compiles and runs this file that way).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/pair_graph.hpp>
#include <gunrock/util/device_array.hpp>

using namespace gunrock;

namespace {

int failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

struct CountingHostMem {
    static int live, mallocs, frees;
    static hipError_t Malloc(void **p, size_t bytes)
    {
        *p = std::malloc(bytes);
        if (!*p) return hipErrorOutOfMemory;
        ++live;
        ++mallocs;
        return hipSuccess;
    }
    static hipError_t Free(void *p)
    {
        std::free(p);
        --live;
        ++frees;
        return hipSuccess;
    }
};
int CountingHostMem::live = 0, CountingHostMem::mallocs = 0, CountingHostMem::frees = 0;

// the same blocks and counts, but Malloc number `fail_at` after the last Arm fails (0: none does)
struct FailingHostMem {
    static int calls, fail_at;
    static void Arm(int nth)
    {
        calls = 0;
        fail_at = nth;
    }
    static hipError_t Malloc(void **p, size_t bytes)
    {
        if (++calls == fail_at) {
            *p = nullptr;
            return hipErrorOutOfMemory;
        }
        return CountingHostMem::Malloc(p, bytes);
    }
    static hipError_t Free(void *p) { return CountingHostMem::Free(p); }
};
int FailingHostMem::calls = 0, FailingHostMem::fail_at = 0;

template <typename T>
using Array = util::DeviceArray<T, CountingHostMem>;
typedef CountingHostMem Mem;

void ScopeExitFreesOnce()
{
    const int frees = Mem::frees;
    {
        Array<int> a;
        CHECK(!a && a.p == nullptr);
        CHECK(a.Alloc(5) == hipSuccess);
        CHECK(a && Mem::live == 1);
        for (int i = 0; i < 5; ++i) a[i] = i;  // (through the conversion to int *)
        CHECK(*(a + 4) == 4);
    }
    CHECK(Mem::live == 0 && Mem::frees == frees + 1);
}

void SecondAllocFreesTheFirstBlock()
{
    const int frees = Mem::frees;
    Array<long long> a;
    CHECK(a.Alloc(3) == hipSuccess);
    a[2] = 7;
    CHECK(a.Alloc(9) == hipSuccess);
    CHECK(Mem::live == 1 && Mem::frees == frees + 1);
    a[8] = 1;
}

void AllocOfNothingIsOneElement()
{
    Array<double> a;
    CHECK(a.Alloc(0) == hipSuccess);
    CHECK(a.p != nullptr && Mem::live == 1);
    a[0] = 0.5;
    CHECK(a[0] == 0.5);
}

void MoveLeavesTheSourceEmpty()
{
    const int frees = Mem::frees;
    {
        Array<int> a;
        CHECK(a.Alloc(4) == hipSuccess);
        int *block = a.p;
        Array<int> b(std::move(a));
        CHECK(a.p == nullptr && b.p == block && Mem::live == 1);
        Array<int> c;
        CHECK(c.Alloc(2) == hipSuccess);
        c = std::move(b);  // (c's own block goes here)
        CHECK(b.p == nullptr && c.p == block && Mem::live == 1 && Mem::frees == frees + 1);
        c[3] = 3;
    }
    CHECK(Mem::live == 0 && Mem::frees == frees + 2);
}

void AdoptOwnsWhatTakeGaveUp()
{
    const int frees = Mem::frees;
    void *raw = nullptr;
    CHECK(Mem::Malloc(&raw, sizeof(int) * 6) == hipSuccess);
    int *d_src = static_cast<int *>(raw);  // (as a PairGraph holds its result)
    {
        Array<int> a;
        a.Adopt(graphio::Take(d_src));
        CHECK(d_src == nullptr && a.p == raw && Mem::live == 1);
        a[5] = 5;
    }
    CHECK(Mem::live == 0 && Mem::frees == frees + 1);
}

void ReleaseHandsBackUnfreed()
{
    const int frees = Mem::frees;
    int *raw = nullptr;
    {
        Array<int> a;
        CHECK(a.Alloc(2) == hipSuccess);
        raw = a.Release();
        CHECK(a.p == nullptr && raw != nullptr);
    }
    CHECK(Mem::live == 1 && Mem::frees == frees);
    raw[1] = 1;
    CHECK(Mem::Free(raw) == hipSuccess);
}

void FreeTwiceIsHarmless()
{
    const int frees = Mem::frees;
    Array<unsigned char> a;
    CHECK(a.Alloc(16) == hipSuccess);
    a.Free();
    a.Free();
    CHECK(a.p == nullptr && Mem::live == 0 && Mem::frees == frees + 1);
    a.Free();  // (and so is freeing what never held anything)
    Array<int> never;
    never.Free();
    CHECK(Mem::frees == frees + 1);
}

// the shape of a problem's slice, and a build that stops where a malformed graph stops it
struct Slice {
    Array<int> d_src, d_dst;
    Array<int> d_list[2];
    Array<unsigned long long> d_words;
    Array<unsigned char> d_mask;  // allocated at the first request
    int *d_view = nullptr;        // points into d_src
};

hipError_t Build(Slice *ds, bool malformed)
{
    hipError_t retval = hipSuccess;
    if ((retval = ds->d_words.Alloc(4))) return retval;
    if (malformed) return hipErrorInvalidValue;
    if ((retval = ds->d_src.Alloc(8))) return retval;
    if ((retval = ds->d_list[1].Alloc(8))) return retval;
    ds->d_view = ds->d_src + 2;
    return retval;
}

void APartlyBuiltSliceFreesWhatItAllocated()
{
    for (int malformed = 0; malformed < 2; ++malformed) {
        const int mallocs = Mem::mallocs, frees = Mem::frees;
        app::SliceHolder<Slice> data_slices;
        CHECK(!data_slices && data_slices[0] == nullptr);
        data_slices.Make();
        CHECK(data_slices && data_slices[0] != nullptr);
        CHECK(Build(data_slices[0], malformed != 0) == (malformed ? hipErrorInvalidValue : hipSuccess));
        CHECK(Mem::mallocs - mallocs == (malformed ? 1 : 3) && Mem::live == Mem::mallocs - mallocs);
        if (!malformed) data_slices[0]->d_view[0] = 1;
        data_slices.Make();  // (a second one: the first goes with all it held)
        CHECK(Mem::live == 0 && Mem::frees - frees == Mem::mallocs - mallocs);
        CHECK(data_slices[0]->d_mask.Alloc(3) == hipSuccess);
    }
    CHECK(Mem::live == 0);
}

void AHolderNeverMadeGoesCleanly()
{
    const int frees = Mem::frees;
    {
        app::SliceHolder<Slice> data_slices;
        CHECK(!data_slices);
    }
    CHECK(Mem::frees == frees && Mem::live == 0);
}

// ---- a frontier queue: the view kernels take, and the three arrays beside it ----
void AFrontierGrowsByThreeBlocks()
{
    const int mallocs = Mem::mallocs, frees = Mem::frees;
    {
        app::FrontierStorage<int, int, Mem> q;
        CHECK(q.view.v == nullptr && q.view.capacity == 0);
        CHECK(q.Grow(8) == hipSuccess);
        CHECK(Mem::live == 3 && Mem::mallocs == mallocs + 3 && q.view.capacity == 8);
        int *old_v = q.view.v, *old_row_start = q.view.row_start, *old_scan = q.view.scan;
        CHECK(old_v == q.v.p && old_row_start == q.row_start.p && old_scan == q.scan.p);
        q.view.v[7] = q.view.row_start[7] = q.view.scan[7] = 7;
        CHECK(q.Grow(4) == hipSuccess);  // (room enough: nothing moves)
        CHECK(Mem::mallocs == mallocs + 3 && Mem::frees == frees && q.view.v == old_v && q.view.capacity == 8);
        CHECK(q.Grow(16) == hipSuccess);  // exactly three blocks go and three come
        CHECK(Mem::live == 3 && Mem::mallocs == mallocs + 6 && Mem::frees == frees + 3 && q.view.capacity == 16);
        CHECK(q.view.v == q.v.p && q.view.row_start == q.row_start.p && q.view.scan == q.scan.p);
        q.view.v[15] = q.view.row_start[15] = q.view.scan[15] = 15;  // (the new blocks: ASan would see the old ones)
        const util::Frontier<int, int> by_value = q.view;             // (as a kernel takes it)
        CHECK(by_value.v == q.v.p && Mem::live == 3);
    }
    CHECK(Mem::live == 0 && Mem::frees == frees + 6);
}

void AGrowThatFailsLeavesAnEmptyQueue()
{
    for (int failing = 1; failing <= 3; ++failing) {  // the first, second and third allocation of the grow
        const int start = Mem::live;
        {
            app::FrontierStorage<int, int, FailingHostMem> q;
            FailingHostMem::Arm(0);
            CHECK(q.Grow(8) == hipSuccess && Mem::live == start + 3);
            FailingHostMem::Arm(failing);
            CHECK(q.Grow(16) == hipErrorOutOfMemory);
            CHECK(Mem::live == start);  // no block leaks: the new ones and the old queue are gone, each freed once
            CHECK(q.view.v == nullptr && q.view.row_start == nullptr && q.view.scan == nullptr && q.view.capacity == 0);
            CHECK(q.v.p == nullptr && q.row_start.p == nullptr && q.scan.p == nullptr);
            FailingHostMem::Arm(0);
            CHECK(q.Grow(16) == hipSuccess);  // the next Reset tries again
            CHECK(Mem::live == start + 3 && q.view.capacity == 16 && q.view.scan == q.scan.p);
            q.view.scan[15] = 1;
        }
        CHECK(Mem::live == start);
    }
}

// ---- the shape of GraphSlice: raw views of its own arrays (a host CSR uploaded) or of the caller's (already on the device) ----
struct GraphShape {
    int *d_row_offsets = nullptr, *d_column_indices = nullptr;
    Array<int> own_row_offsets, own_column_indices;
};

hipError_t InitOwned(app::SliceHolder<GraphShape> &graph_slices, int nodes, int edges)
{
    hipError_t retval = hipSuccess;
    GraphShape *gs = graph_slices.Make();
    if ((retval = gs->own_row_offsets.Alloc(nodes + 1))) return retval;
    if ((retval = gs->own_column_indices.Alloc(edges))) return retval;
    gs->d_row_offsets = gs->own_row_offsets;
    gs->d_column_indices = gs->own_column_indices;
    return retval;
}

void InitBorrowed(app::SliceHolder<GraphShape> &graph_slices, int *d_row_offsets, int *d_column_indices)
{
    GraphShape *gs = graph_slices.Make();
    gs->d_row_offsets = d_row_offsets;
    gs->d_column_indices = d_column_indices;
}

void AGraphSliceFreesItsOwnArraysAndNoBorrowedOnes()
{
    Array<int> caller_offsets, caller_columns;
    CHECK(caller_offsets.Alloc(5) == hipSuccess && caller_columns.Alloc(3) == hipSuccess);
    const int frees = Mem::frees;
    {
        app::SliceHolder<GraphShape> graph_slices;
        CHECK(InitOwned(graph_slices, 4, 3) == hipSuccess);
        CHECK(Mem::live == 4 && graph_slices[0]->d_row_offsets == graph_slices[0]->own_row_offsets.p);
        graph_slices[0]->d_row_offsets[4] = 3;
        InitBorrowed(graph_slices, caller_offsets, caller_columns);  // re-making the slice frees the first: its two arrays, once
        CHECK(Mem::live == 2 && Mem::frees == frees + 2);
        CHECK(graph_slices[0]->d_row_offsets == caller_offsets.p && graph_slices[0]->own_row_offsets.p == nullptr);
        CHECK(InitOwned(graph_slices, 4, 0) == hipSuccess);  // (and back: the borrowed arrays stay the caller's)
        CHECK(Mem::live == 4 && Mem::frees == frees + 2);
        InitBorrowed(graph_slices, caller_offsets, caller_columns);
        CHECK(Mem::live == 2 && Mem::frees == frees + 4);
    }
    CHECK(Mem::live == 2 && Mem::frees == frees + 4);  // the borrowing slice went and freed nothing
    caller_offsets[4] = caller_columns[2] = 1;         // (still the caller's to use)
}

// ---- the shape of BFS, CC, SSSP, BC and PageRank: a slice of raw pointers, copied by value into kernel arguments, over owners
// held beside it in the problem ----
struct ViewSlice {
    int *d_labels = nullptr;
    unsigned *d_mask = nullptr;  // allocated at the first request
    int iteration = 0;
};
static_assert(std::is_trivially_copyable<ViewSlice>::value, "a kernel argument");

struct ViewProblem {
    app::SliceHolder<ViewSlice> data_slices;
    Array<int> d_labels;
    Array<unsigned> d_mask;
    hipError_t AllocData(int nodes)
    {
        hipError_t retval = hipSuccess;
        ViewSlice *ds = data_slices.Make();
        d_mask.Free();
        if ((retval = d_labels.Alloc(nodes))) return retval;
        ds->d_labels = d_labels;
        return retval;
    }
    hipError_t EnsureMask(int words)
    {
        hipError_t retval = hipSuccess;
        ViewSlice *ds = data_slices[0];
        if (ds->d_mask) return retval;
        if ((retval = d_mask.Alloc(words))) return retval;
        ds->d_mask = d_mask;
        return retval;
    }
};

void OwnersBesideASliceOfViews()
{
    const int mallocs = Mem::mallocs, frees = Mem::frees;
    {
        ViewProblem problem;
        CHECK(problem.AllocData(8) == hipSuccess && problem.EnsureMask(2) == hipSuccess && problem.EnsureMask(2) == hipSuccess);
        CHECK(Mem::live == 2 && Mem::mallocs == mallocs + 2);
        ViewSlice slice = *problem.data_slices[0];  // by value, as the enactors and the functors take it
        slice.iteration = 3;
        slice.d_labels[7] = 7;
        ViewSlice again = slice;
        CHECK(again.d_labels == problem.d_labels.p && again.d_mask == problem.d_mask.p);
        CHECK(Mem::live == 2 && Mem::mallocs == mallocs + 2 && Mem::frees == frees);  // copies change no counts
        CHECK(problem.AllocData(16) == hipSuccess);  // a second init on one problem: the first arrays go
        CHECK(Mem::live == 1 && Mem::frees == frees + 2 && problem.data_slices[0]->d_mask == nullptr);
        CHECK(problem.EnsureMask(4) == hipSuccess && Mem::live == 2);
        problem.data_slices[0]->d_labels[15] = problem.data_slices[0]->d_mask[3] = 1;
    }
    CHECK(Mem::live == 0 && Mem::mallocs - mallocs == Mem::frees - frees);
}

void ANeverInitialisedViewProblemGoesCleanly()
{
    const int frees = Mem::frees;
    {
        ViewProblem problem;
        CHECK(!problem.data_slices && problem.d_labels.p == nullptr);
    }
    CHECK(Mem::frees == frees && Mem::live == 0);
}

// ---- a build with scratch of its own scope, left at each of its checks ----
hipError_t BuildWithScratch(Array<int> &d_kept, int stop_at)
{
    hipError_t retval = hipSuccess;
    Array<unsigned> d_counts;
    Array<unsigned long long> d_sums;
    if (stop_at == 0) return hipErrorInvalidValue;
    if ((retval = d_counts.Alloc(9))) return retval;
    if (stop_at == 1) return hipErrorInvalidValue;
    if ((retval = d_sums.Alloc(3))) return retval;
    if (stop_at == 2) return hipErrorInvalidValue;
    {
        Array<int> d_replacement;  // the half-built array that replaces a member (CC's compact froms)
        if ((retval = d_replacement.Alloc(4))) return retval;
        if (stop_at == 3) return hipErrorInvalidValue;
        d_replacement[3] = static_cast<int>(d_counts[8] = 3u);
        d_kept = std::move(d_replacement);
    }
    if (stop_at == 4) return hipErrorInvalidValue;
    d_sums[2] = 2;
    return retval;
}

void ABuildLeftEarlyLeaksNoScratch()
{
    Array<int> d_kept;
    CHECK(d_kept.Alloc(12) == hipSuccess);
    const int start = Mem::live;
    for (int stop_at = 0; stop_at <= 5; ++stop_at) {
        CHECK(BuildWithScratch(d_kept, stop_at) == (stop_at < 5 ? hipErrorInvalidValue : hipSuccess));
        CHECK(Mem::live == start);  // the scratch is gone; the kept array is the old one or the new one, never both
    }
    CHECK(d_kept[3] == 3);
}

}  // namespace

int main()
{
    ScopeExitFreesOnce();
    SecondAllocFreesTheFirstBlock();
    CHECK(Mem::live == 0);
    AllocOfNothingIsOneElement();
    CHECK(Mem::live == 0);
    MoveLeavesTheSourceEmpty();
    AdoptOwnsWhatTakeGaveUp();
    ReleaseHandsBackUnfreed();
    FreeTwiceIsHarmless();
    APartlyBuiltSliceFreesWhatItAllocated();
    AHolderNeverMadeGoesCleanly();
    AFrontierGrowsByThreeBlocks();
    AGrowThatFailsLeavesAnEmptyQueue();
    AGraphSliceFreesItsOwnArraysAndNoBorrowedOnes();
    CHECK(Mem::live == 0);
    OwnersBesideASliceOfViews();
    ANeverInitialisedViewProblemGoesCleanly();
    ABuildLeftEarlyLeaksNoScratch();
    CHECK(Mem::live == 0 && Mem::mallocs == Mem::frees);
    if (failures) {
        std::fprintf(stderr, "%d device_array host checks failed\n", failures);
        return 1;
    }
    std::printf("device_array host checks passed (%d blocks, all freed)\n", Mem::mallocs);
    return 0;
}
