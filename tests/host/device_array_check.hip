// gunrock/util/device_array.hpp and the slice holder of gunrock/app/problem_base.hpp run on their own, without a GPU call: the
// arrays live in host memory through a counting malloc / free, so that a host build with the address and undefined-behaviour
// sanitizers sees every free they make, and the count of live blocks says whether each happened once
// (tests/test_device_array_host.py compiles and runs this file that way).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
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
    CHECK(Mem::live == 0 && Mem::mallocs == Mem::frees);
    if (failures) {
        std::fprintf(stderr, "%d device_array host checks failed\n", failures);
        return 1;
    }
    std::printf("device_array host checks passed (%d blocks, all freed)\n", Mem::mallocs);
    return 0;
}
