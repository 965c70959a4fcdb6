// app/spgemm/spgemm_functor.hpp -- device kernels of the sparse product C = A B with exact int64 values.
//
// The reference snapshot has no SpGEMM; the shape follows this tree's table primitives (c4, sim): Gustavson's row-wise product on the
// LANE / WAVE / BLOCK / GLOBAL ladder of app/table_ladder.hpp over the open-addressed table of oprtr/lds_table.hpp.
//
// A is rows x inner, B is inner x cols, both CSR read as given: duplicates add, a row in any order, values int32 or absent (= 1).  Row i
// of C is the sum over the entries (i, k, a) of A of a times row k of B: w_i = the sum of len(B[k]) products.  C is structural (the
// GraphBLAS rule): (i, j) is stored when some k has A(i, k) and B(k, j) stored, also when the products cancel to 0.  By w_i (Regime()):
//   LANE    w <= lane_max: one lane keeps a sorted list of at most 64 (column, sum) in private memory
//   WAVE    w <= table_slots / 2: one row per wave, a column -> sum table in the wave's part of LDS
//   BLOCK   w <= block_slots / 2: one workgroup per row, the workgroup's LDS as one table
//   GLOBAL  the rest: one workgroup per row and, per workgroup slot in global scratch, a dense int64[cols] accumulator row and a bitmap
//           of cols bits
// Three passes.  WorkKernel: w_i, its sum and largest, the bound on |C(i, j)| and the four row lists.  Symbolic (WRITE = false): the
// distinct columns of every row; an exclusive scan of them gives the offsets.  Numeric (WRITE = true): the same claims, 64-bit atomic
// adds into the value next to the key, the occupied slots ordered by column (a bitonic network over the table, empty sorting last) and
// written by consecutive lanes; GLOBAL drains its bitmap word by word, the popcount prefix of a word giving each set bit its place, and
// clears what it touched.  VALUES = false (pattern_only) leaves the values and the accumulator row out.
//
// Integer sums commute: every output has one value whatever the schedule, the order of a row of A or B, or who claimed a slot first.
// Nothing in a launch reads what the same launch writes, apart from atomics and a workgroup's own scratch slot behind a fence.  No kernel
// waits on another workgroup; every loop bound is a kernel argument, a constant or a value of the validated arrays.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include <gunrock/app/table_ladder.hpp>
#include <gunrock/graphio/rect_csr.hpp>
#include <gunrock/oprtr/lds_table.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace spgemm {

enum { SPGEMM_AUTO = 0, SPGEMM_LANE = 1, SPGEMM_WAVE = 2, SPGEMM_BLOCK = 3, SPGEMM_GLOBAL = 4 };  // "strategy"; 1 .. 4 are the regimes
static_assert(SPGEMM_WAVE == ladder::WAVE && SPGEMM_BLOCK == ladder::BLOCK && SPGEMM_GLOBAL == ladder::GLOBAL, "the ladder's rungs");
enum { SPGEMM_SELF = 0, SPGEMM_TRANSPOSE = 1, SPGEMM_GIVEN = 2 };  // "right"

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / util::kWaveSize;
constexpr int kLaneMax = 64;     // default and largest "lane_max": the private list of a lane
constexpr long long kSaturated = LLONG_MAX;

using ladder::kTableSlots;
using ladder::kMinTableSlots;
using ladder::kBlockSlots;
using ladder::kMinBlockSlots;
using ladder::kScratchMib;
using ladder::kMaxScratchMib;
using ladder::TableSize;

namespace lds = oprtr::lds;
using util::Fmix32;

// the 64-bit words the kernels and the host share
enum {
    W_PROBES = 0,   // table probes of the WAVE and BLOCK regimes, both passes
    W_NNZ,          // the distinct columns of all rows (symbolic pass)
    W_SUM,          // the sum of w_i
    W_MAX,          // the largest w_i
    W_BOUND,        // the largest bound of a row, saturating
    W_BAD,          // graphio::ValidateRectKernel: not a CSR
    W_LISTS,        // four words: the rows listed for LANE, WAVE, BLOCK, GLOBAL
    W_PRODUCTS = W_LISTS + 4,  // four words: their products
    W_COUNT = 16
};

struct Mat {
    const int *ro, *ci, *val;  // val may be NULL: every stored value is 1
    int rows, cols;
};

struct Ctx {
    Mat a, b;
    const long long *babs;  // the sum of |b| over every row of B, or NULL: the row's length
    unsigned long long *words;
    long long *work;  // w_i
    int *lists;       // 4 x a.rows
    int strategy, lane_max, table_slots, block_slots;
};

// what the passes write
struct Out {
    unsigned *count;     // symbolic: the distinct columns per row (all 0 before)
    const int *offsets;  // numeric: where a row starts
    int *cols;
    long long *vals;
};

// ---------------- rules the host shares ----------------

// The regime of a row with w products: LANE while it is short and nothing larger is forced, else the ladder's.
__host__ __device__ __forceinline__ int Regime(long long w, int strategy, int lane_max, int table_slots, int block_slots)
{
    if (strategy <= SPGEMM_LANE && w <= lane_max) return SPGEMM_LANE;
    return ladder::Widen(strategy < SPGEMM_WAVE ? SPGEMM_WAVE : strategy, w, table_slots, block_slots);
}

// a slot of a table: the int key, and the int64 sum when the pass has values
__host__ __device__ __forceinline__ size_t SlotBytes(bool values) { return values ? sizeof(int) + sizeof(long long) : sizeof(int); }
__host__ __device__ __forceinline__ size_t SmallLdsBytes(int table_slots, bool values)
{
    return SlotBytes(values) * static_cast<size_t>(kWaves) * static_cast<size_t>(table_slots);
}
__host__ __device__ __forceinline__ size_t BlockLdsBytes(int block_slots, bool values) { return SlotBytes(values) * static_cast<size_t>(block_slots); }
constexpr size_t kMaxBlockLdsBytes = (sizeof(int) + sizeof(long long)) * kBlockSlots;  // 96 KiB of the CU's 160

// a workgroup slot of the GLOBAL regime in 64-bit words: cols sums, then a bit per column
__host__ __device__ __forceinline__ long long BitmapWords(long long cols) { return (cols + 63) / 64; }
__host__ __device__ __forceinline__ long long SlotWords(long long cols) { return cols + BitmapWords(cols); }
// min(grid, scratch_mib 2^20 / (8 cols + cols / 8 rounded up to a word)), at least 1
__host__ __device__ __forceinline__ long long GlobalSlots(long long grid, long long scratch_mib, long long cols)
{
    long long slots = (scratch_mib << 20) / (8 * SlotWords(cols > 0 ? cols : 1));
    if (slots > grid) slots = grid;
    return slots < 1 ? 1 : slots;
}

// saturating int64 arithmetic on values >= 0
__host__ __device__ __forceinline__ long long SatAdd(long long a, long long b) { return a > kSaturated - b ? kSaturated : a + b; }
__host__ __device__ __forceinline__ long long SatMul(long long a, long long b)
{
    if (a == 0 || b == 0) return 0;
    return a > kSaturated / b ? kSaturated : a * b;
}
__host__ __device__ __forceinline__ long long Abs64(int v) { return v < 0 ? -static_cast<long long>(v) : static_cast<long long>(v); }

// what int32 addresses: the entries of C, and the products of one row (a group counts them in an int)
__host__ __device__ __forceinline__ bool Fits(long long nnz, long long max_row_products)
{
    return nnz >= 0 && nnz <= INT_MAX && max_row_products >= 0 && max_row_products <= INT_MAX;
}

// ---------------- validation and the build ----------------

// babs[k] = the sum of |b| over row k (below 2^62: at most 2^31 entries of at most 2^31)
static __global__ void RowAbsKernel(Mat b, long long *babs)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long k = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; k < b.rows; k += stride) {
        long long sum = 0;
        for (int f = b.ro[k]; f < b.ro[k + 1]; ++f) sum += Abs64(b.val[f]);
        babs[k] = sum;
    }
}

__device__ __forceinline__ unsigned long long WaveMax(unsigned long long x)
{
#pragma unroll
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor(static_cast<unsigned>(x >> 32), o, util::kWaveSize);
        const unsigned lo = __shfl_xor(static_cast<unsigned>(x), o, util::kWaveSize);
        const unsigned long long other = (static_cast<unsigned long long>(hi) << 32) | lo;
        x = other > x ? other : x;
    }
    return x;
}

// ---------------- the work pass ----------------

// One lane per row: w_i and the row's bound, sum over the entries (i, k, a) of |a| times the sum of |b| over row k, saturating; the
// row enters the list of its regime (a wave claims the places of its rows with one atomic per regime).
static __global__ __launch_bounds__(kThreads) void WorkKernel(Ctx c)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    const long long rows = c.a.rows;
    const long long groups = (rows + util::kWaveSize - 1) / util::kWaveSize;
    unsigned long long sum = 0, longest = 0, bound = 0;
    unsigned long long products[4] = {0, 0, 0, 0};
    for (long long g = wave0; g < groups; g += nwaves) {  // (wave-uniform)
        const long long i = g * util::kWaveSize + lane;
        const bool live = i < rows;
        long long w = 0, mine = 0;
        int regime = 0;
        if (live) {
            for (int e = c.a.ro[i]; e < c.a.ro[i + 1]; ++e) {
                const int k = c.a.ci[e];
                const long long len = c.b.ro[k + 1] - c.b.ro[k];
                w += len;
                mine = SatAdd(mine, SatMul(Abs64(c.a.val ? c.a.val[e] : 1), c.babs ? c.babs[k] : len));
            }
            c.work[i] = w;
            regime = Regime(w, c.strategy, c.lane_max, c.table_slots, c.block_slots);
            products[regime - 1] += static_cast<unsigned long long>(w);
            sum += static_cast<unsigned long long>(w);
            longest = static_cast<unsigned long long>(w) > longest ? static_cast<unsigned long long>(w) : longest;
            bound = static_cast<unsigned long long>(mine) > bound ? static_cast<unsigned long long>(mine) : bound;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned long long mask = __ballot(regime == r + 1);
            if (!mask) continue;
            const int leader = __ffsll(static_cast<long long>(mask)) - 1;
            unsigned base = 0;
            if (lane == leader) base = static_cast<unsigned>(atomicAdd(c.words + W_LISTS + r, static_cast<unsigned long long>(__popcll(mask))));
            base = __shfl(base, leader, util::kWaveSize);
            const long long at = static_cast<long long>(base) + util::RankInMask(mask);
            if (regime == r + 1 && at < rows) c.lists[static_cast<long long>(r) * rows + at] = static_cast<int>(i);
        }
    }
    sum = util::WaveSum(sum);
    longest = WaveMax(longest);
    bound = WaveMax(bound);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned long long p = util::WaveSum(products[r]);
        if (lane == 0 && p) atomicAdd(c.words + W_PRODUCTS + r, p);
    }
    if (lane == 0) {
        if (sum) atomicAdd(c.words + W_SUM, sum);
        if (longest) atomicMax(c.words + W_MAX, longest);
        if (bound) atomicMax(c.words + W_BOUND, bound);
    }
}

// the rows a regime's kernel was handed (a kernel boundary lies behind WorkKernel)
__device__ __forceinline__ long long Listed(const Ctx &c, int regime)
{
    const long long listed = static_cast<long long>(c.words[W_LISTS + regime - 1]);
    return listed > c.a.rows ? c.a.rows : listed;
}

// ---------------- LANE ----------------

// One lane per listed row: an insertion into a sorted private list of at most lane_max <= kLaneMax columns.
template <bool WRITE, bool VALUES>
static __global__ __launch_bounds__(kThreads) void LaneKernel(Ctx c, Out o)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long listed = Listed(c, SPGEMM_LANE);
    const int *list = c.lists;
    unsigned long long total = 0;
    for (long long at = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; at < listed; at += stride) {
        const int i = list[at];
        int key[kLaneMax];
        long long val[kLaneMax];
        int n = 0;
        for (int e = c.a.ro[i]; e < c.a.ro[i + 1]; ++e) {
            const int k = c.a.ci[e];
            const long long a = c.a.val ? c.a.val[e] : 1;
            for (int f = c.b.ro[k]; f < c.b.ro[k + 1]; ++f) {
                const int j = c.b.ci[f];
                int pos = 0;
                while (pos < n && key[pos] < j) ++pos;
                if (pos < n && key[pos] == j) {
                    if (VALUES) val[pos] += a * (c.b.val ? c.b.val[f] : 1);
                    continue;
                }
                if (n >= kLaneMax) continue;  // (never: n <= w <= lane_max; keeps a mistake inside the list)
                for (int s = n; s > pos; --s) {
                    key[s] = key[s - 1];
                    if (VALUES) val[s] = val[s - 1];
                }
                key[pos] = j;
                if (VALUES) val[pos] = a * (c.b.val ? c.b.val[f] : 1);
                ++n;
            }
        }
        if (!WRITE) {
            o.count[i] = static_cast<unsigned>(n);
            total += static_cast<unsigned long long>(n);
        } else {
            const int off = o.offsets[i];
            for (int s = 0; s < n; ++s) {
                o.cols[off + s] = key[s];
                if (VALUES) o.vals[off + s] = val[s];
            }
        }
    }
    if (!WRITE) {
        total = util::WaveSum(total);
        if (util::LaneId() == 0 && total) atomicAdd(c.words + W_NNZ, total);
    }
}

// ---------------- WAVE and BLOCK ----------------

// The `size` slots of a group's table ascending by key as unsigned (an empty slot, -1, sorts last), the values with them: a bitonic
// network, every compare-exchange by one thread, a GroupSync between two stages.  All threads of the group call; size is a power of two.
template <bool BLOCK, bool VALUES>
__device__ __forceinline__ void SortTable(int *key, long long *val, int size, int tid)
{
    constexpr int G = BLOCK ? kThreads : util::kWaveSize;
    for (int k = 2; k <= size; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < size / 2; t += G) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const unsigned x = static_cast<unsigned>(key[i]), y = static_cast<unsigned>(key[p]);
                if ((x > y) == ((i & k) == 0)) {
                    key[i] = static_cast<int>(y);
                    key[p] = static_cast<int>(x);
                    if (VALUES) {
                        const long long v = val[i];
                        val[i] = val[p];
                        val[p] = v;
                    }
                }
            }
            lds::GroupSync<BLOCK>();
        }
    }
}

// Row i by a wave (BLOCK = false) or by the workgroup, in the group's table key[] / val[] of `slots` slots.  The products are shared
// out in pieces of g lanes, g the power of two that covers the mean length of the B rows met: 64 / g entries of A at a time per wave.
template <bool BLOCK, bool WRITE, bool VALUES>
__device__ __forceinline__ void TableRow(const Ctx &c, const Out &o, int i, int *key, long long *val, int slots, unsigned long long &probes,
                                         unsigned long long &total)
{
    constexpr int G = BLOCK ? kThreads : util::kWaveSize;
    constexpr int WAVES = BLOCK ? kWaves : 1;
    const int tid = BLOCK ? static_cast<int>(threadIdx.x) : static_cast<int>(util::LaneId());
    const int lane = static_cast<int>(util::LaneId());
    const int wave = BLOCK ? static_cast<int>(threadIdx.x) / util::kWaveSize : 0;
    const long long w = c.work[i];
    const int ab = c.a.ro[i], alen = c.a.ro[i + 1] - ab;
    int off = 0, n = 0;
    if (WRITE) {
        off = o.offsets[i];
        n = o.offsets[i + 1] - off;
        if (n == 0) return;  // (uniform over the group)
    }
    // the symbolic pass knows w alone (at most w, at most cols distinct columns); the numeric pass knows the row's n of them
    const int size = TableSize(WRITE ? n : (w < c.b.cols ? w : c.b.cols), slots);
    lds::Clear<G>(key, size, tid, [&](int s) {
        if (VALUES) val[s] = 0;
    });
    lds::GroupSync<BLOCK>();
    int g = 1;
    while (g < util::kWaveSize && static_cast<long long>(g) * alen < w) g <<= 1;
    const int per = util::kWaveSize / g, sub = lane / g, l = lane & (g - 1);
    for (int e = wave * per + sub; e < alen; e += WAVES * per) {
        const int k = c.a.ci[ab + e];
        const long long a = c.a.val ? c.a.val[ab + e] : 1;
        const int bb = c.b.ro[k], bl = c.b.ro[k + 1] - bb;
        for (int f = l; f < bl; f += g) {
            const int j = c.b.ci[bb + f];
            const int at = lds::Claim(key, size, Fmix32(static_cast<unsigned>(j)), j, probes);
            if (VALUES && at >= 0)  // (always: the table never fills)
                atomicAdd(reinterpret_cast<unsigned long long *>(val + at), static_cast<unsigned long long>(a * (c.b.val ? c.b.val[bb + f] : 1)));
        }
    }
    lds::GroupSync<BLOCK>();
    if (!WRITE) {  // the fresh claims: the occupied slots
        int fresh = 0;
        for (int s = tid; s < size; s += G) fresh += key[s] >= 0;
        fresh = util::WaveSum(fresh);
        if (lane == 0 && fresh) {
            atomicAdd(o.count + i, static_cast<unsigned>(fresh));
            total += static_cast<unsigned long long>(fresh);
        }
    } else {
        SortTable<BLOCK, VALUES>(key, val, size, tid);
        for (int s = tid; s < n; s += G) {
            o.cols[off + s] = key[s];
            if (VALUES) o.vals[off + s] = val[s];
        }
    }
    lds::GroupSync<BLOCK>();  // (the next row clears what this one still reads)
}

// One wave per row of the WAVE list (BLOCK = false), one workgroup per row of the BLOCK list.  LDS: with VALUES the int64 sums of
// all tables first, then the keys; else the keys alone.
template <bool BLOCK, bool WRITE, bool VALUES>
static __global__ __launch_bounds__(kThreads) void TableKernel(Ctx c, Out o)
{
    extern __shared__ long long s_mem[];
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    const long long rows = c.a.rows;
    const long long listed = Listed(c, BLOCK ? SPGEMM_BLOCK : SPGEMM_WAVE);
    const int *list = c.lists + (BLOCK ? 2 : 1) * rows;
    const int slots = BLOCK ? c.block_slots : c.table_slots;
    const int tables = BLOCK ? 1 : kWaves, mine = BLOCK ? 0 : wave;
    long long *val = VALUES ? s_mem + static_cast<size_t>(mine) * slots : nullptr;
    int *key = (VALUES ? reinterpret_cast<int *>(s_mem + static_cast<size_t>(tables) * slots) : reinterpret_cast<int *>(s_mem)) +
               static_cast<size_t>(mine) * slots;
    unsigned long long probes = 0, total = 0;
    if (BLOCK) {
        for (long long at = blockIdx.x; at < listed; at += gridDim.x)  // (uniform over the workgroup)
            TableRow<true, WRITE, VALUES>(c, o, list[at], key, val, slots, probes, total);
    } else {
        const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
        const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
        for (long long at = wave0; at < listed; at += nwaves)  // (wave-uniform)
            TableRow<false, WRITE, VALUES>(c, o, list[at], key, val, slots, probes, total);
    }
    probes = util::WaveSum(probes);
    total = util::WaveSum(total);
    if (lane == 0) {
        if (probes) atomicAdd(c.words + W_PROBES, probes);
        if (total) atomicAdd(c.words + W_NNZ, total);
    }
}

// ---------------- GLOBAL ----------------

// One workgroup per row of the GLOBAL list, workgroup slot blockIdx.x of `scratch`: SlotWords(cols) 64-bit words, all 0 between two
// rows.  The host launches no more workgroups than there are slots.
template <bool WRITE, bool VALUES>
static __global__ __launch_bounds__(kThreads) void GlobalKernel(Ctx c, Out o, unsigned long long *scratch)
{
    __shared__ int s_count[kWaves];
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    const long long cols = c.b.cols, nwords = BitmapWords(cols);
    unsigned long long *acc = scratch + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(SlotWords(cols));
    unsigned long long *bits = acc + cols;
    const long long listed = Listed(c, SPGEMM_GLOBAL);
    const int *list = c.lists + 3 * static_cast<long long>(c.a.rows);
    // a wave drains a run of whole 64-word pieces of the bitmap
    const long long pieces = (nwords + util::kWaveSize - 1) / util::kWaveSize, share = (pieces + kWaves - 1) / kWaves;
    const long long first = wave * share * util::kWaveSize;
    const long long last = first + share * util::kWaveSize < nwords ? first + share * util::kWaveSize : nwords;
    unsigned long long total = 0;
    for (long long at = blockIdx.x; at < listed; at += gridDim.x) {  // (uniform over the workgroup)
        const int i = list[at];
        const int ab = c.a.ro[i], alen = c.a.ro[i + 1] - ab;
        for (int e = wave; e < alen; e += kWaves) {
            const int k = c.a.ci[ab + e];
            const long long a = c.a.val ? c.a.val[ab + e] : 1;
            const int bb = c.b.ro[k], bl = c.b.ro[k + 1] - bb;
            for (int f = lane; f < bl; f += util::kWaveSize) {
                const int j = c.b.ci[bb + f];
                // with values the bit follows the sum: whoever finds the sum 0 is the first at j, or comes behind sums that cancelled
                // (then the bit is set again, which changes nothing); behind a sum that is not 0 the first one has set it
                if (!VALUES || atomicAdd(acc + j, static_cast<unsigned long long>(a * (c.b.val ? c.b.val[bb + f] : 1))) == 0ull)
                    atomicOr(bits + (j >> 6), 1ull << (j & 63));
            }
        }
        lds::GlobalSync();
        // the set bits of this wave's run
        int mine = 0;
        for (long long s = first + lane; s < last; s += util::kWaveSize)
            mine += __popcll(__hip_atomic_load(bits + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        mine = util::WaveSum(mine);
        if (!WRITE) {
            for (long long s = first + lane; s < last; s += util::kWaveSize) bits[s] = 0ull;
            if (lane == 0 && mine) {
                atomicAdd(o.count + i, static_cast<unsigned>(mine));
                total += static_cast<unsigned long long>(mine);
            }
        } else {
            if (lane == 0) s_count[wave] = mine;
            __syncthreads();
            long long pos = o.offsets[i];
            for (int v = 0; v < wave; ++v) pos += s_count[v];
            for (long long s0 = first; s0 < last; s0 += util::kWaveSize) {  // (wave-uniform)
                const long long s = s0 + lane;
                const unsigned long long word = s < last ? __hip_atomic_load(bits + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
                unsigned long long todo = __ballot(word != 0ull);
                while (todo) {  // (wave-uniform) one word at a time, bit l by lane l
                    const int from = __ffsll(static_cast<long long>(todo)) - 1;
                    const unsigned hi = __shfl(static_cast<unsigned>(word >> 32), from, util::kWaveSize);
                    const unsigned lo = __shfl(static_cast<unsigned>(word), from, util::kWaveSize);
                    const unsigned long long set = (static_cast<unsigned long long>(hi) << 32) | lo;
                    if ((set >> lane) & 1ull) {
                        const long long j = (s0 + from) * 64 + lane;
                        const long long to = pos + __popcll(set & ((1ull << lane) - 1ull));
                        o.cols[to] = static_cast<int>(j);
                        if (VALUES) {
                            o.vals[to] = static_cast<long long>(__hip_atomic_load(acc + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                            acc[j] = 0ull;
                        }
                    }
                    pos += __popcll(set);
                    todo &= todo - 1;
                }
                if (word) bits[s] = 0ull;
            }
        }
        lds::GlobalSync();  // (the next row counts in the slot this one cleared; s_count is free again)
    }
    if (!WRITE) {
        total = util::WaveSum(total);
        if (lane == 0 && total) atomicAdd(c.words + W_NNZ, total);
    }
}

}  // namespace spgemm
}  // namespace app
}  // namespace gunrock
