// lib/blocks_app.hip -- the device building blocks under the operators, each on its own behind the C ABI
// (include/gunrock/gunrock_mi355x.h), so that they can be checked element by element without a primitive around them
// (tests/test_blocks_gpu.py; the precedents are grx_filter_queue and grx_advance_queue):
//
//  * grx_device_scan       graphio::DeviceExclusiveScan<int | unsigned | unsigned long long>, scratch of ScanScratchWords(n);
//  * grx_device_key_sort   ONE graphio::DeviceKeySort sorts a sequence of key arrays, as a problem's long-lived sorter does;
//  * grx_device_transpose  graphio::DeviceTransposeCsr, with or without a 32-bit value per edge;
//  * grx_wave_ops          one thread per element: load, call a block of util/device_intrinsics.hpp, store;
//  * grx_bisect_queue      priority_queue::Bisect with the SSSP enactor's own template arguments
//                          <256, 4, SSSPProblem<int, int, int, MARK_PATHS>, PQFunctor>.  The real DataSlice is a struct of raw
//                          pointers, so it is filled here from the caller's arrays; no problem object is built.
//
// Nothing here changes the code it calls: every function only allocates scratch, launches and copies back.
#include <gunrock/gunrock_mi355x.h>

#include <climits>
#include <type_traits>
#include <vector>

#include <gunrock/app/sssp/sssp_functor.hpp>
// (only the DataSlice of the problem header is used here; its extract kernel stays unreferenced)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include <gunrock/app/sssp/sssp_problem.hpp>
#pragma clang diagnostic pop
#include <gunrock/graphio/device_csr.hpp>
#include <gunrock/graphio/device_sort.hpp>
#include <gunrock/oprtr/advance/kernel.hpp>
#include <gunrock/priority_queue/kernel.hpp>
#include <gunrock/util/device_array.hpp>
#include <gunrock/util/device_intrinsics.hpp>
#include <gunrock/util/error_utils.hpp>
#include <gunrock/util/frontier.hpp>

using namespace gunrock;

namespace {

constexpr int kBadArgument = -1;
constexpr int kNotInstantiated = -2;

// ---- wave blocks: one struct per block, In -> Out ----
template <typename T>
struct OpInclusiveSum {
    typedef T In;
    typedef T Out;
    static __device__ __forceinline__ Out Run(In x, bool) { return util::WaveInclusiveSum(x); }
};
struct OpInclusiveSumDpp {
    typedef unsigned In;
    typedef unsigned Out;
    static __device__ __forceinline__ Out Run(In x, bool) { return util::WaveInclusiveSumDpp(x); }
};
struct OpInclusiveMaxDpp {
    typedef unsigned In;
    typedef unsigned Out;
    static __device__ __forceinline__ Out Run(In x, bool) { return util::WaveInclusiveMaxDpp(x); }
};
template <oprtr::advance::REDUCE_OP OP, typename T>
struct OpSegmentedScan {
    typedef T In;
    typedef T Out;
    static __device__ __forceinline__ Out Run(In x, bool head)
    {
        return util::WaveSegmentedScanDpp<oprtr::advance::ReduceOps<OP, T>, T>(head, x);
    }
};
template <typename T>
struct OpWaveSum {
    typedef T In;
    typedef T Out;
    static __device__ __forceinline__ Out Run(In x, bool) { return util::WaveSum(x); }
};
struct OpRankInMask {
    typedef unsigned long long In;
    typedef unsigned Out;
    static __device__ __forceinline__ Out Run(In mask, bool) { return util::RankInMask(mask); }
};
// the six (control, row mask) pairs of the scan network; lanes without a source show the identity pattern
template <int CTRL, int ROW_MASK, typename T>
struct OpDppMove {
    typedef T In;
    typedef T Out;
    static __device__ __forceinline__ Out Run(In x, bool)
    {
        return util::DppMove<CTRL, ROW_MASK, T>(static_cast<T>(GRX_DPP_MOVE_IDENTITY), x);
    }
};

// element i is thread i of the launch, i.e. lane i % 64 (workgroups are whole waves); threads past n take part with a zero
// and no head -- every block here is inclusive or a sum, so they change nothing a stored lane sees
template <typename Op>
__global__ __launch_bounds__(1024) void WaveOpKernel(const typename Op::In *d_in, const unsigned char *d_heads, long long n,
                                                     typename Op::Out *d_out)
{
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    typename Op::In x = typename Op::In();
    if (i < n) x = d_in[i];
    const bool head = d_heads != nullptr && i < n && d_heads[i] != 0;
    const typename Op::Out r = Op::Run(x, head);
    if (i < n) d_out[i] = r;
}

// two scans back to back on the same storage: the second takes the workgroup's elements in mirrored order.
// d_out[i] = first result, d_aux[i], d_aux[n + i], d_aux[2n + i] = first total, second result, second total of thread i
template <int THREADS, typename T>
__global__ __launch_bounds__(THREADS) void BlockScanKernel(const T *d_in, long long n, T *d_out, T *d_aux)
{
    typedef util::BlockScan<THREADS, T> Scan;
    __shared__ typename Scan::Storage s_scan;
    const long long base = static_cast<long long>(blockIdx.x) * THREADS;
    const long long i = base + threadIdx.x;
    const long long j = base + (THREADS - 1 - static_cast<int>(threadIdx.x));
    T x = 0, y = 0;
    if (i < n) x = d_in[i];
    if (j < n) y = d_in[j];
    T total1, total2;
    const T first = Scan::ExclusiveSum(x, total1, s_scan);
    const T second = Scan::ExclusiveSum(y, total2, s_scan);
    if (i < n) {
        d_out[i] = first;
        d_aux[i] = total1;
        d_aux[n + i] = second;
        d_aux[2 * n + i] = total2;
    }
}

struct WaveCall {
    int threads;
    long long n;
    const void *d_in;
    const unsigned char *d_heads;
    void *d_out;
    void *d_aux;
};

template <typename Op>
int RunWave(const WaveCall &c)
{
    const long long grid = (c.n + c.threads - 1) / c.threads;
    hipLaunchKernelGGL((WaveOpKernel<Op>), dim3(static_cast<unsigned>(grid)), dim3(c.threads), 0, 0,
                       static_cast<const typename Op::In *>(c.d_in), c.d_heads, c.n, static_cast<typename Op::Out *>(c.d_out));
    return static_cast<int>(util::GRError("WaveOpKernel launch failed", __FILE__, __LINE__));
}

template <typename T>
int RunBlockScan(const WaveCall &c)
{
    if (!c.d_aux) return kBadArgument;
    const long long grid = (c.n + c.threads - 1) / c.threads;
    const T *in = static_cast<const T *>(c.d_in);
    T *out = static_cast<T *>(c.d_out), *aux = static_cast<T *>(c.d_aux);
    if (c.threads == 64) hipLaunchKernelGGL((BlockScanKernel<64, T>), dim3(static_cast<unsigned>(grid)), dim3(64), 0, 0, in, c.n, out, aux);
    else if (c.threads == 256) hipLaunchKernelGGL((BlockScanKernel<256, T>), dim3(static_cast<unsigned>(grid)), dim3(256), 0, 0, in, c.n, out, aux);
    else hipLaunchKernelGGL((BlockScanKernel<1024, T>), dim3(static_cast<unsigned>(grid)), dim3(1024), 0, 0, in, c.n, out, aux);
    return static_cast<int>(util::GRError("BlockScanKernel launch failed", __FILE__, __LINE__));
}

// every (REDUCE_OP, value type) the library hands to WaveSegmentedScanDpp through advance::LaunchReduce (lib/oprtr_app.hip lists
// them; BC, PageRank and SSSP use PLUS float, PLUS int and MINIMUM unsigned / unsigned long long), but for float MULTIPLIES:
// the blocks are checked exactly, and a float product is exact only for chosen factors
template <typename T, bool ARITH32, bool BITS>
int DispatchSegmented(int r_op, const WaveCall &c)
{
    using namespace oprtr::advance;
    switch (r_op) {
        case GRX_REDUCE_PLUS: return RunWave<OpSegmentedScan<PLUS, T>>(c);
        case GRX_REDUCE_MAXIMUM: return RunWave<OpSegmentedScan<MAXIMUM, T>>(c);
        case GRX_REDUCE_MINIMUM: return RunWave<OpSegmentedScan<MINIMUM, T>>(c);
        case GRX_REDUCE_MULTIPLIES:
            if constexpr (ARITH32) return RunWave<OpSegmentedScan<MULTIPLIES, T>>(c);
            break;
        case GRX_REDUCE_BIT_OR:
            if constexpr (BITS) return RunWave<OpSegmentedScan<BIT_OR, T>>(c);
            break;
        case GRX_REDUCE_BIT_AND:
            if constexpr (BITS) return RunWave<OpSegmentedScan<BIT_AND, T>>(c);
            break;
        case GRX_REDUCE_BIT_XOR:
            if constexpr (BITS) return RunWave<OpSegmentedScan<BIT_XOR, T>>(c);
            break;
        default: break;
    }
    return kNotInstantiated;
}

template <typename T>
int DispatchMove(int step, const WaveCall &c)
{
    switch (step) {
        case 0: return RunWave<OpDppMove<0x111, 0xF, T>>(c);
        case 1: return RunWave<OpDppMove<0x112, 0xF, T>>(c);
        case 2: return RunWave<OpDppMove<0x114, 0xF, T>>(c);
        case 3: return RunWave<OpDppMove<0x118, 0xF, T>>(c);
        case 4: return RunWave<OpDppMove<0x142, 0xA, T>>(c);
        case 5: return RunWave<OpDppMove<0x143, 0xC, T>>(c);
        default: break;
    }
    return kNotInstantiated;
}

// ---- the near/far split ----
struct BisectCall {
    const int *d_row_offsets;
    const void *d_dist;
    int *d_visit_lookup;
    float delta;
    const int *d_in;
    const unsigned *d_in_dist;
    int num_elements;
    const unsigned long long *d_num_elements;
    unsigned level;
    int tag;
    int near_capacity;
    int *d_near_v, *d_near_row_start, *d_near_scan;
    int far_capacity;
    int *d_far_v;
    unsigned *d_far_d;
    int max_grid_size;
};

template <bool PATHS>
hipError_t RunBisect(const BisectCall &c, unsigned long long *d_near_tail, unsigned long long *d_far_tail, unsigned *d_far_min,
                     int *d_overflow)
{
    typedef app::sssp::SSSPProblem<int, int, int, PATHS> Problem;
    typedef app::sssp::PQFunctor<int, int, Problem> PqFunctor;
    typename Problem::DataSlice slice;
    if (PATHS) slice.d_dist_pred = static_cast<unsigned long long *>(const_cast<void *>(c.d_dist));
    else slice.d_labels = static_cast<unsigned *>(const_cast<void *>(c.d_dist));
    slice.d_visit_lookup = c.d_visit_lookup;
    slice.delta = c.delta;
    priority_queue::BisectArgs<int, int> b;
    b.d_in = c.d_in;
    b.d_in_dist = c.d_in_dist;
    b.num_elements = c.num_elements;
    b.d_num_elements = c.d_num_elements;
    b.level = c.level;
    b.tag = c.tag;
    b.near.v = c.d_near_v;
    b.near.row_start = c.d_near_row_start;
    b.near.scan = c.d_near_scan;
    b.near.capacity = c.near_capacity;
    b.d_near_tail = d_near_tail;
    b.d_far_v = c.d_far_v;
    b.d_far_d = c.d_far_d;
    b.far_capacity = c.far_capacity;
    b.d_far_tail = d_far_tail;
    b.d_far_min = d_far_min;
    b.d_overflow = d_overflow;
    b.d_row_offsets = c.d_row_offsets;
    int grid = c.max_grid_size;
    if (grid <= 0) grid = util::ResidentGrid(priority_queue::BisectKernel<256, 4, Problem, PqFunctor>, 256);
    return priority_queue::Bisect<256, 4, Problem, PqFunctor>(b, slice, grid, 0);
}

}  // namespace

extern "C" {

int grx_device_scan(const unsigned *d_in, long long n, int out_type, void *d_out, unsigned long long *total)
{
    if (n < 0 || !total || (n > 0 && (!d_in || !d_out))) return kBadArgument;
    if (out_type != GRX_SCAN_INT && out_type != GRX_SCAN_UINT && out_type != GRX_SCAN_ULONGLONG) return kBadArgument;
    hipError_t retval = hipSuccess;
    util::DeviceArray<unsigned long long> d_sums;
    GR_CHECK(d_sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(n))), "grx_device_scan scratch failed");
    GR_CHECK(hipDeviceSynchronize(), "grx_device_scan sync failed");
    if (out_type == GRX_SCAN_INT) retval = graphio::DeviceExclusiveScan<int>(d_in, static_cast<int *>(d_out), n, d_sums, 0);
    else if (out_type == GRX_SCAN_UINT) retval = graphio::DeviceExclusiveScan<unsigned>(d_in, static_cast<unsigned *>(d_out), n, d_sums, 0);
    else retval = graphio::DeviceExclusiveScan<unsigned long long>(d_in, static_cast<unsigned long long *>(d_out), n, d_sums, 0);
    if (retval) return static_cast<int>(retval);
    const long long tiles = (n + graphio::kScanTile - 1) / graphio::kScanTile;
    GR_CHECK(hipMemcpy(total, d_sums + tiles, sizeof(unsigned long long), hipMemcpyDeviceToHost), "grx_device_scan read total failed");
    return 0;
}

int grx_device_key_sort(int arrays, const long long *counts, const int *key_bits, const unsigned long long *d_in,
                        unsigned long long *d_out)
{
    if (arrays < 0 || (arrays > 0 && (!counts || !key_bits))) return kBadArgument;
    long long all = 0;
    for (int a = 0; a < arrays; ++a) {
        if (counts[a] < 0 || key_bits[a] < 1 || key_bits[a] > 64) return kBadArgument;
        all += counts[a];
    }
    if (all > 0 && (!d_in || !d_out)) return kBadArgument;
    hipError_t retval = hipSuccess;
    GR_CHECK(hipDeviceSynchronize(), "grx_device_key_sort sync failed");
    graphio::DeviceKeySort sorter;
    long long at = 0;
    for (int a = 0; a < arrays; ++a) {
        const long long n = counts[a];
        GR_CHECK(sorter.Reserve(n), "grx_device_key_sort reserve failed");
        if (n > 0)
            GR_CHECK(hipMemcpyAsync(sorter.Keys(), d_in + at, sizeof(unsigned long long) * static_cast<size_t>(n), hipMemcpyDeviceToDevice, 0),
                     "grx_device_key_sort copy in failed");
        unsigned long long *sorted = nullptr;
        GR_CHECK(sorter.Sort(n, key_bits[a], 0, &sorted), "grx_device_key_sort sort failed");
        if (n > 0)
            GR_CHECK(hipMemcpyAsync(d_out + at, sorted, sizeof(unsigned long long) * static_cast<size_t>(n), hipMemcpyDeviceToDevice, 0),
                     "grx_device_key_sort copy out failed");
        at += n;
    }
    return static_cast<int>(util::GRError(hipDeviceSynchronize(), "grx_device_key_sort failed", __FILE__, __LINE__));
}

int grx_device_transpose(int nodes, long long edges, const int *d_row_offsets, const int *d_col_indices, const unsigned *d_vals,
                         int *d_inv_row_offsets, int *d_inv_col_indices, unsigned *d_inv_vals)
{
    if (nodes < 0 || edges < 0 || !d_row_offsets || !d_inv_row_offsets) return kBadArgument;
    if (edges > 0 && (!d_col_indices || !d_inv_col_indices)) return kBadArgument;
    if ((d_vals == nullptr) != (d_inv_vals == nullptr)) return kBadArgument;
    hipError_t retval = hipSuccess;
    GR_CHECK(hipDeviceSynchronize(), "grx_device_transpose sync failed");
    GR_CHECK(graphio::DeviceTransposeCsr(nodes, edges, d_row_offsets, d_col_indices, d_inv_row_offsets, d_inv_col_indices, 0, d_vals,
                                         d_inv_vals),
             "grx_device_transpose failed");
    return static_cast<int>(util::GRError(hipDeviceSynchronize(), "grx_device_transpose failed", __FILE__, __LINE__));
}

int grx_wave_ops(int op, int r_op, int value_type, int threads, long long n, const void *d_in, const unsigned char *d_heads, void *d_out,
                 void *d_aux)
{
    if (n < 0 || (threads != 64 && threads != 256 && threads != 1024)) return kBadArgument;
    if (n > 0 && (!d_in || !d_out)) return kBadArgument;
    if (n == 0) return 0;
    hipError_t retval = hipSuccess;
    GR_CHECK(hipDeviceSynchronize(), "grx_wave_ops sync failed");
    const WaveCall c{threads, n, d_in, d_heads, d_out, d_aux};
    int rc = kNotInstantiated;
    switch (op) {
        case GRX_WAVE_INCLUSIVE_SUM:
            if (value_type == GRX_VALUE_INT) rc = RunWave<OpInclusiveSum<int>>(c);
            else if (value_type == GRX_VALUE_UINT) rc = RunWave<OpInclusiveSum<unsigned>>(c);
            else if (value_type == GRX_VALUE_ULONGLONG) rc = RunWave<OpInclusiveSum<unsigned long long>>(c);
            break;
        case GRX_WAVE_INCLUSIVE_SUM_DPP:
            if (value_type == GRX_VALUE_UINT) rc = RunWave<OpInclusiveSumDpp>(c);
            break;
        case GRX_WAVE_INCLUSIVE_MAX_DPP:
            if (value_type == GRX_VALUE_UINT) rc = RunWave<OpInclusiveMaxDpp>(c);
            break;
        case GRX_WAVE_SEGMENTED_SCAN_DPP:
            if (value_type == GRX_VALUE_INT) rc = DispatchSegmented<int, true, true>(r_op, c);
            else if (value_type == GRX_VALUE_UINT) rc = DispatchSegmented<unsigned, true, true>(r_op, c);
            else if (value_type == GRX_VALUE_FLOAT) rc = DispatchSegmented<float, false, false>(r_op, c);
            else if (value_type == GRX_VALUE_LONGLONG) rc = DispatchSegmented<long long, false, false>(r_op, c);
            else if (value_type == GRX_VALUE_ULONGLONG) rc = DispatchSegmented<unsigned long long, false, false>(r_op, c);
            break;
        case GRX_WAVE_SUM:
            if (value_type == GRX_VALUE_INT) rc = RunWave<OpWaveSum<int>>(c);
            else if (value_type == GRX_VALUE_UINT) rc = RunWave<OpWaveSum<unsigned>>(c);
            else if (value_type == GRX_VALUE_ULONGLONG) rc = RunWave<OpWaveSum<unsigned long long>>(c);
            break;
        case GRX_WAVE_RANK_IN_MASK:
            if (value_type == GRX_VALUE_ULONGLONG) rc = RunWave<OpRankInMask>(c);
            break;
        case GRX_WAVE_BLOCK_SCAN:
            if (value_type == GRX_VALUE_INT) rc = RunBlockScan<int>(c);
            else if (value_type == GRX_VALUE_ULONGLONG) rc = RunBlockScan<unsigned long long>(c);
            break;
        case GRX_WAVE_DPP_MOVE:
            if (value_type == GRX_VALUE_UINT) rc = DispatchMove<unsigned>(r_op, c);
            else if (value_type == GRX_VALUE_ULONGLONG) rc = DispatchMove<unsigned long long>(r_op, c);
            break;
        default: break;
    }
    if (rc) return rc;
    return static_cast<int>(util::GRError(hipDeviceSynchronize(), "grx_wave_ops failed", __FILE__, __LINE__));
}

int grx_bisect_queue(const int *d_row_offsets, const void *d_dist, int mark_paths, int *d_visit_lookup, float delta, const int *d_in,
                     const unsigned *d_in_dist, int num_elements, const unsigned long long *d_num_elements, unsigned level, int tag,
                     int near_capacity, int *d_near_v, int *d_near_row_start, int *d_near_scan, int far_capacity, int *d_far_v,
                     unsigned *d_far_d, unsigned long long *near_tail, unsigned long long *far_tail, unsigned *far_min, int *overflow,
                     int max_grid_size)
{
    if (!d_row_offsets || !d_dist || !d_visit_lookup || !near_tail || !far_tail || !far_min || !overflow) return kBadArgument;
    if (num_elements < 0 || near_capacity < 0 || far_capacity < 0 || (num_elements > 0 && !d_in)) return kBadArgument;
    if (!d_near_v || !d_near_row_start || !d_near_scan || !d_far_v || !d_far_d) return kBadArgument;
    hipError_t retval = hipSuccess;
    util::DeviceArray<unsigned long long> d_tails;  // [0] near, [1] far
    util::DeviceArray<unsigned> d_far_min;
    util::DeviceArray<int> d_overflow;
    GR_CHECK(d_tails.Alloc(2), "grx_bisect_queue tail words failed");
    GR_CHECK(d_far_min.Alloc(1), "grx_bisect_queue far-min word failed");
    GR_CHECK(d_overflow.Alloc(1), "grx_bisect_queue overflow word failed");
    GR_CHECK(hipMemset(d_tails, 0, sizeof(unsigned long long) * 2), "grx_bisect_queue memset failed");
    GR_CHECK(hipMemset(d_far_min, 0xFF, sizeof(unsigned)), "grx_bisect_queue memset failed");
    GR_CHECK(hipMemset(d_overflow, 0, sizeof(int)), "grx_bisect_queue memset failed");
    GR_CHECK(hipDeviceSynchronize(), "grx_bisect_queue sync failed");
    const BisectCall c{d_row_offsets, d_dist, d_visit_lookup, delta, d_in, d_in_dist, num_elements, d_num_elements, level, tag,
                       near_capacity, d_near_v, d_near_row_start, d_near_scan, far_capacity, d_far_v, d_far_d, max_grid_size};
    retval = mark_paths ? RunBisect<true>(c, d_tails, d_tails + 1, d_far_min, d_overflow)
                        : RunBisect<false>(c, d_tails, d_tails + 1, d_far_min, d_overflow);
    if (retval) return static_cast<int>(retval);
    GR_CHECK(hipDeviceSynchronize(), "grx_bisect_queue failed");
    unsigned long long tails[2] = {0, 0};
    GR_CHECK(hipMemcpy(tails, d_tails, sizeof(tails), hipMemcpyDeviceToHost), "grx_bisect_queue read failed");
    GR_CHECK(hipMemcpy(far_min, d_far_min, sizeof(unsigned), hipMemcpyDeviceToHost), "grx_bisect_queue read failed");
    GR_CHECK(hipMemcpy(overflow, d_overflow, sizeof(int), hipMemcpyDeviceToHost), "grx_bisect_queue read failed");
    *near_tail = tails[0];
    *far_tail = tails[1];
    return 0;
}

}  // extern "C"
