// lib/oprtr_app.hip -- the ADVANCE operator on its own, behind the C ABI (include/gunrock/gunrock_mi355x.h).
//
//  * grx_advance_queue:  advance::LaunchKernel (ids only / full frontier / COUNT_ONLY) over a caller-provided input frontier,
//  * grx_advance_reduce: advance::LaunchReduce for every (R_OP, value type, R_TYPE, BY_VERTEX) listed at Dispatch* below,
// both with the library's own policy KernelPolicy<256, 4, 8, LB> and a small Problem / Functor pair defined here, so the
// operator can be checked edge by edge without a primitive around it (tests/test_advance_gpu.py).  The precedent is
// grx_filter_queue (lib/bfs_app.hip).
//
// Two functors with the same meaning: PlainFunctor has only the reference's CondEdge / ApplyEdge (the shape of
// examples/user_functor.hip); HookedFunctor adds ScreenEdge and IssueEdge / ResolveEdge (oprtr/advance/functor_hooks.hpp), so
// the operator takes its batch path.  The edge rule is a template parameter:
//   RULE_MASK   accept the edge iff d_mask[dst] != 0 (no mask: every edge); duplicates are kept
//   RULE_CLAIM  atomicCAS(&d_labels[dst], -1, depth): the winner accepts (the reference's non-idempotent BFS rule,
//               bfs_functor.cuh:56-58)
// ApplyEdge counts the visit of every accepted edge in d_edge_hits[e_id] and records its source in d_edge_src[e_id].
#include <gunrock/gunrock_mi355x.h>

#include <gunrock/oprtr/advance/kernel.hpp>
#include <gunrock/util/error_utils.hpp>
#include <gunrock/util/frontier.hpp>

using namespace gunrock;
using namespace gunrock::oprtr::advance;

namespace {

enum { RULE_MASK = 0, RULE_CLAIM = 1 };

struct OprtrProblem {
    typedef int VertexId;
    typedef int SizeT;
    typedef int Value;
    struct DataSlice {
        const int *d_mask = nullptr;  // RULE_MASK: per destination vertex
        int *d_labels = nullptr;      // RULE_CLAIM
        int depth = 0;
        int *d_edge_hits = nullptr;   // per edge: times ApplyEdge ran for it
        int *d_edge_src = nullptr;    // per edge: the s_id ApplyEdge saw
    };
};
typedef OprtrProblem::DataSlice Slice;

__device__ __forceinline__ void RecordEdge(int s_id, Slice *p, int e_id)
{
    if (p->d_edge_hits) atomicAdd(&p->d_edge_hits[e_id], 1);
    if (p->d_edge_src) p->d_edge_src[e_id] = s_id;
}

template <int RULE>
struct PlainFunctor {
    static __device__ __forceinline__ bool CondEdge(int /*s_id*/, int d_id, Slice *p, int /*e_id*/ = 0, int /*e_id_in*/ = 0)
    {
        if (RULE == RULE_CLAIM) return atomicCAS(&p->d_labels[d_id], -1, p->depth) == -1;
        return !p->d_mask || p->d_mask[d_id] != 0;
    }
    static __device__ __forceinline__ void ApplyEdge(int s_id, int /*d_id*/, Slice *p, int e_id = 0, int /*e_id_in*/ = 0) { RecordEdge(s_id, p, e_id); }
};

template <int RULE>
struct HookedFunctor {
    // side-effect free, and called for every slot of a tile (dead slots with vertex 0 / edge 0)
    static __device__ __forceinline__ bool ScreenEdge(int /*s_id*/, int d_id, Slice *p, int /*e_id*/, int /*e_id_in*/)
    {
        if (RULE == RULE_CLAIM) return p->d_labels[d_id] == -1;
        return !p->d_mask || p->d_mask[d_id] != 0;
    }
    static __device__ __forceinline__ int IssueEdge(int /*s_id*/, int d_id, Slice *p, int /*e_id*/, int /*e_id_in*/)
    {
        if (RULE == RULE_CLAIM) return atomicCAS(&p->d_labels[d_id], -1, p->depth);
        return -1;
    }
    static __device__ __forceinline__ bool ResolveEdge(int token, int, int, Slice *, int, int) { return token == -1; }
    static __device__ __forceinline__ bool CondEdge(int s_id, int d_id, Slice *p, int e_id = 0, int e_id_in = 0)
    {
        return ScreenEdge(s_id, d_id, p, e_id, e_id_in) && ResolveEdge(IssueEdge(s_id, d_id, p, e_id, e_id_in), s_id, d_id, p, e_id, e_id_in);
    }
    static __device__ __forceinline__ void ApplyEdge(int s_id, int /*d_id*/, Slice *p, int e_id = 0, int /*e_id_in*/ = 0) { RecordEdge(s_id, p, e_id); }
};

typedef KernelPolicy<256, 4, 8, LB> Policy;

constexpr int kBadArgument = -1;
constexpr int kNotInstantiated = -2;

template <typename Functor>
hipError_t LaunchQueue(int mode, const AdvanceArgs<int, int> &a, const Slice &slice, int max_grid_size)
{
    if (mode == GRX_ADVANCE_IDS) return LaunchKernel<Policy, OprtrProblem, Functor, false, false>(a, slice, max_grid_size, 0);
    if (mode == GRX_ADVANCE_FRONTIER) return LaunchKernel<Policy, OprtrProblem, Functor, true, false>(a, slice, max_grid_size, 0);
    return LaunchKernel<Policy, OprtrProblem, Functor, false, true>(a, slice, max_grid_size, 0);
}

struct ReduceCall {
    AdvanceArgs<int, int> args;
    Slice slice;
    const void *d_values;
    void *d_reduced;
    int max_grid_size;
    long long out_len;
    bool prefill;
    int r_type, r_op, by_vertex, functor;
};

template <typename Functor, REDUCE_TYPE RT, REDUCE_OP OP, typename T, bool BV>
int RunReduce(const ReduceCall &c)
{
    return static_cast<int>(LaunchReduce<Policy, OprtrProblem, Functor, RT, OP, T, BV>(
        c.args, c.slice, static_cast<const T *>(c.d_values), static_cast<T *>(c.d_reduced), c.max_grid_size, 0, c.out_len, c.prefill));
}

// every instantiated (op, type) exists for both R_TYPEs and both BY_VERTEX settings with PlainFunctor; HookedFunctor only
// where `HOOKED` says so (the reduction itself does not depend on the functor)
template <REDUCE_OP OP, typename T, bool HOOKED = false>
int DispatchShape(const ReduceCall &c)
{
    if (c.functor == GRX_ADVANCE_FUNCTOR_HOOKED) {
        if constexpr (HOOKED) {
            if (c.r_type == GRX_REDUCE_VERTEX && !c.by_vertex) return RunReduce<HookedFunctor<RULE_MASK>, VERTEX, OP, T, false>(c);
            if (c.r_type == GRX_REDUCE_EDGE && c.by_vertex) return RunReduce<HookedFunctor<RULE_MASK>, EDGE, OP, T, true>(c);
        }
        return kNotInstantiated;
    }
    typedef PlainFunctor<RULE_MASK> F;
    if (c.r_type == GRX_REDUCE_VERTEX) return c.by_vertex ? RunReduce<F, VERTEX, OP, T, true>(c) : RunReduce<F, VERTEX, OP, T, false>(c);
    if (c.r_type == GRX_REDUCE_EDGE) return c.by_vertex ? RunReduce<F, EDGE, OP, T, true>(c) : RunReduce<F, EDGE, OP, T, false>(c);
    return kNotInstantiated;
}

// int / unsigned: PLUS MULTIPLIES MAXIMUM MINIMUM BIT_OR BIT_AND BIT_XOR;  float: PLUS MULTIPLIES MAXIMUM MINIMUM;
// long long / unsigned long long: PLUS MAXIMUM MINIMUM.  Everything else is an error, never a silent fall-through.
template <typename T, bool ARITH32, bool BITS>
int DispatchOp(const ReduceCall &c)
{
    constexpr bool HOOKED = std::is_same<T, int>::value || std::is_same<T, float>::value;
    switch (c.r_op) {
        case GRX_REDUCE_PLUS: return DispatchShape<PLUS, T, HOOKED>(c);
        case GRX_REDUCE_MAXIMUM: return DispatchShape<MAXIMUM, T>(c);
        case GRX_REDUCE_MINIMUM: return DispatchShape<MINIMUM, T, HOOKED>(c);
        case GRX_REDUCE_MULTIPLIES:
            if constexpr (ARITH32) return DispatchShape<MULTIPLIES, T>(c);
            break;
        case GRX_REDUCE_BIT_OR:
            if constexpr (BITS) return DispatchShape<BIT_OR, T>(c);
            break;
        case GRX_REDUCE_BIT_AND:
            if constexpr (BITS) return DispatchShape<BIT_AND, T>(c);
            break;
        case GRX_REDUCE_BIT_XOR:
            if constexpr (BITS) return DispatchShape<BIT_XOR, T>(c);
            break;
        default: break;
    }
    return kNotInstantiated;
}

bool FrontierGiven(const int *v, const int *row_start, const int *scan, int in_len, int in_edges)
{
    return in_len >= 0 && in_edges >= 0 && (in_len == 0 || (v && row_start && scan));
}

}  // namespace

static_assert(int(GRX_REDUCE_VERTEX) == int(VERTEX) && int(GRX_REDUCE_EDGE) == int(EDGE) && int(GRX_REDUCE_PLUS) == int(PLUS) &&
                  int(GRX_REDUCE_MINUS) == int(MINUS) && int(GRX_REDUCE_MULTIPLIES) == int(MULTIPLIES) && int(GRX_REDUCE_MODULUS) == int(MODULUS) &&
                  int(GRX_REDUCE_BIT_OR) == int(BIT_OR) && int(GRX_REDUCE_BIT_AND) == int(BIT_AND) && int(GRX_REDUCE_BIT_XOR) == int(BIT_XOR) &&
                  int(GRX_REDUCE_MAXIMUM) == int(MAXIMUM) && int(GRX_REDUCE_MINIMUM) == int(MINIMUM),
              "the header's constants are the operator's enums");

extern "C" {

int grx_advance_queue(const int *d_row_offsets, const int *d_col_indices, const int *d_in_v, const int *d_in_row_start,
                      const int *d_in_scan, int in_len, int in_edges, int mode, int rule, int functor, const int *d_mask, int *d_labels,
                      int depth, int *d_edge_hits, int *d_edge_src, int capacity, int *d_out_v, int *d_out_row_start, int *d_out_scan,
                      int *out_len, long long *out_edges, int max_grid_size)
{
    if (!d_row_offsets || !d_col_indices || !out_len || !FrontierGiven(d_in_v, d_in_row_start, d_in_scan, in_len, in_edges)) return kBadArgument;
    if (mode != GRX_ADVANCE_IDS && mode != GRX_ADVANCE_FRONTIER && mode != GRX_ADVANCE_COUNT_ONLY) return kBadArgument;
    if (rule != GRX_ADVANCE_RULE_MASK && rule != GRX_ADVANCE_RULE_CLAIM) return kBadArgument;
    if (functor != GRX_ADVANCE_FUNCTOR_PLAIN && functor != GRX_ADVANCE_FUNCTOR_HOOKED) return kBadArgument;
    if (rule == GRX_ADVANCE_RULE_CLAIM && !d_labels) return kBadArgument;
    if (mode != GRX_ADVANCE_COUNT_ONLY && (capacity < 0 || !d_out_v)) return kBadArgument;
    if (mode == GRX_ADVANCE_FRONTIER && (!d_out_row_start || !d_out_scan)) return kBadArgument;
    hipError_t retval = hipSuccess;
    util::DeviceArray<unsigned long long> d_tail;
    util::DeviceArray<int> d_overflow;
    GR_CHECK(d_tail.Alloc(1), "grx_advance_queue tail word failed");
    GR_CHECK(d_overflow.Alloc(1), "grx_advance_queue overflow word failed");
    GR_CHECK(hipMemset(d_tail, 0, sizeof(unsigned long long)), "grx_advance_queue memset failed");
    GR_CHECK(hipMemset(d_overflow, 0, sizeof(int)), "grx_advance_queue memset failed");
    GR_CHECK(hipDeviceSynchronize(), "grx_advance_queue sync failed");
    AdvanceArgs<int, int> a{};
    a.in.v = const_cast<int *>(d_in_v);
    a.in.row_start = const_cast<int *>(d_in_row_start);
    a.in.scan = const_cast<int *>(d_in_scan);
    a.in.capacity = in_len;
    a.out.v = d_out_v;
    a.out.row_start = d_out_row_start;
    a.out.scan = d_out_scan;
    a.out.capacity = capacity;
    a.in_len = in_len;
    a.in_edges = in_edges;
    a.d_row_offsets = d_row_offsets;
    a.d_column_indices = d_col_indices;
    a.d_tail_out = d_tail;
    a.d_tail_clear = nullptr;
    a.d_overflow = d_overflow;
    Slice slice;
    slice.d_mask = d_mask;
    slice.d_labels = d_labels;
    slice.depth = depth;
    slice.d_edge_hits = d_edge_hits;
    slice.d_edge_src = d_edge_src;
    if (rule == GRX_ADVANCE_RULE_MASK) {
        if (functor == GRX_ADVANCE_FUNCTOR_PLAIN) retval = LaunchQueue<PlainFunctor<RULE_MASK>>(mode, a, slice, max_grid_size);
        else retval = LaunchQueue<HookedFunctor<RULE_MASK>>(mode, a, slice, max_grid_size);
    } else {
        if (functor == GRX_ADVANCE_FUNCTOR_PLAIN) retval = LaunchQueue<PlainFunctor<RULE_CLAIM>>(mode, a, slice, max_grid_size);
        else retval = LaunchQueue<HookedFunctor<RULE_CLAIM>>(mode, a, slice, max_grid_size);
    }
    unsigned long long tail = 0;
    int overflow = 0;
    if (!retval) retval = util::GRError(hipMemcpy(&tail, d_tail, sizeof(tail), hipMemcpyDeviceToHost), "grx_advance_queue read failed", __FILE__, __LINE__);
    if (!retval) retval = util::GRError(hipMemcpy(&overflow, d_overflow, sizeof(int), hipMemcpyDeviceToHost), "grx_advance_queue read failed", __FILE__, __LINE__);
    if (retval) return static_cast<int>(retval);
    if (overflow) return static_cast<int>(util::GRError(hipErrorInvalidConfiguration, "Frontier queue overflow. Please increase queue-sizing factor.", __FILE__, __LINE__));
    *out_len = static_cast<int>(util::TailCount(tail));
    if (out_edges) *out_edges = static_cast<long long>(util::TailEdges(tail));
    return 0;
}

int grx_advance_reduce(const int *d_row_offsets, const int *d_col_indices, const int *d_in_v, const int *d_in_row_start,
                       const int *d_in_scan, int in_len, int in_edges, int r_type, int r_op, int value_type, int by_vertex, int prefill,
                       long long out_len, const void *d_values, void *d_reduced, int functor, const int *d_mask, int *d_edge_hits,
                       int *d_edge_src, int max_grid_size)
{
    if (!d_row_offsets || !d_col_indices || !d_values || !d_reduced || !FrontierGiven(d_in_v, d_in_row_start, d_in_scan, in_len, in_edges))
        return kBadArgument;
    if (out_len < 0 || (!by_vertex && out_len != 0 && out_len < in_len)) return kBadArgument;
    if (functor != GRX_ADVANCE_FUNCTOR_PLAIN && functor != GRX_ADVANCE_FUNCTOR_HOOKED) return kBadArgument;
    hipError_t retval = hipSuccess;
    GR_CHECK(hipDeviceSynchronize(), "grx_advance_reduce sync failed");
    ReduceCall c;
    c.args = AdvanceArgs<int, int>{};
    c.args.in.v = const_cast<int *>(d_in_v);
    c.args.in.row_start = const_cast<int *>(d_in_row_start);
    c.args.in.scan = const_cast<int *>(d_in_scan);
    c.args.in.capacity = in_len;
    c.args.in_len = in_len;
    c.args.in_edges = in_edges;
    c.args.d_row_offsets = d_row_offsets;
    c.args.d_column_indices = d_col_indices;
    c.slice.d_mask = d_mask;
    c.slice.d_edge_hits = d_edge_hits;
    c.slice.d_edge_src = d_edge_src;
    c.d_values = d_values;
    c.d_reduced = d_reduced;
    c.max_grid_size = max_grid_size;
    c.out_len = out_len;
    c.prefill = prefill != 0;
    c.r_type = r_type;
    c.r_op = r_op;
    c.by_vertex = by_vertex != 0;
    c.functor = functor;
    int rc = kNotInstantiated;
    switch (value_type) {
        case GRX_VALUE_INT: rc = DispatchOp<int, true, true>(c); break;
        case GRX_VALUE_UINT: rc = DispatchOp<unsigned, true, true>(c); break;
        case GRX_VALUE_FLOAT: rc = DispatchOp<float, true, false>(c); break;
        case GRX_VALUE_LONGLONG: rc = DispatchOp<long long, false, false>(c); break;
        case GRX_VALUE_ULONGLONG: rc = DispatchOp<unsigned long long, false, false>(c); break;
        default: break;
    }
    if (rc) return rc;
    return static_cast<int>(util::GRError(hipDeviceSynchronize(), "grx_advance_reduce failed", __FILE__, __LINE__));
}

}  // extern "C"
