// convert.hip -- astype: out = D(a) for every ordered pair of {f32, f64, i32, i64} (smhip_convert; the rules: sm_convert.h).
//
// The view is first simplified (extents of 1 dropped, adjacent axes that walk memory as one merged), then takes one route:
//   DENSE   one pass, sizeof(S) + sizeof(D) bytes per element; roofline: HBM.  Every lane converts a fixed group of elements:
//             4 <-> 4   4 elements: one 16-byte access on each side
//             8 <-> 8   2 elements: one 16-byte access on each side
//             8  -> 4   4 elements: two adjacent 16-byte loads, one 16-byte store
//             4  -> 8   2 elements: one 8-byte load, one 16-byte store
//           The last one was first built as the mirror of 8 -> 4 (one 16-byte load, two adjacent 16-byte stores) and ran at 51 % of
//           8 TB/s where NEG over the same bytes reaches 80 %: each store instruction of a wavefront then writes 16 bytes of every
//           32, and non-temporal stores with such holes are what limits it (tools/sweep_widen.hip -> profiles/sweep_widen.txt:
//           3.9 TB/s; 5.9 with plain stores; 6.6 with one 16-byte store per lane and an 8-byte load).  Holes on the READ side cost
//           4-5 % (8 -> 4) and are left.  Workgroups of 256, the launch's streaming policy over the true byte counts of the two
//           sides, the n % group elements past the body by the first lane past it, operands above 256 MiB on their wider side in
//           pieces (piece_for).  Pointers need only element alignment (ops.hip.h: vec_t), so a slice that starts mid-vector is
//           DENSE too.
//   ROWS    innermost stride 1 (a block of rows or columns, an outer axis broadcast): the same groups along each row, the
//           row's start found from up to five outer (extent, stride) pairs; the same traffic as DENSE.
//   STAGED  everything else (transposed, stepped or broadcast along the last axis): the view is copied dense IN THE SOURCE
//           TYPE by the broadcast kernels (SMHIP_OP_LEFT) into a pooled block and converted by DENSE: 3 * sizeof(S) + sizeof(D)
//           bytes per element against sizeof(S) + sizeof(D).  Reading such views in place would need the tile / strided-row /
//           gather kernels of broadcast.hip once more for each of the 12 pairs; as with EXP / LOG of a view (unary.hip) that was
//           too much code for the rarer case.
//   COPY    src_dtype == dst_dtype: the dense copy (the array kernel as LEFT) or the LEFT gather; no kernel of this file.
#include <type_traits>

#include "abi_args.h"
#include "internal.h"
#include "ops.hip.h"
#include "sm_convert.h"

namespace smhip {
namespace {

using namespace dev;

constexpr int kBlock = 256;
constexpr size_t kPieceWideBytes = (size_t)256 << 20;  // a piece's wider side
constexpr int kMaxOuter = SMHIP_MAX_NDIM - 1;
constexpr uint64_t kRowsLanesPerLaunch = (uint64_t)1 << 36;  // 2^28 workgroups

template <typename S, typename D>
struct Group {
    static constexpr int size = sizeof(D) == 8 ? 2 : 4;  // the wide side of a lane is ONE 16-byte access unless the result is the narrow side
};
constexpr int group_size(size_t, size_t dsz) { return dsz == 8 ? 2 : 4; }

// One lane's group at `src` -> `dst`: the loads in one policy branch, the stores in another (one branch per access would
// serialise them: ops.hip.h, load_stream_as).  NT: the 4 -> 8 pairs' read policy, chosen by the host as an instantiation -- as a
// launch-time branch around one 8-byte load the two arms are the same load with different metadata to the optimiser, which
// merges them and drops the hint (ops.hip.h: load_stream_if; its two-halves form does not survive for halves of one element).
template <typename S, typename D>
constexpr bool kWidens = sizeof(S) < sizeof(D);
template <typename S, typename D, bool NT>
__device__ __forceinline__ void convert_group(const S *src, D *dst, int pol) {
    typedef VecTraits<S> TS;
    typedef VecTraits<D> TD;
    constexpr int G = Group<S, D>::size;
    typename TD::vec_t *pd = reinterpret_cast<typename TD::vec_t *>(dst);
    if constexpr (sizeof(S) < sizeof(D)) {  // 4 -> 8: an 8-byte load, one 16-byte store
        typename TS::half_full_t in;
        const typename TS::half_t *ps = reinterpret_cast<const typename TS::half_t *>(src);
        if constexpr (NT) in = __builtin_nontemporal_load(ps);
        else in = *ps;
        const typename TD::full_t res = {smconvert::convert<D, S>(in[0]), smconvert::convert<D, S>(in[1])};
        store_stream_if(D, pd, res, pol);
    } else {
        constexpr int NS = G / TS::width, ND = G / TD::width;
        const typename TS::vec_t *ps = reinterpret_cast<const typename TS::vec_t *>(src);
        typename TS::full_t in[NS];
        if (pol & kLoadNt) {
#pragma unroll
            for (int k = 0; k < NS; ++k) in[k] = load_stream_as(S, ps + k, true);
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k) in[k] = load_stream_as(S, ps + k, false);
        }
        typename TD::full_t res[ND];
#pragma unroll
        for (int e = 0; e < G; ++e) res[e / TD::width][e % TD::width] = smconvert::convert<D, S>(in[e / TS::width][e % TS::width]);
        static_assert(ND == 1, "the result side of a lane is one 16-byte store");
        store_stream_if(D, pd, res[0], pol);
    }
}

template <typename S, typename D, bool NT>
__global__ __launch_bounds__(kBlock) void convert_vec_kernel(const S *__restrict__ a, D *__restrict__ out, size_t n_grp, int tail, int pol) {
    constexpr int G = Group<S, D>::size;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n_grp) {
        convert_group<S, D, NT>(a + i * G, out + i * G, pol);
    } else if (i == n_grp) {  // the n % G elements past the last whole group: the first lane past the body
        for (int k = 0; k < tail; ++k) out[n_grp * G + k] = smconvert::convert<D, S>(a[n_grp * G + k]);
    }
}

// The outer axes of a ROWS view, outermost first; `count` of them.
struct RowsOuter {
    uint64_t extent[kMaxOuter];
    uint64_t stride[kMaxOuter];
    int count;
};

// Lane i of the launch: row row0 + i / gpr of the view, group i % gpr of that row (gpr = ceil(cols / G): a row's last group
// may be short and is then converted element by element).  `out` points at row row0's result.  I: 32-bit indices when
// everything fits (two to six divisions per lane).
template <typename S, typename D, typename I, bool NT>
__global__ __launch_bounds__(kBlock) void convert_rows_kernel(const S *__restrict__ a, D *__restrict__ out, RowsOuter o, uint64_t row0, uint64_t cols,
                                                              uint64_t gpr, uint64_t lanes, int pol) {
    constexpr int G = Group<S, D>::size;
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= lanes) return;
    const I row = (I)i / (I)gpr, cg = (I)i - row * (I)gpr;
    I r = row + (I)row0;
    uint64_t off = 0;
    for (int d = o.count - 1; d >= 0; --d) {
        const I q = r / (I)o.extent[d];
        off += (uint64_t)(r - q * (I)o.extent[d]) * o.stride[d];
        r = q;
    }
    const uint64_t c0 = (uint64_t)cg * G;
    const S *src = a + off + c0;
    D *dst = out + (uint64_t)row * cols + c0;
    if (c0 + G <= cols) {
        convert_group<S, D, NT>(src, dst, pol);
    } else {
        const int rem = (int)(cols - c0);
        for (int k = 0; k < rem; ++k) dst[k] = smconvert::convert<D, S>(src[k]);
    }
}

// ------------------------------------------------------------------------------------------------------------ planner
struct Plan {
    int route = SMHIP_CONVERT_ROUTE_NONE;
    int launches = 0;
    int64_t bytes = 0;
    size_t n = 0;
    // the simplified view: extents > 1, no two adjacent axes that merge
    int nd = 0;
    int64_t shape[SMHIP_MAX_NDIM], strides[SMHIP_MAX_NDIM];
    size_t piece_grp = 0;      // DENSE / STAGED: groups per launch
    uint64_t rows_per = 0;     // ROWS: rows per launch
};

size_t dense_piece_groups(size_t n_grp, size_t ssz, size_t dsz) {
    const size_t wide_per_grp = (size_t)group_size(ssz, dsz) * (ssz > dsz ? ssz : dsz);
    const size_t most = kPieceWideBytes / wide_per_grp;
    size_t piece = piece_for(n_grp, 2);  // honours SMHIP_PIECE_LOG2VEC (tests run the piece loop at small sizes)
    if (piece == 0 || piece > most) piece = most;
    return piece;
}

int dense_launches(size_t n, size_t ssz, size_t dsz, size_t *piece_out) {
    const int G = group_size(ssz, dsz);
    const size_t n_grp = n / G, piece = dense_piece_groups(n_grp, ssz, dsz);
    *piece_out = piece;
    const size_t pieces = n_grp == 0 ? 1 : (n_grp + piece - 1) / piece;  // (a call of fewer than G elements is its tail lane alone)
    return (int)pieces;
}

Plan make_plan(int src_dtype, int dst_dtype, const int64_t *shape, const int64_t *strides, int ndim) {
    Plan pl;
    const size_t ssz = dtype_size(src_dtype), dsz = dtype_size(dst_dtype);
    size_t n = 1;
    for (int d = 0; d < ndim; ++d) n *= (size_t)shape[d];
    pl.n = n;
    if (n == 0) return pl;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] == 1) continue;
        if (pl.nd > 0 && pl.strides[pl.nd - 1] == shape[d] * strides[d]) {  // the axis before walks memory as this one continued
            pl.shape[pl.nd - 1] *= shape[d];
            pl.strides[pl.nd - 1] = strides[d];
        } else {
            pl.shape[pl.nd] = shape[d];
            pl.strides[pl.nd] = strides[d];
            ++pl.nd;
        }
    }
    if (pl.nd == 0) {  // one element
        pl.shape[0] = 1;
        pl.strides[0] = 1;
        pl.nd = 1;
    }
    const bool dense = pl.nd == 1 && (pl.strides[0] == 1 || n == 1);
    if (src_dtype == dst_dtype) {
        pl.route = SMHIP_CONVERT_ROUTE_COPY;
        pl.launches = 1;
        pl.bytes = (int64_t)(n * 2 * ssz);
        if (dense) {
            const size_t n_vec = n * ssz / 16, piece = piece_for(n_vec, 2);  // launch_array_scalar's own piece loop
            if (piece) pl.launches = (int)((n_vec + piece - 1) / piece);
        }
        return pl;
    }
    if (dense) {
        pl.route = SMHIP_CONVERT_ROUTE_DENSE;
        pl.launches = dense_launches(n, ssz, dsz, &pl.piece_grp);
        pl.bytes = (int64_t)(n * (ssz + dsz));
        return pl;
    }
    if (pl.strides[pl.nd - 1] == 1) {
        const int G = group_size(ssz, dsz);
        const uint64_t cols = (uint64_t)pl.shape[pl.nd - 1], rows = n / cols, gpr = (cols + G - 1) / G;
        if (gpr <= kRowsLanesPerLaunch) {
            pl.route = SMHIP_CONVERT_ROUTE_ROWS;
            pl.rows_per = kRowsLanesPerLaunch / gpr;
            pl.launches = (int)((rows + pl.rows_per - 1) / pl.rows_per);
            pl.bytes = (int64_t)(n * (ssz + dsz));
            return pl;
        }
    }
    pl.route = SMHIP_CONVERT_ROUTE_STAGED;
    pl.launches = 1 + dense_launches(n, ssz, dsz, &pl.piece_grp);  // the copy counted as one
    pl.bytes = (int64_t)(n * (3 * ssz + dsz));
    return pl;
}

// ----------------------------------------------------------------------------------------------------------- launches
template <typename S, typename D>
int run_dense(const Plan &pl, const void *a, void *out, hipStream_t s) {
    constexpr int G = Group<S, D>::size;
    const S *pa = static_cast<const S *>(a);
    D *po = static_cast<D *>(out);
    const size_t n = pl.n, n_grp = n / G, piece = pl.piece_grp;
    const int tail = (int)(n % G);
    const int pol = stream_policy({{pa, n * sizeof(S)}}, {po, n * sizeof(D)});
    for (size_t g0 = 0;; g0 += piece) {
        const bool last = g0 + piece >= n_grp;
        const size_t ng = last ? n_grp - g0 : piece;
        const size_t threads = ng + (last && tail ? 1 : 0);
        const size_t grid = (threads + kBlock - 1) / kBlock;  // <= 2^24 / 256 + 1
        if (!grid) {
        } else if (kWidens<S, D> && (pol & kPolicyLoadNt)) {
            hipLaunchKernelGGL((convert_vec_kernel<S, D, kWidens<S, D>>), dim3((unsigned)grid), dim3(kBlock), 0, s, pa + g0 * G, po + g0 * G, ng, last ? tail : 0, pol);
        } else {
            hipLaunchKernelGGL((convert_vec_kernel<S, D, false>), dim3((unsigned)grid), dim3(kBlock), 0, s, pa + g0 * G, po + g0 * G, ng, last ? tail : 0, pol);
        }
        if (last) break;
    }
    SMHIP_LAUNCH_CHECK("convert");
    return SMHIP_OK;
}

template <typename S, typename D>
int run_rows(const Plan &pl, const void *a, void *out, hipStream_t s) {
    constexpr int G = Group<S, D>::size;
    const S *pa = static_cast<const S *>(a);
    D *po = static_cast<D *>(out);
    RowsOuter o{};
    o.count = pl.nd - 1;
    bool narrow = true;  // 32-bit row arithmetic
    for (int d = 0; d < o.count; ++d) {
        o.extent[d] = (uint64_t)pl.shape[d];
        o.stride[d] = (uint64_t)pl.strides[d];
        narrow = narrow && o.extent[d] < ((uint64_t)1 << 31);
    }
    const uint64_t cols = (uint64_t)pl.shape[pl.nd - 1], rows = pl.n / cols, gpr = (cols + G - 1) / G;
    narrow = narrow && rows * gpr < ((uint64_t)1 << 31);
    int64_t last = 0;
    for (int d = 0; d < pl.nd; ++d) last += (pl.shape[d] - 1) * pl.strides[d];
    const int pol = stream_policy({{pa, (size_t)(last + 1) * sizeof(S)}}, {po, pl.n * sizeof(D)});
    for (uint64_t r0 = 0; r0 < rows; r0 += pl.rows_per) {
        const uint64_t nr = rows - r0 < pl.rows_per ? rows - r0 : pl.rows_per, lanes = nr * gpr;
        const unsigned grid = (unsigned)((lanes + kBlock - 1) / kBlock);
        const bool nt = kWidens<S, D> && (pol & kPolicyLoadNt);
        if (narrow && nt)
            hipLaunchKernelGGL((convert_rows_kernel<S, D, uint32_t, kWidens<S, D>>), dim3(grid), dim3(kBlock), 0, s, pa, po + r0 * cols, o, r0, cols, gpr, lanes, pol);
        else if (narrow)
            hipLaunchKernelGGL((convert_rows_kernel<S, D, uint32_t, false>), dim3(grid), dim3(kBlock), 0, s, pa, po + r0 * cols, o, r0, cols, gpr, lanes, pol);
        else if (nt)
            hipLaunchKernelGGL((convert_rows_kernel<S, D, uint64_t, kWidens<S, D>>), dim3(grid), dim3(kBlock), 0, s, pa, po + r0 * cols, o, r0, cols, gpr, lanes, pol);
        else
            hipLaunchKernelGGL((convert_rows_kernel<S, D, uint64_t, false>), dim3(grid), dim3(kBlock), 0, s, pa, po + r0 * cols, o, r0, cols, gpr, lanes, pol);
    }
    SMHIP_LAUNCH_CHECK("convert rows");
    return SMHIP_OK;
}

template <typename S, typename D>
int run_pair(const Plan &pl, const void *a, void *out, hipStream_t s) {
    return pl.route == SMHIP_CONVERT_ROUTE_ROWS ? run_rows<S, D>(pl, a, out, s) : run_dense<S, D>(pl, a, out, s);
}

template <typename S>
int run_from(const Plan &pl, int dst_dtype, const void *a, void *out, hipStream_t s) {
    switch (dst_dtype) {
        case SMHIP_F32: if constexpr (!std::is_same<S, float>::value) return run_pair<S, float>(pl, a, out, s); break;
        case SMHIP_F64: if constexpr (!std::is_same<S, double>::value) return run_pair<S, double>(pl, a, out, s); break;
        case SMHIP_I32: if constexpr (!std::is_same<S, int32_t>::value) return run_pair<S, int32_t>(pl, a, out, s); break;
        case SMHIP_I64: if constexpr (!std::is_same<S, int64_t>::value) return run_pair<S, int64_t>(pl, a, out, s); break;
    }
    return fail(SMHIP_ERR_INVALID, "convert: bad dtype pair");
}

int run_kernels(const Plan &pl, int src_dtype, int dst_dtype, const void *a, void *out, hipStream_t s) {
    switch (src_dtype) {
        case SMHIP_F32: return run_from<float>(pl, dst_dtype, a, out, s);
        case SMHIP_F64: return run_from<double>(pl, dst_dtype, a, out, s);
        case SMHIP_I32: return run_from<int32_t>(pl, dst_dtype, a, out, s);
        case SMHIP_I64: return run_from<int64_t>(pl, dst_dtype, a, out, s);
    }
    return fail(SMHIP_ERR_INVALID, "convert: bad dtype %d", src_dtype);
}

int launch_convert(const Plan &pl, int src_dtype, int dst_dtype, const void *a, void *out, hipStream_t s) {
    const int64_t zero[SMHIP_MAX_NDIM] = {};
    switch (pl.route) {
        case SMHIP_CONVERT_ROUTE_COPY: {
            if (pl.nd == 1 && (pl.strides[0] == 1 || pl.n == 1)) {
                const int64_t unused = 0;
                return launch_array_scalar(SMHIP_OP_LEFT, src_dtype, a, &unused, pl.n, out, s);
            }
            return launch_broadcast(SMHIP_OP_LEFT, src_dtype, a, pl.strides, a, zero, pl.shape, pl.nd, out, s);
        }
        case SMHIP_CONVERT_ROUTE_STAGED: {
            ScratchLease lease;
            double *dense;
            if (int rc = lease.take((pl.n * dtype_size(src_dtype) + 7) / 8, &dense)) return rc;
            if (int rc = launch_broadcast(SMHIP_OP_LEFT, src_dtype, a, pl.strides, a, zero, pl.shape, pl.nd, dense, s)) return rc;
            return run_kernels(pl, src_dtype, dst_dtype, dense, out, s);  // the lease ends here: the pool's reuse is stream-ordered
        }
        default: return run_kernels(pl, src_dtype, dst_dtype, a, out, s);
    }
}

int convert_check(const char *who, int src_dtype, int dst_dtype, const int64_t *shape, const int64_t *strides, int ndim) {
    if (!valid_dtype(src_dtype) || !valid_dtype(dst_dtype)) return fail(SMHIP_ERR_INVALID, "%s: bad dtype %d -> %d", who, src_dtype, dst_dtype);
    if (ndim < 1 || ndim > SMHIP_MAX_NDIM) return fail(SMHIP_ERR_INVALID, "%s: ndim %d outside 1..%d", who, ndim, SMHIP_MAX_NDIM);
    if (!strides || !shape) return fail(SMHIP_ERR_INVALID, "%s: null shape/stride", who);
    for (int i = 0; i < ndim; ++i)
        if (shape[i] < 0 || strides[i] < 0) return fail(SMHIP_ERR_INVALID, "%s: negative extent or stride at dim %d", who, i);
    return SMHIP_OK;
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_convert(int src_dtype, int dst_dtype, const void *a, const int64_t *strides, const int64_t *shape, int ndim, void *out) {
    if (int rc = convert_check("convert", src_dtype, dst_dtype, shape, strides, ndim)) return rc;
    const int64_t n = element_count(shape, ndim);
    if (n == 0) return SMHIP_OK;
    if (!a || !out) return fail(SMHIP_ERR_INVALID, "convert: null buffer");
    const Span read{a, span_bytes(shape, strides, ndim, dtype_size(src_dtype))}, write{out, (size_t)n * dtype_size(dst_dtype)};
    if (spans_overlap(read, write)) return fail(SMHIP_ERR_INVALID, "convert: `out` overlaps the operand");
    const Plan pl = make_plan(src_dtype, dst_dtype, shape, strides, ndim);
    hipStream_t s;
    OpScope op_scope;
    // recorded tiny operators are flushed first; STAGED uses a pooled block that is not declared, so it orders itself behind
    // everything and everything later behind it
    if (int rc = op_scope.begin(&read, 1, write, &s, pl.route == SMHIP_CONVERT_ROUTE_STAGED)) return rc;
    return launch_convert(pl, src_dtype, dst_dtype, a, out, s);
}

int smhip_convert_plan(int src_dtype, int dst_dtype, const int64_t *shape, const int64_t *strides, int ndim, int *route, int *launches,
                       int64_t *bytes_moved) {
    if (int rc = convert_check("convert_plan", src_dtype, dst_dtype, shape, strides, ndim)) return rc;
    const Plan pl = make_plan(src_dtype, dst_dtype, shape, strides, ndim);
    if (route) *route = pl.route;
    if (launches) *launches = pl.launches;
    if (bytes_moved) *bytes_moved = pl.bytes;
    return SMHIP_OK;
}
