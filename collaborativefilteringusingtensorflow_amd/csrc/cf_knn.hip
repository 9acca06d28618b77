// cf_knn.hip -- the memory-based family of src/models/basic/models
// (pop.py, usercf.py, itemcf.py) and src/models/others/models/useritemcf.py,
// on gfx950.  Input: the binarised train matrix R as a pattern-only CSR.
//
// Similarity (usercf.py:19-27 and its copies): np.dot(sR, sR.T) in float32,
// then for ind ascending row ind and column ind divided by den_ind =
// float32(sqrt(nnz_ind)), the diagonal zeroed.  For a != b with c the
// intersection count that is
//     S[a, b] = fl32(fl32(c / den_lo) / den_hi),   lo = min(a, b), hi = max(a, b)
// two IEEE divisions in that order; a zero den is never divided by (c is 0).
// Neighbours: the topK largest positive similarities of a row, ties to the
// lower id -- the reference's argsort leaves that tie open.
// Predictions are float64 sums of float32 terms:
//   UserCF      pred[u, :] = sum_{v in N(u)} S[u, v] R[v, :]          (usercf.py:29-42)
//   ItemCF      pred[u, :] = sum_{i in R_u} Sk[i, :]                  (itemcf.py:42-50)
//   UserItemCF  sum_v fl32(fl32(theta) S_user[u, v]) R[v, :]
//             + sum_{i in R_u} fl32(fl32(1. - theta) S_item[i, :])    (useritemcf.py:41-51)
//   PopRank     the item's train count                                (pop.py:20-22)
//
// Both passes have one shape: an outer list is walked one member at a time,
// and the lanes of one wave spread over that member's inner list, whose ids
// are distinct -- no two lanes meet on an accumulator cell, so no sum takes an
// atomic and the order of every sum is the outer list's order: equal inputs
// give equal bits at every shape.  The accumulators are an LDS tile of the
// column range (u32 counts, fp64 predictions); a block is one wave and owns
// one (row, tile), so several blocks share a CU's 160 KiB.
//   knn_sim_kernel      outer = the members j of query row a, inner = row j of
//                       the transposed side (sorted: entered at the tile's
//                       lower bound); the finished counts become S, written
//                       as float_key(S) for launch_topk and / or as floats
//   knn_pad_kernel      selected entries with sim <= 0 become pads (-1, 0)
//   knn_predict_kernel  USER: outer = N(u) with its weights, inner = R_v;
//                       ITEM: outer = R_u, inner = the neighbour list of item
//                       i (sorted by sim, so filtered by tile range); the tile
//                       leaves as float_key(float32(pred)), key 0 at the
//                       user's train items under exclude_train, or as fp64
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cf_engine.h"
#include "cf_device.h"
#include "cf_host.h"

namespace cfk {

constexpr int kKnnBlock = kWave;          // one wave per (row, tile)
constexpr int kKnnTileCols = 8192;        // u32 counts: 32 KiB
constexpr int kKnnTileItems = 4096;       // fp64 sums: 32 KiB
constexpr int kKnnMaxTileCols = 16384;    // 64 KiB: two blocks per CU still fit
constexpr int kKnnMaxTileItems = 8192;
constexpr int kKnnMaxTopK = 4096;         // launch_topk's k

struct KnnSimArgs {
    int64_t n_side;                        // rows = columns of S
    int tile;
    const int32_t* __restrict__ rows;      // [grid.x] query rows
    const int64_t* __restrict__ ptrA;      // the side's CSR: row a -> members j
    const int32_t* __restrict__ idxA;
    const int64_t* __restrict__ ptrB;      // the transposed side: member j -> rows b
    const int32_t* __restrict__ idxB;
    const float* __restrict__ den;         // [n_side] float32(sqrt(nnz))
    uint32_t* __restrict__ keys;           // [grid.x, n_side], nullable
    float* __restrict__ sims;              // [grid.x, n_side], nullable
};

struct KnnPredArgs {
    int kind, topK;
    int64_t n_users, n_items;
    int tile;
    float th_user, th_item;                // fl32(theta), fl32(1. - theta)
    const int32_t* __restrict__ users;     // [grid.x]
    const int64_t* __restrict__ indptr;    // R
    const int32_t* __restrict__ indices;
    const int64_t* __restrict__ indptr_t;  // R^T (POP: the counts)
    const int32_t* __restrict__ nb_idx_u;  // [n_users, topK], -1 pads
    const float* __restrict__ nb_sim_u;
    const int32_t* __restrict__ nb_idx_i;  // [n_items, topK]
    const float* __restrict__ nb_sim_i;
    int exclude_train;
    uint32_t* __restrict__ keys;           // [grid.x, n_items], nullable
    double* __restrict__ pred;             // [grid.x, n_items], nullable
};

// first position in the sorted run [lo, hi) whose id is >= key
__device__ __forceinline__ int64_t knn_lower_bound(const int32_t* __restrict__ a, int64_t lo, int64_t hi,
                                                   int32_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kKnnBlock) void knn_sim_kernel(KnnSimArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_cnt[];
    const int lane = threadIdx.x;
    const int32_t row = a.rows[blockIdx.x];
    const int64_t c0 = (int64_t)blockIdx.y * a.tile;
    const int w = (int)min((int64_t)a.tile, a.n_side - c0);
    const int32_t c1 = (int32_t)(c0 + w);
    for (int t = lane; t < w; t += kKnnBlock) s_cnt[t] = 0u;
    __syncthreads();
    for (int64_t p = a.ptrA[row]; p < a.ptrA[row + 1]; ++p) {   // outer: one member at a time
        const int32_t j = a.idxA[p];
        const int64_t hi = a.ptrB[j + 1];
        for (int64_t q = knn_lower_bound(a.idxB, a.ptrB[j], hi, (int32_t)c0) + lane; q < hi; q += kKnnBlock) {
            const int32_t b = a.idxB[q];   // inner: distinct ids, one lane each
            if (b >= c1) break;
            s_cnt[b - (int32_t)c0] += 1u;
        }
        __syncthreads();   // the next member's lanes may meet this one's cells
    }
    const float den_a = a.den[row];
    for (int t = lane; t < w; t += kKnnBlock) {
        const int64_t b = c0 + t;
        const uint32_t c = s_cnt[t];
        float s = 0.f;
        if (c != 0u && b != row) {   // c > 0: both rows hold a member, both dens are positive
            const float den_b = a.den[b];
            const float lo = b < row ? den_b : den_a, hi = b < row ? den_a : den_b;
            s = __fdiv_rn(__fdiv_rn((float)c, lo), hi);
        }
        const int64_t o = (int64_t)blockIdx.x * a.n_side + b;
        if (a.keys) a.keys[o] = float_key(s);
        if (a.sims) a.sims[o] = s;
    }
}

// the selected rows [n, k]: a pad of the selection (-1, NaN) and an entry that is no
// positive similarity become (-1, 0); the rows are sorted, so the pads form the tail
__global__ __launch_bounds__(kBlock) void knn_pad_kernel(int32_t* __restrict__ idx, float* __restrict__ sim,
                                                         int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    if (idx[t] < 0 || !(sim[t] > 0.f)) {
        idx[t] = -1;
        sim[t] = 0.f;
    }
}

__global__ __launch_bounds__(kKnnBlock) void knn_predict_kernel(KnnPredArgs a) {
    extern __shared__ __attribute__((aligned(16))) double s_acc[];
    const int lane = threadIdx.x;
    const int32_t u = a.users[blockIdx.x];
    const int64_t c0 = (int64_t)blockIdx.y * a.tile;
    const int w = (int)min((int64_t)a.tile, a.n_items - c0);
    const int32_t c1 = (int32_t)(c0 + w);
    const int64_t rb = a.indptr[u], re = a.indptr[u + 1];
    if (a.kind == CF_KNN_POP) {
        for (int t = lane; t < w; t += kKnnBlock)
            s_acc[t] = (double)(a.indptr_t[c0 + t + 1] - a.indptr_t[c0 + t]);
    } else {
        for (int t = lane; t < w; t += kKnnBlock) s_acc[t] = 0.0;
    }
    __syncthreads();
    if (a.kind == CF_KNN_USER || a.kind == CF_KNN_USERITEM) {
        const bool scaled = a.kind == CF_KNN_USERITEM;
        for (int n = 0; n < a.topK; ++n) {   // outer: the user's neighbours, in table order
            const int32_t v = a.nb_idx_u[(int64_t)u * a.topK + n];
            if (v < 0) continue;             // block-uniform
            const float s = a.nb_sim_u[(int64_t)u * a.topK + n];
            const double term = (double)(scaled ? __fmul_rn(a.th_user, s) : s);
            const int64_t hi = a.indptr[v + 1];
            for (int64_t q = knn_lower_bound(a.indices, a.indptr[v], hi, (int32_t)c0) + lane; q < hi;
                 q += kKnnBlock) {
                const int32_t i = a.indices[q];   // inner: R_v, distinct items
                if (i >= c1) break;
                s_acc[i - (int32_t)c0] += term;
            }
            __syncthreads();
        }
    }
    if (a.kind == CF_KNN_ITEM || a.kind == CF_KNN_USERITEM) {
        const bool scaled = a.kind == CF_KNN_USERITEM;
        for (int64_t p = rb; p < re; ++p) {   // outer: the user's own items
            const int64_t i = a.indices[p];
            for (int n = lane; n < a.topK; n += kKnnBlock) {   // inner: item i's neighbours, sorted by sim
                const int32_t j = a.nb_idx_i[i * a.topK + n];
                if (j < (int32_t)c0 || j >= c1) continue;      // pads (-1) and the other tiles
                const float s = a.nb_sim_i[i * a.topK + n];
                s_acc[j - (int32_t)c0] += (double)(scaled ? __fmul_rn(a.th_item, s) : s);
            }
            __syncthreads();
        }
    }
    if (a.pred)
        for (int t = lane; t < w; t += kKnnBlock) a.pred[(int64_t)blockIdx.x * a.n_items + c0 + t] = s_acc[t];
    if (!a.keys) return;
    if (a.exclude_train) {   // the user's train items leave the tile as NaN: no sum is one
        for (int64_t q = knn_lower_bound(a.indices, rb, re, (int32_t)c0) + lane; q < re; q += kKnnBlock) {
            const int32_t i = a.indices[q];
            if (i >= c1) break;
            s_acc[i - (int32_t)c0] = __longlong_as_double(0x7ff8000000000000ll);
        }
        __syncthreads();
    }
    for (int t = lane; t < w; t += kKnnBlock) {
        const double v = s_acc[t];
        a.keys[(int64_t)blockIdx.x * a.n_items + c0 + t] = (v != v) ? 0u : float_key((float)v);
    }
}

}  // namespace cfk

using namespace cfk;

struct cf_knn {
    int64_t n_users = 0, n_items = 0;
    int kind = 0, topK = 0;
    double theta = 0.0;
    int tile_cols = kKnnTileCols, tile_items = kKnnTileItems;
    int device = 0;
    hipStream_t stream = nullptr;
    bool have_csr = false;
    cfi::DevBuf<int64_t> indptr, indptr_t;
    cfi::DevBuf<int32_t> indices, indices_t;
    cfi::DevBuf<float> den[2];        // [0] users, [1] items
    cfi::DevBuf<int32_t> nb_idx[2];   // [n_side, topK]; null until fit / set_neighbours
    cfi::DevBuf<float> nb_sim[2];
};

namespace {

int64_t knn_side_n(const cf_knn* e, int side) { return side == 0 ? e->n_users : e->n_items; }
bool knn_uses(const cf_knn* e, int side) {
    return e->kind == CF_KNN_USERITEM || (side == 0 ? e->kind == CF_KNN_USER : e->kind == CF_KNN_ITEM);
}

// rows per chunk under the 256 MiB rule of score_topk_chunks
int knn_chunk(int64_t n, int64_t row_elems, size_t elem_bytes) {
    const size_t per = (size_t)row_elems * elem_bytes;
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / std::max<size_t>(per, 1)));
}

hipError_t launch_knn_sim(const cf_knn* e, int side, const int32_t* d_rows, int m, uint32_t* keys, float* sims) {
    KnnSimArgs a{};
    a.n_side = knn_side_n(e, side);
    a.tile = e->tile_cols;
    a.rows = d_rows;
    a.ptrA = side == 0 ? e->indptr : e->indptr_t;
    a.idxA = side == 0 ? e->indices : e->indices_t;
    a.ptrB = side == 0 ? e->indptr_t : e->indptr;
    a.idxB = side == 0 ? e->indices_t : e->indices;
    a.den = e->den[side];
    a.keys = keys;
    a.sims = sims;
    const int64_t tiles = (a.n_side + a.tile - 1) / a.tile;
    if (tiles > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_sim_kernel, dim3((unsigned)m, (unsigned)tiles), dim3(kKnnBlock),
                       (size_t)a.tile * sizeof(uint32_t), e->stream, a);
    return hipGetLastError();
}

hipError_t launch_knn_predict(const cf_knn* e, const int32_t* d_users, int m, int exclude_train, uint32_t* keys,
                              double* pred) {
    KnnPredArgs a{};
    a.kind = e->kind; a.topK = e->topK;
    a.n_users = e->n_users; a.n_items = e->n_items;
    a.tile = e->tile_items;
    a.th_user = (float)e->theta;
    a.th_item = (float)(1. - e->theta);   // formed in double first (useritemcf.py:49)
    a.users = d_users;
    a.indptr = e->indptr; a.indices = e->indices; a.indptr_t = e->indptr_t;
    a.nb_idx_u = e->nb_idx[0]; a.nb_sim_u = e->nb_sim[0];
    a.nb_idx_i = e->nb_idx[1]; a.nb_sim_i = e->nb_sim[1];
    a.exclude_train = exclude_train ? 1 : 0;
    a.keys = keys;
    a.pred = pred;
    const int64_t tiles = (a.n_items + a.tile - 1) / a.tile;
    if (tiles > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_predict_kernel, dim3((unsigned)m, (unsigned)tiles), dim3(kKnnBlock),
                       (size_t)a.tile * sizeof(double), e->stream, a);
    return hipGetLastError();
}

// the calls that read the tables: the CSR is set and every table the kind needs is there
int knn_ready(const cf_knn* e, const char* who) {
    if (!e->have_csr) return cfi::fail(CF_ESTATE, std::string(who) + " needs cf_knn_set_interactions");
    for (int side = 0; side < 2; ++side)
        if (knn_uses(e, side) && !e->nb_idx[side].p)
            return cfi::fail(CF_ESTATE, std::string(who) + " needs cf_knn_fit or cf_knn_set_neighbours");
    return CF_OK;
}

int knn_check_side(const cf_knn* e, int side) {
    if (side != 0 && side != 1) return cfi::fail(CF_EINVAL, "side must be 0 (users) or 1 (items)");
    if (!knn_uses(e, side)) return cfi::fail(CF_EINVAL, "this kind keeps no neighbour table of that side");
    return CF_OK;
}

int knn_fit_side(cf_knn* e, int side) {
    const int64_t n = knn_side_n(e, side);
    const int K = e->topK;
    CF_TRY(e->nb_idx[side].reset((size_t)n * K, "neighbour ids"));
    CF_TRY(e->nb_sim[side].reset((size_t)n * K, "neighbour sims"));
    const int chunk = knn_chunk(n, n, 4);
    cfi::DevBuf<uint32_t> keys;
    cfi::DevBuf<int32_t> d_rows;
    CF_TRY(keys.reset((size_t)chunk * n, "similarity keys"));
    CF_TRY(d_rows.reset((size_t)n, "similarity rows"));
    std::vector<int32_t> rows((size_t)n);
    for (int64_t r = 0; r < n; ++r) rows[(size_t)r] = (int32_t)r;
    CF_HIP(hipMemcpyAsync(d_rows, rows.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int m = (int)std::min<int64_t>(chunk, n - r0);
        CF_HIP(launch_knn_sim(e, side, d_rows + r0, m, keys, nullptr));
        TopkArgs t{};
        t.k = K;
        t.n_items = n;
        t.keys = keys;
        t.idx_out = e->nb_idx[side] + r0 * K;
        t.val_out = e->nb_sim[side] + r0 * K;
        CF_HIP(launch_topk(t, m, e->stream));
    }
    const int64_t cells = n * K;
    hipLaunchKernelGGL(knn_pad_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, e->stream,
                       e->nb_idx[side].get(), e->nb_sim[side].get(), cells);
    CF_HIP(hipGetLastError());
    CF_HIP(hipStreamSynchronize(e->stream));   // rows and keys go out of scope
    return CF_OK;
}

}  // namespace

extern "C" {

int cf_knn_create(int64_t n_users, int64_t n_items, int32_t kind, int32_t topK, double theta, int32_t device,
                  cf_knn** out) {
    if (!out || n_users < 1 || n_items < 1 || n_users > INT32_MAX || n_items > INT32_MAX)
        return cfi::set_error(CF_EINVAL, "bad neighbourhood configuration");
    if (kind != CF_KNN_POP && kind != CF_KNN_USER && kind != CF_KNN_ITEM && kind != CF_KNN_USERITEM)
        return cfi::set_error(CF_EINVAL, "kind must be CF_KNN_POP, _USER, _ITEM or _USERITEM");
    if (topK < 1 || topK > kKnnMaxTopK) return cfi::set_error(CF_EINVAL, "topK must be 1..4096");
    if (!(theta >= 0.0 && theta <= 1.0)) return cfi::set_error(CF_EINVAL, "theta must be in [0, 1]");
    *out = nullptr;
    CF_TRY(cfi::open_device(device));
    cf_knn* e = new cf_knn();
    e->n_users = n_users; e->n_items = n_items; e->kind = kind; e->topK = topK; e->theta = theta;
    e->device = device;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
        cf_knn_destroy(e);
        return cfi::set_error(CF_EHIP, "hipStreamCreate failed");
    }
    *out = e;
    return CF_OK;
}

int cf_knn_destroy(cf_knn* e) {
    return cfi::destroy_object(e);
}

int cf_knn_set_option(cf_knn* e, const char* name, int64_t value) {
    if (!e || !name) return cfi::set_error(CF_EINVAL, "null argument");
    const bool cols = std::strcmp(name, "tile_cols") == 0;
    if (!cols && std::strcmp(name, "tile_items") != 0)
        return cfi::set_error(CF_EINVAL, std::string("unknown option: ") + name);
    const int dflt = cols ? kKnnTileCols : kKnnTileItems, top = cols ? kKnnMaxTileCols : kKnnMaxTileItems;
    if (value < 0 || value > top)
        return cfi::set_error(CF_EINVAL, std::string(name) + " must be 0 (default) or 1.." + std::to_string(top));
    const int tile = value == 0 ? dflt : (int)value;
    const int64_t widest = cols ? std::max(e->n_users, e->n_items) : e->n_items;
    if ((widest + tile - 1) / tile > 65535)
        return cfi::set_error(CF_EINVAL, std::string(name) + " leaves more than 65,535 tiles at this shape");
    (cols ? e->tile_cols : e->tile_items) = tile;
    return CF_OK;
}

int cf_knn_set_interactions(cf_knn* e, const int64_t* indptr, const int32_t* indices, int64_t nnz) {
    if (!e) return cfi::set_error(CF_EINVAL, "null CSR");
    CF_TRY(cfi::check_csr(indptr, indices, nnz, e->n_users, e->n_items));
    CF_HIP(hipSetDevice(e->device));
    // the transpose: a counting sort by item keeps each item's users ascending
    std::vector<int64_t> tptr((size_t)e->n_items + 1, 0);
    std::vector<int32_t> tidx((size_t)std::max<int64_t>(nnz, 1));
    for (int64_t k = 0; k < nnz; ++k) tptr[(size_t)indices[k] + 1]++;
    for (int64_t i = 0; i < e->n_items; ++i) tptr[(size_t)i + 1] += tptr[(size_t)i];
    {
        std::vector<int64_t> at(tptr.begin(), tptr.end() - 1);
        for (int64_t u = 0; u < e->n_users; ++u)
            for (int64_t k = indptr[u]; k < indptr[u + 1]; ++k) tidx[(size_t)at[(size_t)indices[k]]++] = (int32_t)u;
    }
    // np.linalg.norm of a 0/1 float32 row: float32(sqrt(nnz)), IEEE
    std::vector<float> du((size_t)e->n_users), di((size_t)e->n_items);
    for (int64_t u = 0; u < e->n_users; ++u) du[(size_t)u] = std::sqrt((float)(indptr[u + 1] - indptr[u]));
    for (int64_t i = 0; i < e->n_items; ++i) di[(size_t)i] = std::sqrt((float)(tptr[(size_t)i + 1] - tptr[(size_t)i]));
    e->have_csr = false;
    CF_TRY(cfi::upload_csr(e->stream, e->indptr, e->indices, indptr, indices, nnz, e->n_users));
    CF_TRY(cfi::upload_csr(e->stream, e->indptr_t, e->indices_t, tptr.data(), tidx.data(), nnz, e->n_items));
    CF_TRY(e->den[0].reset((size_t)e->n_users, "user norms"));
    CF_TRY(e->den[1].reset((size_t)e->n_items, "item norms"));
    CF_HIP(hipMemcpy(e->den[0], du.data(), du.size() * 4, hipMemcpyHostToDevice));
    CF_HIP(hipMemcpy(e->den[1], di.data(), di.size() * 4, hipMemcpyHostToDevice));
    e->have_csr = true;
    return CF_OK;
}

int cf_knn_fit(cf_knn* e) {
    if (!e) return cfi::set_error(CF_EINVAL, "null neighbourhood object");
    if (!e->have_csr) return cfi::set_error(CF_ESTATE, "cf_knn_fit needs cf_knn_set_interactions");
    CF_HIP(hipSetDevice(e->device));
    CF_HIP(hipStreamSynchronize(e->stream));
    for (int side = 0; side < 2; ++side)
        if (knn_uses(e, side)) CF_TRY(knn_fit_side(e, side));
    return CF_OK;
}

int cf_knn_check_neighbours(int64_t n_side, int32_t topK, const int32_t* idx, const float* sim) {
    if (!idx || !sim || n_side < 1 || topK < 1) return cfi::set_error(CF_EINVAL, "null argument");
    std::vector<int64_t> seen((size_t)n_side, -1);   // the last row that held the id
    for (int64_t r = 0; r < n_side; ++r)
        for (int32_t n = 0; n < topK; ++n) {
            const int64_t at = r * topK + n;
            const int32_t j = idx[at];
            if (j == -1) continue;   // a pad
            if (j < 0 || j >= n_side)
                return cfi::set_error(CF_EINVAL, "neighbour id out of range in row " + std::to_string(r));
            if (seen[(size_t)j] == r)
                return cfi::set_error(CF_EINVAL, "neighbour id repeated in row " + std::to_string(r));
            seen[(size_t)j] = r;
            if (!std::isfinite(sim[at]))
                return cfi::set_error(CF_EINVAL, "similarity not finite in row " + std::to_string(r));
        }
    return CF_OK;
}

int cf_knn_set_neighbours(cf_knn* e, int32_t side, const int32_t* idx, const float* sim) {
    if (!e || !idx || !sim) return cfi::set_error(CF_EINVAL, "null argument");
    CF_TRY(knn_check_side(e, side));
    const int64_t n = knn_side_n(e, side);
    CF_TRY(cf_knn_check_neighbours(n, e->topK, idx, sim));
    CF_HIP(hipSetDevice(e->device));
    CF_HIP(hipStreamSynchronize(e->stream));
    const size_t cells = (size_t)n * e->topK;
    CF_TRY(e->nb_idx[side].reserve(cells, "neighbour ids"));
    CF_TRY(e->nb_sim[side].reserve(cells, "neighbour sims"));
    CF_HIP(hipMemcpy(e->nb_idx[side], idx, cells * 4, hipMemcpyHostToDevice));
    CF_HIP(hipMemcpy(e->nb_sim[side], sim, cells * 4, hipMemcpyHostToDevice));
    return CF_OK;
}

int cf_knn_get_neighbours(cf_knn* e, int32_t side, int32_t* idx_out, float* sim_out) {
    if (!e || !idx_out || !sim_out) return cfi::set_error(CF_EINVAL, "null argument");
    CF_TRY(knn_check_side(e, side));
    if (!e->nb_idx[side].p) return cfi::set_error(CF_ESTATE, "no neighbour table yet: cf_knn_fit first");
    CF_HIP(hipSetDevice(e->device));
    CF_HIP(hipStreamSynchronize(e->stream));
    const size_t cells = (size_t)knn_side_n(e, side) * e->topK;
    CF_HIP(hipMemcpy(idx_out, e->nb_idx[side], cells * 4, hipMemcpyDeviceToHost));
    CF_HIP(hipMemcpy(sim_out, e->nb_sim[side], cells * 4, hipMemcpyDeviceToHost));
    return CF_OK;
}

int cf_knn_similarity(cf_knn* e, int32_t side, const int32_t* rows, int32_t n, float* out) {
    if (!e || n < 0 || (n > 0 && (!rows || !out))) return cfi::set_error(CF_EINVAL, "bad arguments");
    if (side != 0 && side != 1) return cfi::set_error(CF_EINVAL, "side must be 0 (users) or 1 (items)");
    if (!e->have_csr) return cfi::set_error(CF_ESTATE, "cf_knn_similarity needs cf_knn_set_interactions");
    if (n == 0) return CF_OK;
    const int64_t ns = knn_side_n(e, side);
    for (int r = 0; r < n; ++r)
        if (rows[r] < 0 || rows[r] >= ns) return cfi::set_error(CF_EINVAL, "row id out of range");
    CF_HIP(hipSetDevice(e->device));
    const int chunk = knn_chunk(n, ns, 4);
    cfi::DevBuf<int32_t> d_rows;
    cfi::DevBuf<float> d_s;
    CF_TRY(d_rows.reset((size_t)n, "similarity rows"));
    CF_TRY(d_s.reset((size_t)chunk * ns, "similarity chunk"));
    CF_HIP(hipMemcpyAsync(d_rows, rows, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int m = std::min(chunk, n - r0);
        CF_HIP(launch_knn_sim(e, side, d_rows + r0, m, nullptr, d_s));
        CF_HIP(hipStreamSynchronize(e->stream));
        CF_HIP(hipMemcpy(out + (size_t)r0 * ns, d_s, (size_t)m * ns * 4, hipMemcpyDeviceToHost));
    }
    return CF_OK;
}

int cf_knn_predict(cf_knn* e, const int32_t* users, int32_t n, double* out) {
    if (!e || n < 0 || (n > 0 && (!users || !out))) return cfi::set_error(CF_EINVAL, "bad arguments");
    CF_TRY(knn_ready(e, "cf_knn_predict"));
    if (n == 0) return CF_OK;
    for (int r = 0; r < n; ++r)
        if (users[r] < 0 || users[r] >= e->n_users) return cfi::set_error(CF_EINVAL, "user id out of range");
    CF_HIP(hipSetDevice(e->device));
    const int chunk = knn_chunk(n, e->n_items, 8);
    cfi::DevBuf<int32_t> d_users;
    cfi::DevBuf<double> d_p;
    CF_TRY(d_users.reset((size_t)n, "predict users"));
    CF_TRY(d_p.reset((size_t)chunk * e->n_items, "predict chunk"));
    CF_HIP(hipMemcpyAsync(d_users, users, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    for (int r0 = 0; r0 < n; r0 += chunk) {
        const int m = std::min(chunk, n - r0);
        CF_HIP(launch_knn_predict(e, d_users + r0, m, 0, nullptr, d_p));
        CF_HIP(hipStreamSynchronize(e->stream));
        CF_HIP(hipMemcpy(out + (size_t)r0 * e->n_items, d_p, (size_t)m * e->n_items * 8, hipMemcpyDeviceToHost));
    }
    return CF_OK;
}

int cf_knn_score_topk(cf_knn* e, const int32_t* users, int32_t n, int32_t k, int32_t exclude_train,
                      int32_t* idx_out, float* val_out) {
    if (!e) return cfi::set_error(CF_EINVAL, "bad arguments");
    CF_TRY(knn_ready(e, "cf_knn_score_topk"));
    CF_HIP(hipSetDevice(e->device));
    return cfi::score_topk_chunks(
        e->stream, "cf_knn", e->n_users, e->n_items, e->have_csr, users, n, k, exclude_train, idx_out, val_out,
        true, [&](const int32_t* d_users, int m, uint32_t* keys, int32_t*, float*) {
            return launch_knn_predict(e, d_users, m, exclude_train, keys, nullptr);
        });
}

}  // extern "C"
