// cf_lrml.hip -- LRML (src/models/others/models/lrml.py), the consumer of
// sampler_lrml_ranking, on gfx950.
//
// Tables: U [n_users, d] and V [n_items, d] are trained; Key [d, M] and
// Mem [M, d] are drawn once and stay fixed (lrml.py:114 var_list).  For a
// batch of B positive pairs (u, i) and B negative pairs (u', i')
// (lrml.py:59-80), per row:
//   e = U_u o V_i,  a = softmax_n(e^T Key),  r = a^T Mem,
//   dp = U_u + r - V_i,  dn = U_u' + r - V_i',
//   h = |dp|^2 + margin - |dn|^2,  loss = sum relu(h)
// and for a row with h > 0, with g_r = 2 (dp - dn), g_a = Mem g_r,
// g_z = a o (g_a - <a, g_a>), g_e = Key g_z:
//   dU_u = 2 dp + g_e o V_i,  dV_i = -2 dp + g_e o U_u,
//   dU_u' = -2 dn,            dV_i' = 2 dn.
// TF1 sums the gradient rows of one table row over the whole batch -- both
// roles -- before SparseApplyAdagrad; every row of U and V is then clipped to
// norm <= clip_norm (lrml.py:106-116).
//
// One step = two launches:
//   lrml_step_kernel   Key^T and Mem staged in LDS once per block; one 16-lane
//                      group per batch row gathers the four table rows, forms
//                      a, r, h and the four gradient rows, counts each row's
//                      occurrences (returning atomic: rank 0 owns the row) and
//                      scatters the gradients into the dense, zero-between-
//                      steps GU / GV with float atomics; the pre-update loss
//                      reduces per block into fp64 partials in a fixed order;
//   lrml_apply_kernel  one group per occurrence (2B user + 2B item): the owner
//                      reads the summed row, applies Adagrad + clip
//                      (adagrad_row), zeroes the gradient row and the count.
// Untouched rows are fixed points of the clip once clipped:
// launch_clip_full runs on both tables once after the first step that
// follows create / init_params / set_table.
//
// Recommend (lrml.py:86-104) is NOT the training attention: the reference
// multiplies elementwise and takes the softmax over the factor axis,
//   x[n, k] = (U_u[k] V_i[k]) Key[k, n],  att[n, .] = softmax_k x[n, .],
//   rel[k] = sum_n att[n, k] Mem[n, k],   score = -|U_u + rel - V_i|^2
// (predict_mode 0, the default); predict_mode 1 scores with the step's own a
// and r.  lrml_score_kernel writes order-preserving keys for launch_topk.
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cf_engine.h"
#include "cf_host.h"
#include "cf_kernels_impl.h"

namespace cfk {

constexpr int kLrmlMaxD = 128;
constexpr int kLrmlMaxM = 64;
// floats per LDS table (Key^T, Mem): the small class holds the driver's
// d = 100, M = 20; the large one the limits d = 128, M = 64 (2 x 32 KB)
constexpr int kLrmlSmall = 2048;
constexpr int kLrmlLarge = kLrmlMaxD * kLrmlMaxM;
constexpr int kLrmlScoreItems = 256;   // items per scoring block (16 per group)

struct LrmlArgs {
    int d, M, B;
    float margin, lr, clip_norm;
    const int32_t* __restrict__ pos;     // [B, 2]
    const int32_t* __restrict__ neg;     // [B, 2]
    const float* __restrict__ Key;       // [d, M]
    const float* __restrict__ Mem;       // [M, d]
    float* __restrict__ U; float* __restrict__ AU; float* __restrict__ GU;
    float* __restrict__ V; float* __restrict__ AV; float* __restrict__ GV;
    int32_t* __restrict__ cntU;          // [n_users] occurrences in this batch (0 between steps)
    int32_t* __restrict__ cntV;          // [n_items]
    int32_t* __restrict__ rankU;         // [2B] rank of (u_p | u'_p) inside its row
    int32_t* __restrict__ rankV;         // [2B]
    double* __restrict__ loss_partial;   // [step blocks]
    double* __restrict__ loss_acc;       // running sum until cf_lrml_take_loss
};

struct LrmlScoreArgs {
    int d, M;
    int64_t n_items;
    const int32_t* __restrict__ users;   // this chunk's users (grid y)
    const float* __restrict__ U;
    const float* __restrict__ V;
    const float* __restrict__ Key;
    const float* __restrict__ Mem;
    uint32_t* __restrict__ keys;         // [users, n_items]
    int exclude_train;
    const int64_t* __restrict__ indptr;
    const int32_t* __restrict__ indices;
};

// max over a 16-lane group (one DPP row), the steps of gsum
__device__ __forceinline__ float gmax(float v) {
    v = fmaxf(v, dpp_f<0xB1>(v));
    v = fmaxf(v, dpp_f<0x4E>(v));
    v = fmaxf(v, dpp_f<0x141>(v));
    v = fmaxf(v, dpp_f<0x140>(v));
    return v;
}

// Key [d, M] -> s_k[n * d + k] (transposed), Mem [M, d] -> s_m as it is
__device__ __forceinline__ void lrml_stage(const float* __restrict__ Key, const float* __restrict__ Mem,
                                           int d, int M, float* s_k, float* s_m) {
    for (int t = threadIdx.x; t < M * d; t += kBlock) {
        const int n = t / d, k = t - n * d;
        s_k[t] = Key[k * M + n];
        s_m[t] = Mem[t];
    }
    __syncthreads();
}

// the element each slot of this lane holds (row_ld's mapping), clamped into
// the row for the LDS reads of a padding slot (whose values are zero)
template <int EPL>
__device__ __forceinline__ void lrml_slots(int d, int gl, int (&idx)[EPL], bool (&ok)[EPL]) {
    const bool full = vec_rows<EPL>() && d == kGL * EPL;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int e = elem_of<EPL>(s, gl, full);
        ok[s] = e < d;
        idx[s] = ok[s] ? e : 0;
    }
}

// out[n] = <x, T[n, :]> for n < M, held by lane n % 16 in slot n / 16
// (the other slots: fill).  UJ: rows in flight (the unroll of the row loop):
// 16 in the step (110 VGPRs at d = 100); the scoring kernel, whose item loop
// surrounds it, spills at 16 and takes 2
template <int EPL, int UJ>
__device__ __forceinline__ void lrml_rows_dot(const float (&x)[EPL], const int (&idx)[EPL],
                                              const float* T, int d, int M, int gl, float fill,
                                              float (&out)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        out[c] = fill;
#pragma unroll UJ
        for (int j = 0; j < kGL; ++j) {
            const int n = c * kGL + j;
            if (n >= M) break;
            const float* row = T + n * d;
            float p = 0.f;
#pragma unroll
            for (int s = 0; s < EPL; ++s) p = fmaf(x[s], row[idx[s]], p);
            p = gsum(p);
            if (gl == j) out[c] = p;
        }
    }
}

// y[k] = sum_n w[n] T[n, k]; w: the group's [kLrmlMaxM] LDS vector
template <int EPL>
__device__ __forceinline__ void lrml_cols_sum(const float* w, const int (&idx)[EPL], const bool (&ok)[EPL],
                                              const float* T, int d, int M, float (&y)[EPL]) {
#pragma unroll
    for (int s = 0; s < EPL; ++s) y[s] = 0.f;
    for (int n = 0; n < M; ++n) {
        const float wn = w[n];
        const float* row = T + n * d;
#pragma unroll
        for (int s = 0; s < EPL; ++s) y[s] = fmaf(wn, row[idx[s]], y[s]);
    }
#pragma unroll
    for (int s = 0; s < EPL; ++s) y[s] = ok[s] ? y[s] : 0.f;
}

// the group's vector, one value per (lane, slot), into its LDS row; the
// group's lanes belong to one wave, whose LDS operations retire in order
__device__ __forceinline__ void lrml_publish(float* w, int gl, const float (&v)[4]) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int c = 0; c < 4; ++c) w[c * kGL + gl] = v[c];
    __builtin_amdgcn_wave_barrier();
}

// a = softmax_n(e^T Key) with the row maximum subtracted (lane-distributed as
// lrml_rows_dot leaves it, and published to w), r = a^T Mem
template <int EPL, int UJ>
__device__ __forceinline__ void lrml_attend(const float (&e)[EPL], const int (&idx)[EPL], const bool (&ok)[EPL],
                                            const float* s_k, const float* s_m, int d, int M, int gl,
                                            float* w, float (&al)[4], float (&r)[EPL]) {
    float z[4];
    lrml_rows_dot<EPL, UJ>(e, idx, s_k, d, M, gl, -INFINITY, z);
    const float zm = gmax(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])));
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        al[c] = (c * kGL + gl < M) ? expf(z[c] - zm) : 0.f;
        t += al[c];
    }
    t = gsum(t);
#pragma unroll
    for (int c = 0; c < 4; ++c) al[c] = al[c] / t;
    lrml_publish(w, gl, al);
    lrml_cols_sum<EPL>(w, idx, ok, s_m, d, M, r);
}

template <int EPL, int KMAX>
__global__ __launch_bounds__(kBlock) void lrml_step_kernel(LrmlArgs a) {
    __shared__ float s_k[KMAX], s_m[KMAX];
    __shared__ float s_w[kGroupsPerBlock][kLrmlMaxM];
    __shared__ double s_l[kGroupsPerBlock];
    const int d = a.d, M = a.M;
    lrml_stage(a.Key, a.Mem, d, M, s_k, s_m);
    const int gl = threadIdx.x & (kGL - 1), grp = threadIdx.x >> 4;
    const int p = blockIdx.x * kGroupsPerBlock + grp;
    float lossf = 0.f;
    if (p < a.B) {
        const int64_t u = a.pos[2 * p], i = a.pos[2 * p + 1];
        const int64_t u2 = a.neg[2 * p], i2 = a.neg[2 * p + 1];
        int idx[EPL];
        bool ok[EPL];
        lrml_slots<EPL>(d, gl, idx, ok);
        float uu[EPL], vi[EPL], un[EPL], vn[EPL];
        gload<EPL>(a.U, u, d, gl, uu);
        gload<EPL>(a.V, i, d, gl, vi);
        gload<EPL>(a.U, u2, d, gl, un);
        gload<EPL>(a.V, i2, d, gl, vn);
        // occurrence ranks, lanes 0..3 one row each (rank 0 owns the row in the apply)
        if (gl < 4) {
            int32_t* cnt = (gl & 1) ? a.cntV : a.cntU;
            const int64_t row = gl == 0 ? u : gl == 1 ? i : gl == 2 ? u2 : i2;
            int32_t* rk = (gl & 1) ? a.rankV : a.rankU;
            rk[(gl >> 1) * a.B + p] = atomicAdd(cnt + row, 1);
        }
        float e[EPL], r[EPL], al[4];
#pragma unroll
        for (int s = 0; s < EPL; ++s) e[s] = uu[s] * vi[s];
        lrml_attend<EPL, kGL>(e, idx, ok, s_k, s_m, d, M, gl, s_w[grp], al, r);
        float dp[EPL], dn[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            dp[s] = (uu[s] + r[s]) - vi[s];
            dn[s] = (un[s] + r[s]) - vn[s];
        }
        const float h = (gdot<EPL>(dp, dp) + a.margin) - gdot<EPL>(dn, dn);
        if (h > 0.f) {   // group-uniform: gsum leaves the same bits in every lane
            lossf = h;
            float gr[EPL], ga[4], gz[4], ge[EPL];
#pragma unroll
            for (int s = 0; s < EPL; ++s) gr[s] = 2.f * (dp[s] - dn[s]);
            lrml_rows_dot<EPL, kGL>(gr, idx, s_m, d, M, gl, 0.f, ga);
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) dot = fmaf(al[c], ga[c], dot);
            dot = gsum(dot);
#pragma unroll
            for (int c = 0; c < 4; ++c) gz[c] = al[c] * (ga[c] - dot);
            lrml_publish(s_w[grp], gl, gz);
            lrml_cols_sum<EPL>(s_w[grp], idx, ok, s_k, d, M, ge);
            float g[EPL];
#pragma unroll
            for (int s = 0; s < EPL; ++s) g[s] = fmaf(ge[s], vi[s], 2.f * dp[s]);
            gatomic<EPL>(a.GU, u, d, gl, g);
#pragma unroll
            for (int s = 0; s < EPL; ++s) g[s] = fmaf(ge[s], uu[s], -2.f * dp[s]);
            gatomic<EPL>(a.GV, i, d, gl, g);
#pragma unroll
            for (int s = 0; s < EPL; ++s) g[s] = -2.f * dn[s];
            gatomic<EPL>(a.GU, u2, d, gl, g);
#pragma unroll
            for (int s = 0; s < EPL; ++s) g[s] = 2.f * dn[s];
            gatomic<EPL>(a.GV, i2, d, gl, g);
        }
    }
    if (gl == 0) s_l[grp] = (double)lossf;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int g = 0; g < kGroupsPerBlock; ++g) acc += s_l[g];
        a.loss_partial[blockIdx.x] = acc;
        atomicAdd(a.loss_acc, acc);
    }
}

// occurrences [0, 2B): users (u_p | u'_p), [2B, 4B): items (i_p | i'_p)
template <int EPL>
__global__ __launch_bounds__(kBlock) void lrml_apply_kernel(LrmlArgs a) {
    const int gl = threadIdx.x & (kGL - 1);
    const int64_t q = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4;
    const int64_t B2 = 2 * (int64_t)a.B;
    if (q >= 2 * B2) return;
    const bool isU = q < B2;
    const int64_t o = isU ? q : q - B2;
    if ((isU ? a.rankU : a.rankV)[o] != 0) return;
    const int32_t* ids = o < a.B ? a.pos : a.neg;
    const int64_t r = ids[2 * (o < a.B ? o : o - a.B) + (isU ? 0 : 1)];
    float* X = isU ? a.U : a.V;
    float* A = isU ? a.AU : a.AV;
    float* G = isU ? a.GU : a.GV;
    float x[EPL], acc[EPL], g[EPL];
    gload<EPL>(X, r, a.d, gl, x);
    gload<EPL>(G, r, a.d, gl, g);
    gload_acc<EPL>(A, r, a.d, gl, true, acc);
    adagrad_row<EPL, VecRows>(X, A, r, a.d, gl, 0, x, acc, g, a.lr, true, a.clip_norm);
    row_zero<EPL>(G + r * (int64_t)a.d, a.d, gl);
    if (gl == 0) (isU ? a.cntU : a.cntV)[r] = 0;
}

// (user, item) scores -> order-preserving keys (topk_kernel input): a block
// per kLrmlScoreItems items of one user, one 16-lane group per item.  Group
// per item, not lane per item: the group reads V_i coalesced and holds e, rel
// in d / 16 registers per lane, the Key^T / Mem rows it reads from LDS are
// consecutive words (and the same words in the wave's four groups: one
// broadcast read), and the softmax over the factor axis is one max and one
// sum butterfly on DPP per memory slot.  A lane per item would hold rel[d] in
// up to 128 registers and read V with a stride of d words.
template <int EPL, int KMAX, int MODE>
__global__ __launch_bounds__(kBlock) void lrml_score_kernel(LrmlScoreArgs a) {
    __shared__ float s_k[KMAX], s_m[KMAX];
    __shared__ float s_w[kGroupsPerBlock][kLrmlMaxM];
    const int d = a.d, M = a.M;
    lrml_stage(a.Key, a.Mem, d, M, s_k, s_m);
    const int gl = threadIdx.x & (kGL - 1), grp = threadIdx.x >> 4;
    const int c = blockIdx.y;
    const int64_t u = a.users[c];
    int idx[EPL];
    bool ok[EPL];
    lrml_slots<EPL>(d, gl, idx, ok);
    float uu[EPL], pad[EPL];
    gload<EPL>(a.U, u, d, gl, uu);
#pragma unroll
    for (int s = 0; s < EPL; ++s) pad[s] = ok[s] ? 0.f : -INFINITY;
    const int64_t it0 = (int64_t)blockIdx.x * kLrmlScoreItems + grp;
#pragma unroll 1   // one item in flight per group: the unrolled memory-slot loops are the body
    for (int t = 0; t < kLrmlScoreItems / kGroupsPerBlock; ++t) {
        const int64_t it = it0 + (int64_t)t * kGroupsPerBlock;
        if (it >= a.n_items) break;   // group-uniform
        float vi[EPL], e[EPL], rel[EPL];
        gload<EPL>(a.V, it, d, gl, vi);
#pragma unroll
        for (int s = 0; s < EPL; ++s) e[s] = uu[s] * vi[s];
        if (MODE == 0) {   // lrml.py:95-100: softmax over the factor axis, per memory slot
            // M d exponentials per pair: the pass is bound by VALU issue, so the
            // inner loop is kept short -- a padding slot's x is 0 * key - inf (no
            // branch around its LDS read), exp is the hardware exp2 of x log2(e)
            // (x <= 0 after the maximum: |error| <= 2 ulp + |x| 2^-24) and 1 / sum
            // the hardware reciprocal (1 ulp), against the rtol 1e-4 of the scores
#pragma unroll
            for (int s = 0; s < EPL; ++s) rel[s] = 0.f;
            for (int n = 0; n < M; ++n) {
                const float* kr = s_k + n * d;
                const float* mr = s_m + n * d;
                float x[EPL], xm = -INFINITY;
#pragma unroll
                for (int s = 0; s < EPL; ++s) {
                    x[s] = fmaf(e[s], kr[idx[s]], pad[s]);
                    xm = fmaxf(xm, x[s]);
                }
                xm = gmax(xm);
                float sum = 0.f;
#pragma unroll
                for (int s = 0; s < EPL; ++s) {
                    x[s] = __expf(x[s] - xm);
                    sum += x[s];
                }
                const float inv = __builtin_amdgcn_rcpf(gsum(sum));
#pragma unroll
                for (int s = 0; s < EPL; ++s) rel[s] = fmaf(x[s] * inv, mr[idx[s]], rel[s]);
            }
        } else {
            float al[4];
            lrml_attend<EPL, 2>(e, idx, ok, s_k, s_m, d, M, gl, s_w[grp], al, rel);
        }
        float dv[EPL];
#pragma unroll
        for (int s = 0; s < EPL; ++s) dv[s] = ok[s] ? (uu[s] + rel[s]) - vi[s] : 0.f;
        const float sc = -gdot<EPL>(dv, dv);
        if (gl == 0) {
            uint32_t key = float_key(sc);
            if (a.exclude_train && sorted_contains(a.indices, a.indptr[u], a.indptr[u + 1], (int32_t)it)) key = 0u;
            a.keys[(int64_t)c * a.n_items + it] = key;
        }
    }
}

}  // namespace cfk

using namespace cfk;

struct cf_lrml {
    int64_t n_users = 0, n_items = 0;
    int d = 0, M = 0;
    float margin = 0.2f, clip_norm = 1.f, lr = 0.01f, acc_init = 0.1f;
    int device = 0;
    hipStream_t stream = nullptr;
    cfi::DevBuf<float> U, V, Key, Mem, AU, AV, GU, GV;
    cfi::DevBuf<int32_t> cntU, cntV;
    cfi::DevBuf<int64_t> indptr;
    cfi::DevBuf<int32_t> indices;
    cfi::DevBuf<int32_t> ids;    // pos [B,2] | neg [B,2] | rankU [2B] | rankV [2B]
    cfi::DevBuf<double> loss_partial;
    cfi::DevBuf<double> loss_acc;
    std::vector<double> h_loss;
    bool clip_pending = true;  // the full-table clip after the next step
};

namespace {

float* lrml_table(cf_lrml* e, int t, int64_t* n) {
    const int64_t nu = e->n_users * e->d, ni = e->n_items * e->d, nk = (int64_t)e->d * e->M;
    switch (t) {
        case 0: *n = nu; return e->U;
        case 1: *n = ni; return e->V;
        case 2: *n = nk; return e->Key;
        case 3: *n = nk; return e->Mem;
        case 4: *n = nu; return e->AU;
        case 5: *n = ni; return e->AV;
        default: *n = 0; return nullptr;
    }
}

bool lrml_small(const cf_lrml* e) { return e->d * e->M <= kLrmlSmall; }

hipError_t launch_lrml_step(const cf_lrml* e, const LrmlArgs& a, int blocks) {
    return with_epl<8>(a.d, [&](auto w) {
        constexpr int E = decltype(w)::value;
        if (lrml_small(e))
            hipLaunchKernelGGL((lrml_step_kernel<E, kLrmlSmall>), dim3(blocks), dim3(kBlock), 0, e->stream, a);
        else
            hipLaunchKernelGGL((lrml_step_kernel<E, kLrmlLarge>), dim3(blocks), dim3(kBlock), 0, e->stream, a);
    });
}

hipError_t launch_lrml_apply(const cf_lrml* e, const LrmlArgs& a) {
    const int blocks = (4 * a.B + kGroupsPerBlock - 1) / kGroupsPerBlock;
    return with_epl<8>(a.d, [&](auto w) {
        hipLaunchKernelGGL(lrml_apply_kernel<decltype(w)::value>, dim3(blocks), dim3(kBlock), 0, e->stream, a);
    });
}

template <int MODE>
hipError_t launch_lrml_score_m(const cf_lrml* e, const LrmlScoreArgs& a, dim3 grid) {
    return with_epl<8>(a.d, [&](auto w) {
        constexpr int E = decltype(w)::value;
        if (lrml_small(e))
            hipLaunchKernelGGL((lrml_score_kernel<E, kLrmlSmall, MODE>), grid, dim3(kBlock), 0, e->stream, a);
        else
            hipLaunchKernelGGL((lrml_score_kernel<E, kLrmlLarge, MODE>), grid, dim3(kBlock), 0, e->stream, a);
    });
}

}  // namespace

extern "C" {

int cf_lrml_create(int64_t n_users, int64_t n_items, int32_t d, int32_t M, float margin, float clip_norm,
                   float lr, float acc_init, int32_t device, cf_lrml** out) {
    if (!out || n_users < 1 || n_items < 2 || !(lr > 0.f) || !(acc_init > 0.f) || !(clip_norm > 0.f) ||
        n_users > INT32_MAX || n_items > INT32_MAX)
        return cfi::set_error(CF_EINVAL, "bad LRML configuration");
    if (d < 1 || d > kLrmlMaxD) return cfi::set_error(CF_EINVAL, "LRML n_factors must be 1..128");
    if (M < 1 || M > kLrmlMaxM) return cfi::set_error(CF_EINVAL, "LRML n_memory must be 1..64");
    *out = nullptr;
    CF_TRY(cfi::open_device(device));
    cf_lrml* e = new cf_lrml();
    e->n_users = n_users; e->n_items = n_items; e->d = d; e->M = M;
    e->margin = margin; e->clip_norm = clip_norm; e->lr = lr; e->acc_init = acc_init; e->device = device;
    auto bail = [&](int r) { cf_lrml_destroy(e); return r; };
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(cfi::set_error(CF_EHIP, "hipStreamCreate failed"));
    const size_t nu = (size_t)n_users * d, ni = (size_t)n_items * d, nk = (size_t)d * M;
    int r;
    if ((r = e->U.reset(nu, "U")) || (r = e->AU.reset(nu, "AU")) || (r = e->GU.reset(nu, "GU")) ||
        (r = e->V.reset(ni, "V")) || (r = e->AV.reset(ni, "AV")) || (r = e->GV.reset(ni, "GV")) ||
        (r = e->Key.reset(nk, "Key")) || (r = e->Mem.reset(nk, "Mem")) ||
        (r = e->cntU.reset((size_t)n_users, "cntU")) || (r = e->cntV.reset((size_t)n_items, "cntV")) ||
        (r = e->loss_acc.reset(1, "loss_acc")))
        return bail(r);
    if (hipMemsetAsync(e->U, 0, nu * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->V, 0, ni * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->Key, 0, nk * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->Mem, 0, nk * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->GU, 0, nu * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->GV, 0, ni * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->cntU, 0, (size_t)n_users * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->cntV, 0, (size_t)n_items * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->loss_acc, 0, 8, e->stream) != hipSuccess ||
        launch_fill(e->AU, (int64_t)nu, acc_init, e->stream) != hipSuccess ||
        launch_fill(e->AV, (int64_t)ni, acc_init, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return bail(cfi::set_error(CF_EHIP, "LRML init failed"));
    *out = e;
    return CF_OK;
}

int cf_lrml_destroy(cf_lrml* e) {
    return cfi::destroy_object(e);
}

int cf_lrml_init_params(cf_lrml* e, float mean, float stddev, uint64_t seed) {
    if (!e) return cfi::set_error(CF_EINVAL, "null LRML object");
    CF_HIP(hipSetDevice(e->device));
    const int64_t nk = (int64_t)e->d * e->M;
    // tf.random_normal_initializer on all four tables (lrml.py:30-41): not truncated
    CF_HIP(launch_init_normal(e->U, e->n_users * e->d, mean, stddev, 0, mix64(seed ^ 0x11u), e->stream));
    CF_HIP(launch_init_normal(e->V, e->n_items * e->d, mean, stddev, 0, mix64(seed ^ 0x22u), e->stream));
    CF_HIP(launch_init_normal(e->Key, nk, mean, stddev, 0, mix64(seed ^ 0x33u), e->stream));
    CF_HIP(launch_init_normal(e->Mem, nk, mean, stddev, 0, mix64(seed ^ 0x44u), e->stream));
    CF_HIP(hipStreamSynchronize(e->stream));
    e->clip_pending = true;
    return CF_OK;
}

int cf_lrml_set_table(cf_lrml* e, int32_t t, const float* src, int64_t n) {
    if (!e) return cfi::set_error(CF_EINVAL, "null argument");
    int64_t want = 0;
    float* p = lrml_table(e, t, &want);
    CF_HIP(hipSetDevice(e->device));
    CF_TRY(cfi::copy_table_in(e->stream, p, want, src, n, "LRML"));
    if (t <= 1) e->clip_pending = true;
    return CF_OK;
}

int cf_lrml_get_table(cf_lrml* e, int32_t t, float* dst, int64_t n) {
    if (!e) return cfi::set_error(CF_EINVAL, "null argument");
    int64_t want = 0;
    const float* p = lrml_table(e, t, &want);
    CF_HIP(hipSetDevice(e->device));
    return cfi::copy_table_out(e->stream, p, want, dst, n, "LRML");
}

int cf_lrml_set_interactions(cf_lrml* e, const int64_t* indptr, const int32_t* indices, int64_t nnz) {
    if (!e) return cfi::set_error(CF_EINVAL, "null CSR");
    CF_TRY(cfi::check_csr(indptr, indices, nnz, e->n_users, e->n_items));
    CF_HIP(hipSetDevice(e->device));
    return cfi::upload_csr(e->stream, e->indptr, e->indices, indptr, indices, nnz, e->n_users);
}

int cf_lrml_step(cf_lrml* e, const int32_t* pos, const int32_t* neg, int32_t B, double* loss_out) {
    if (!e || !pos || !neg || B < 1) return cfi::set_error(CF_EINVAL, "bad arguments");
    if (B > (1 << 24)) return cfi::set_error(CF_EINVAL, "B must be <= 2^24");
    for (int p = 0; p < B; ++p) {
        if (pos[2 * p] < 0 || pos[2 * p] >= e->n_users || pos[2 * p + 1] < 0 || pos[2 * p + 1] >= e->n_items)
            return cfi::set_error(CF_EINVAL, "positive pair " + std::to_string(p) + " out of range");
        if (neg[2 * p] < 0 || neg[2 * p] >= e->n_users || neg[2 * p + 1] < 0 || neg[2 * p + 1] >= e->n_items)
            return cfi::set_error(CF_EINVAL, "negative pair " + std::to_string(p) + " out of range");
    }
    CF_HIP(hipSetDevice(e->device));
    const int nb = (B + kGroupsPerBlock - 1) / kGroupsPerBlock;
    CF_TRY(cfi::grow(e->stream, e->ids, (size_t)B * 8, "ids"));
    CF_TRY(cfi::grow(e->stream, e->loss_partial, (size_t)nb, "loss_partial"));
    CF_HIP(hipMemcpyAsync(e->ids, pos, (size_t)B * 8, hipMemcpyHostToDevice, e->stream));
    CF_HIP(hipMemcpyAsync(e->ids + 2 * (size_t)B, neg, (size_t)B * 8, hipMemcpyHostToDevice, e->stream));
    LrmlArgs a{};
    a.d = e->d; a.M = e->M; a.B = B;
    a.margin = e->margin; a.lr = e->lr; a.clip_norm = e->clip_norm;
    a.pos = e->ids; a.neg = e->ids + 2 * (size_t)B;
    a.rankU = e->ids + 4 * (size_t)B; a.rankV = e->ids + 6 * (size_t)B;
    a.Key = e->Key; a.Mem = e->Mem;
    a.U = e->U; a.AU = e->AU; a.GU = e->GU;
    a.V = e->V; a.AV = e->AV; a.GV = e->GV;
    a.cntU = e->cntU; a.cntV = e->cntV;
    a.loss_partial = e->loss_partial;
    a.loss_acc = e->loss_acc;
    CF_HIP(launch_lrml_step(e, a, nb));
    CF_HIP(launch_lrml_apply(e, a));
    if (e->clip_pending) {   // lrml.py:106-109 clips every row; later steps: fixed points
        CF_HIP(launch_clip_full(e->U, e->n_users, e->d, e->clip_norm, e->stream));
        CF_HIP(launch_clip_full(e->V, e->n_items, e->d, e->clip_norm, e->stream));
        e->clip_pending = false;
    }
    if (loss_out) CF_TRY(cfi::read_loss(e->stream, e->loss_partial, nb, e->h_loss, loss_out));
    return CF_OK;
}

int cf_lrml_take_loss(cf_lrml* e, double* sum_out) {
    if (!e || !sum_out) return cfi::set_error(CF_EINVAL, "null argument");
    CF_HIP(hipSetDevice(e->device));
    return cfi::take_loss(e->stream, e->loss_acc, sum_out);
}

int cf_lrml_score_topk(cf_lrml* e, const int32_t* users, int32_t n, int32_t k, int32_t exclude_train,
                       int32_t predict_mode, int32_t* idx_out, float* val_out) {
    if (!e) return cfi::set_error(CF_EINVAL, "bad arguments");
    if (predict_mode != CF_LRML_REFERENCE && predict_mode != CF_LRML_TRAIN)
        return cfi::set_error(CF_EINVAL, "predict_mode must be CF_LRML_REFERENCE or CF_LRML_TRAIN");
    CF_HIP(hipSetDevice(e->device));
    return cfi::score_topk_chunks(
        e->stream, "cf_lrml", e->n_users, e->n_items, e->indptr != nullptr, users, n, k, exclude_train, idx_out,
        val_out, true, [&](const int32_t* d_users, int m, uint32_t* keys, int32_t*, float*) {
            const dim3 grid((unsigned)((e->n_items + kLrmlScoreItems - 1) / kLrmlScoreItems), (unsigned)m);
            LrmlScoreArgs a{};
            a.d = e->d; a.M = e->M; a.n_items = e->n_items;
            a.users = d_users;
            a.U = e->U; a.V = e->V; a.Key = e->Key; a.Mem = e->Mem;
            a.keys = keys;
            a.exclude_train = exclude_train;
            a.indptr = e->indptr; a.indices = e->indices;
            return predict_mode == CF_LRML_TRAIN ? launch_lrml_score_m<1>(e, a, grid)
                                                 : launch_lrml_score_m<0>(e, a, grid);
        });
}

}  // extern "C"
