// cf_pointwise.hip -- the pointwise family of src/models/basic/models
// (mf.py, svd.py, wrmf.py), the consumers of sampler_rating, on gfx950.
//
// Tables: U [n_users, d] and V [n_items, d]; SVD adds the dense kernel matrix
// K [d, d] (svd.py:29-31).  For a batch of B rows (u, i, r):
//   MF / WRMF  pred = <U_u, V_i>            (mf.py:62-68, wrmf.py:69-75)
//   SVD        pred = <U_u K, V_i>          (svd.py:65-71)
//   e = pred - r,  L = 1/2 sum (e s)^2 + reg 1/2 (sum |U_u|^2 + sum |V_i|^2)
// with s = float32(sqrt(weight)) (wrmf.py:60; s = 1 for MF and SVD; K is not
// regularised, svd.py:51-54), and with w = (e s) s:
//   MF / WRMF  dU_u = w V_i + reg U_u,        dV_i = w U_u + reg V_i
//   SVD        dU_u = e (K V_i) + reg U_u,    dV_i = e (K^T U_u) + reg V_i,
//              dK = sum_b e_b U_u (x) V_i.
// tf.train.AdagradOptimizer: the U and V gradients are IndexedSlices, so the
// rows of one table row are summed over the batch first and every distinct
// row takes one acc += g^2; x -= lr g / sqrt(acc); K's gradient is dense and
// every element of K takes the update every step.
//
// The batches of sampler_rating at negRatio 0 are rows [kB, (k+1)B) of
// trasR.nonzero(): a handful of users own all B rows and nearly every item is
// seen once.  So the host orders the batch's rows by user (a counting sort,
// users in order of first appearance, rows of a user in batch order) while it
// range-checks them, and one step is
//   pw_mf_kernel / pw_svd_kernel   a 16-lane group per row, 16 rows (a tile)
//       per block.  An item seen once takes Adagrad in registers; an item seen
//       more often stores its gradient row.  The user gradients of a tile meet
//       in LDS: the first row of a user's run inside the tile sums the run in
//       batch order; a run that lies inside one tile takes Adagrad there, one
//       that crosses tiles stores one partial row per (tile, user);
//   pw_apply_kernel                a group per deferred row: adds its partial
//       rows in a fixed order plus n reg x, then adagrad_row;
//   pw_kfold_kernel (SVD)          sums the per-block d x d partials of dK in
//       block order and applies K's dense Adagrad.
// No table is accumulated with float atomics: two runs from the same tables
// give the same bits in every table, and the same per-step loss (block
// partials added in block order).  Only the running sum behind
// cf_pw_take_loss takes one fp64 atomic per block, so its last bits may
// depend on the order the blocks arrive in.
//
// SVD: K (zero-padded to Dp = d rounded up to 16, row stride Dp + 2) and the
// tile's U and V rows are staged in LDS; P = U_b K, Q = V_b K^T and the dK
// tile products (e o U_b)^T V_b run on MFMA: P and Q on v_mfma_f32_16x16x4_f32
// (exact f32), dK on v_mfma_f64_16x16x4_f64 with fp64 block partials.
// The padding is zero, so no MFMA loop branches on d or B.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cf_engine.h"
#include "cf_host.h"
#include "cf_kernels_impl.h"

namespace cfk {

constexpr int kPwMaxD = 128;
constexpr int kPwTile = kGroupsPerBlock;   // rows per tile: the MFMA M extent, and dK's k extent
constexpr int kPwMaxBlocks = 512;          // SVD: blocks (= dK partials); a block takes consecutive tiles
constexpr int kPwEvalRows = kGroupsPerBlock;

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef double doublex4 __attribute__((ext_vector_type(4)));

struct PwArgs {
    int d, Dp, B, kind;
    float s, reg, lr;
    const int32_t* __restrict__ ui;       // [B, 2], ordered by user
    const float* __restrict__ r;          // [B]
    const int32_t* __restrict__ ustart;   // [B] first position of the row's user run
    const int32_t* __restrict__ ulen;     // [B] rows of that run
    const int32_t* __restrict__ icnt;     // [B] occurrences of the row's item in the batch
    float* __restrict__ U; float* __restrict__ AU;
    float* __restrict__ V; float* __restrict__ AV;
    float* __restrict__ K; float* __restrict__ AK;
    float* __restrict__ part;             // [2B, d]: user partial rows at p, item gradient rows at B + p
    double* __restrict__ kpart;           // SVD: [blocks, Dp * Dp]
    int tiles, tiles_per_block, blocks;
    double* __restrict__ loss_partial;    // [blocks]
    double* __restrict__ loss_acc;
    // deferred rows: [0, n_def_u) users, [n_def_u, n_def) items
    int n_def, n_def_u;
    const int32_t* __restrict__ def_row;
    const int32_t* __restrict__ def_n;    // occurrences (the reg term's factor)
    const int32_t* __restrict__ def_ptr;  // [n_def + 1] into def_pos
    const int32_t* __restrict__ def_pos;  // rows of part, in the order they are added
};

struct PwEvalArgs {
    int d, kind;
    int64_t n;
    float lo, hi;
    const int32_t* __restrict__ ui;
    const float* __restrict__ r;
    const float* __restrict__ U; const float* __restrict__ V; const float* __restrict__ K;
    float* __restrict__ pred;             // nullable
    double* __restrict__ partial;         // [blocks, 2]
};

// the element each slot of this lane holds (row_ld's mapping), clamped into
// the row for reads of a padding slot
template <int EPL>
__device__ __forceinline__ void pw_slots(int d, int gl, int (&idx)[EPL], bool (&ok)[EPL]) {
    const bool full = vec_rows<EPL>() && d == kGL * EPL;
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
        const int e = elem_of<EPL>(s, gl, full);
        ok[s] = e < d;
        idx[s] = ok[s] ? e : 0;
    }
}

// Both sides of one tile's update, called by every thread of the block.  gu /
// gv: the row's gradient rows without the reg term.  s_g: [kPwTile][kGL * EPL]
// floats of LDS, slot-indexed.
template <int EPL>
__device__ __forceinline__ void pw_finish(const PwArgs& a, int p, int tile0, bool valid, int64_t u, int64_t i,
                                          int gl, int grp, const float (&uu)[EPL], const float (&vi)[EPL],
                                          const float (&gu)[EPL], const float (&gv)[EPL], float* s_g) {
    constexpr int ROW = kGL * EPL;
    if (valid) {
        if (a.icnt[p] == 1) {   // the item's only row: Adagrad in registers
            float acc[EPL], g[EPL];
            gload_acc<EPL>(a.AV, i, a.d, gl, true, acc);
#pragma unroll
            for (int s = 0; s < EPL; ++s) g[s] = fmaf(a.reg, vi[s], gv[s]);
            adagrad_row<EPL, VecRows>(a.V, a.AV, i, a.d, gl, 0, vi, acc, g, a.lr, false, 0.f);
        } else {
            gstore<EPL>(a.part, (int64_t)a.B + p, a.d, gl, gv);
        }
    }
#pragma unroll
    for (int s = 0; s < EPL; ++s) s_g[grp * ROW + s * kGL + gl] = valid ? gu[s] : 0.f;
    __syncthreads();
    if (valid) {
        const int us = a.ustart[p], ue = us + a.ulen[p];
        if (p == max(us, tile0)) {   // the run's first row inside this tile sums it, in batch order
            const int n = min(ue, tile0 + kPwTile) - p;
            float g[EPL];
#pragma unroll
            for (int s = 0; s < EPL; ++s) g[s] = gu[s];
            for (int q = 1; q < n; ++q) {
#pragma unroll
                for (int s = 0; s < EPL; ++s) g[s] += s_g[(grp + q) * ROW + s * kGL + gl];
            }
            if (us >= tile0 && ue <= tile0 + kPwTile) {   // the whole run: no other tile reads or writes U_u
                float acc[EPL];
                gload_acc<EPL>(a.AU, u, a.d, gl, true, acc);
                const float nr = (float)n * a.reg;
#pragma unroll
                for (int s = 0; s < EPL; ++s) g[s] = fmaf(nr, uu[s], g[s]);
                adagrad_row<EPL, VecRows>(a.U, a.AU, u, a.d, gl, 0, uu, acc, g, a.lr, false, 0.f);
            } else {
                gstore<EPL>(a.part, p, a.d, gl, g);
            }
        }
    }
    __syncthreads();   // s_g is written again by the block's next tile
}

// the block's pre-update loss: the groups' values added in group order in fp64
__device__ __forceinline__ void pw_fold_loss(const PwArgs& a, double mine, int gl, int grp, double* s_l) {
    if (gl == 0) s_l[grp] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int g = 0; g < kGroupsPerBlock; ++g) acc += s_l[g];
        a.loss_partial[blockIdx.x] = acc;
        atomicAdd(a.loss_acc, acc);
    }
}

template <int EPL>
__global__ __launch_bounds__(kBlock) void pw_mf_kernel(PwArgs a) {
    __shared__ float s_g[kPwTile * kGL * EPL];
    __shared__ double s_l[kGroupsPerBlock];
    const int gl = threadIdx.x & (kGL - 1), grp = threadIdx.x >> 4;
    const int tile0 = blockIdx.x * kPwTile, p = tile0 + grp;
    const bool valid = p < a.B;
    float uu[EPL], vi[EPL], gu[EPL], gv[EPL];
    int64_t u = 0, i = 0;
    float lossf = 0.f;
#pragma unroll
    for (int s = 0; s < EPL; ++s) uu[s] = vi[s] = gu[s] = gv[s] = 0.f;
    if (valid) {
        u = a.ui[2 * p];
        i = a.ui[2 * p + 1];
        gload<EPL>(a.U, u, a.d, gl, uu);
        gload<EPL>(a.V, i, a.d, gl, vi);
        const float e = gdot<EPL>(uu, vi) - a.r[p];
        const float es = e * a.s, w = es * a.s;   // l2_loss((pred - r) * sqrt(weight)), wrmf.py:60
        lossf = 0.5f * es * es + 0.5f * a.reg * (gdot<EPL>(uu, uu) + gdot<EPL>(vi, vi));
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            gu[s] = w * vi[s];
            gv[s] = w * uu[s];
        }
    }
    pw_finish<EPL>(a, p, tile0, valid, u, i, gl, grp, uu, vi, gu, gv, s_g);
    pw_fold_loss(a, (double)lossf, gl, grp, s_l);
}

// out tile [16 rows][16 columns at n0] = A [16][Dp] (row stride ld) times
// B[k][n] = *(b + k * bk + n * bn), on 16x16x4 f32 MFMA: lane l feeds
// A[l & 15][k0 + (l >> 4)] and B[k0 + (l >> 4)][l & 15]; two accumulators
// alternate (the dependent-accumulator latency exceeds the issue interval)
__device__ __forceinline__ floatx4 pw_mma_tile(const float* A, int ld, const float* b, int bk, int bn, int Dp,
                                               int lane) {
    const int c = lane & 15, q = lane >> 4;
    const float* ap = A + c * ld + q;
    const float* bp = b + q * bk + c * bn;
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < Dp; k0 += 8) {   // Dp is a multiple of 16
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0], bp[k0 * bk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0 + 4], bp[(k0 + 4) * bk], acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// NT2: d x d output tiles of dK per wave, (Dp / 16)^2 / 4 rounded up
template <int EPL, int NT2>
__global__ __launch_bounds__(kBlock) void pw_svd_kernel(PwArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    __shared__ double s_l[kGroupsPerBlock];
    const int d = a.d, Dp = a.Dp, LD = Dp + 2, NT = Dp >> 4;
    // K [Dp][LD] | U tile, V tile, P, Q: [16][LD] each; the user gradients reuse P and Q
    // (16 * 16 EPL floats <= 32 LD at every width)
    float* sK = s_dyn;
    float* sU = sK + Dp * LD;
    float* sV = sU + kPwTile * LD;
    float* sP = sV + kPwTile * LD;
    float* sQ = sP + kPwTile * LD;
    const int gl = threadIdx.x & (kGL - 1), grp = threadIdx.x >> 4;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    for (int t = threadIdx.x; t < Dp * LD; t += kBlock) {
        const int k = t / LD, n = t - k * LD;
        sK[t] = (k < d && n < d) ? a.K[k * d + n] : 0.f;
    }
    int idx[EPL];
    bool ok[EPL];
    pw_slots<EPL>(d, gl, idx, ok);
    doublex4 kacc[NT2];
#pragma unroll
    for (int t = 0; t < NT2; ++t) kacc[t] = doublex4{0.0, 0.0, 0.0, 0.0};
    double loss = 0.0;
    const int t_begin = blockIdx.x * a.tiles_per_block;
    const int t_end = min(a.tiles, t_begin + a.tiles_per_block);
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int tile0 = tile * kPwTile, p = tile0 + grp;
        const bool valid = p < a.B;
        float uu[EPL], vi[EPL], gu[EPL], gv[EPL];
        int64_t u = 0, i = 0;
#pragma unroll
        for (int s = 0; s < EPL; ++s) uu[s] = vi[s] = 0.f;
        if (valid) {
            u = a.ui[2 * p];
            i = a.ui[2 * p + 1];
            gload<EPL>(a.U, u, d, gl, uu);
            gload<EPL>(a.V, i, d, gl, vi);
        }
        // the group's rows into the tiles, zero beyond d and beyond B
        for (int e = gl; e < LD; e += kGL) sU[grp * LD + e] = sV[grp * LD + e] = 0.f;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < EPL; ++s)
            if (ok[s]) {
                sU[grp * LD + idx[s]] = uu[s];
                sV[grp * LD + idx[s]] = vi[s];
            }
        __syncthreads();   // tiles (and, the first time, K) staged
        // P = U_b K (B[k][n] = K[k][n]) and Q = V_b K^T (B[k][n] = K[n][k]): 2 NT column tiles
        for (int j = wave; j < 2 * NT; j += kWavesPerBlock) {
            const bool isQ = j >= NT;
            const int n0 = (isQ ? j - NT : j) << 4;
            const floatx4 acc = pw_mma_tile(isQ ? sV : sU, LD, sK + (isQ ? n0 * LD : n0), isQ ? 1 : LD,
                                            isQ ? LD : 1, Dp, lane);
            float* out = (isQ ? sQ : sP) + ((lane >> 4) * 4) * LD + n0 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) out[r * LD] = acc[r];
        }
        __syncthreads();
        float pr[EPL], qr[EPL], e = 0.f;
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            pr[s] = ok[s] ? sP[grp * LD + idx[s]] : 0.f;
            qr[s] = ok[s] ? sQ[grp * LD + idx[s]] : 0.f;
        }
        if (valid) {
            e = gdot<EPL>(pr, vi) - a.r[p];
            loss += (double)(0.5f * e * e + 0.5f * a.reg * (gdot<EPL>(uu, uu) + gdot<EPL>(vi, vi)));
        }
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
            gu[s] = e * qr[s];   // e (K V_i)
            gv[s] = e * pr[s];   // e (K^T U_u)
            if (ok[s]) sU[grp * LD + idx[s]] = e * uu[s];   // dK's A operand: (e o U_b)^T
        }
        __syncthreads();   // P and Q are read: sP becomes the user-gradient buffer
        pw_finish<EPL>(a, p, tile0, valid, u, i, gl, grp, uu, vi, gu, gv, sP);
        // dK[m][n] += sum_b (e_b U_b[m]) V_b[n]: A[i][k] = sU[k][m0 + i], B[k][j] = sV[k][n0 + j], k = 16 rows.
        // On the f64 MFMA (operands as the f32 16x16x4 form): the sum over the batch in float32
        // alone moves the ten-step trajectory out of the parity band
#pragma unroll
        for (int t = 0; t < NT2; ++t) {
            const int job = wave + t * kWavesPerBlock;
            if (job < NT * NT) {   // wave-uniform
                const int m0 = (job / NT) << 4, n0 = (job % NT) << 4;
                // lane quarter q takes rows kq + 0..3: quarters 0 and 1 (and 2 and 3), which share
                // an LDS cycle, read rows 8 apart -- 8 LD = 16 (mod 32) banks: no conflict
                const int kq = 8 * ((lane >> 4) & 1) + 4 * (lane >> 5);
                const float* ap = sU + kq * LD + m0 + (lane & 15);
                const float* bp = sV + kq * LD + n0 + (lane & 15);
#pragma unroll
                for (int k0 = 0; k0 < 4; ++k0)
                    kacc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)ap[k0 * LD], (double)bp[k0 * LD], kacc[t],
                                                                   0, 0, 0);
            }
        }
        __syncthreads();   // the tiles are staged again
    }
    // the block's dK partial, [Dp][Dp]; the f64 MFMA's D[i = (lane >> 4) + 4 r][j = lane & 15]
    double* kp = a.kpart + (int64_t)blockIdx.x * Dp * Dp;
#pragma unroll
    for (int t = 0; t < NT2; ++t) {
        const int job = wave + t * kWavesPerBlock;
        if (job < NT * NT) {
            const int m0 = (job / NT) << 4, n0 = (job % NT) << 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) kp[(m0 + (lane >> 4) + 4 * r) * Dp + n0 + (lane & 15)] = kacc[t][r];
        }
    }
    pw_fold_loss(a, loss, gl, grp, s_l);
}

// dK = the blocks' partials added in block order; dense Adagrad on K (svd.py:76)
__global__ __launch_bounds__(kBlock) void pw_kfold_kernel(PwArgs a) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= a.d * a.d) return;
    const int m = t / a.d, n = t - m * a.d;
    const double* kp = a.kpart + m * a.Dp + n;
    double gd = 0.0;
    for (int b = 0; b < a.blocks; ++b) gd += kp[(int64_t)b * a.Dp * a.Dp];
    const float g = (float)gd;
    const float acc = fmaf(g, g, a.AK[t]);
    a.AK[t] = acc;
    a.K[t] -= adagrad_delta(a.lr, g, acc);
}

template <int EPL>
__global__ __launch_bounds__(kBlock) void pw_apply_kernel(PwArgs a) {
    const int gl = threadIdx.x & (kGL - 1);
    const int q = (int)(((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4);
    if (q >= a.n_def) return;
    const bool isU = q < a.n_def_u;
    const int64_t r = a.def_row[q];
    float* X = isU ? a.U : a.V;
    float* A = isU ? a.AU : a.AV;
    float x[EPL], acc[EPL], g[EPL], t[EPL];
    gload<EPL>(X, r, a.d, gl, x);
    gload_acc<EPL>(A, r, a.d, gl, true, acc);
#pragma unroll
    for (int s = 0; s < EPL; ++s) g[s] = 0.f;
    for (int k = a.def_ptr[q]; k < a.def_ptr[q + 1]; ++k) {
        gload<EPL>(a.part, a.def_pos[k], a.d, gl, t);
#pragma unroll
        for (int s = 0; s < EPL; ++s) g[s] += t[s];
    }
    const float nr = (float)a.def_n[q] * a.reg;
#pragma unroll
    for (int s = 0; s < EPL; ++s) g[s] = fmaf(nr, x[s], g[s]);
    adagrad_row<EPL, VecRows>(X, A, r, a.d, gl, 0, x, acc, g, a.lr, false, 0.f);
}

// clip(predict) per tuple (mf.py:77-79, svd.py:80-82) and the block's
// sum |r - p|, sum (r - p)^2 in fp64, added in group order
template <int EPL>
__global__ __launch_bounds__(kBlock) void pw_eval_kernel(PwEvalArgs a) {
    __shared__ float s_u[kGroupsPerBlock][kPwMaxD];
    __shared__ double s_a[kGroupsPerBlock], s_q[kGroupsPerBlock];
    const int gl = threadIdx.x & (kGL - 1), grp = threadIdx.x >> 4;
    const int64_t p = (int64_t)blockIdx.x * kPwEvalRows + grp;
    double ab = 0.0, sq = 0.0;
    if (p < a.n) {
        const int64_t u = a.ui[2 * p], i = a.ui[2 * p + 1];
        float uu[EPL], vi[EPL];
        gload<EPL>(a.U, u, a.d, gl, uu);
        gload<EPL>(a.V, i, a.d, gl, vi);
        if (a.kind == CF_PW_SVD) {   // uu <- U_u K, through the group's LDS row
            int idx[EPL];
            bool ok[EPL];
            pw_slots<EPL>(a.d, gl, idx, ok);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int s = 0; s < EPL; ++s)
                if (ok[s]) s_u[grp][idx[s]] = uu[s];
            __builtin_amdgcn_wave_barrier();
            float y[EPL];
#pragma unroll
            for (int s = 0; s < EPL; ++s) y[s] = 0.f;
            for (int k = 0; k < a.d; ++k) {
                const float uk = s_u[grp][k];
                const float* row = a.K + k * a.d;
#pragma unroll
                for (int s = 0; s < EPL; ++s) y[s] = fmaf(uk, row[idx[s]], y[s]);
            }
#pragma unroll
            for (int s = 0; s < EPL; ++s) uu[s] = ok[s] ? y[s] : 0.f;
        }
        const float pred = fminf(fmaxf(gdot<EPL>(uu, vi), a.lo), a.hi);
        if (gl == 0 && a.pred) a.pred[p] = pred;
        const double dlt = (double)a.r[p] - (double)pred;
        ab = fabs(dlt);
        sq = dlt * dlt;
    }
    if (gl == 0) {
        s_a[grp] = ab;
        s_q[grp] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0.0, t1 = 0.0;
        for (int g = 0; g < kGroupsPerBlock; ++g) {
            t0 += s_a[g];
            t1 += s_q[g];
        }
        a.partial[2 * (int64_t)blockIdx.x] = t0;
        a.partial[2 * (int64_t)blockIdx.x + 1] = t1;
    }
}

}  // namespace cfk

using namespace cfk;

struct cf_pw {
    int64_t n_users = 0, n_items = 0;
    int d = 0, Dp = 0, kind = 0;
    float weight = 1.f, s = 1.f, reg = 0.f, lr = 0.1f, acc_init = 0.1f;
    int device = 0;
    hipStream_t stream = nullptr;
    cfi::DevBuf<float> U, V, K, AU, AV, AK;
    cfi::DevBuf<int64_t> indptr;
    cfi::DevBuf<int32_t> indices;
    cfi::DevBuf<int32_t> meta;          // the step's host-built arrays (PwMeta)
    cfi::DevBuf<float> part;            // [2 B, d]
    cfi::DevBuf<double> kpart;          // [min(kPwMaxBlocks, tiles), Dp * Dp], SVD
    cfi::DevBuf<double> loss_partial;   // [tiles]
    cfi::DevBuf<double> loss_acc;
    std::vector<double> h_loss;
    std::vector<int32_t> h_meta, ucnt, icnt, upos;   // ucnt / icnt: zero between steps
};

namespace {

// one allocation of 14 B + 1 words carved into the step's arrays, on the host and on the device
struct PwMeta {
    int32_t* ui;        // [B, 2] the batch ordered by user
    float* r;           // [B]
    int32_t *ustart, *ulen, *icnt;   // [B] each
    int32_t *def_row, *def_n;        // [2 B] each
    int32_t* def_ptr;   // [2 B + 1]
    int32_t* def_pos;   // [2 B]
};
constexpr size_t pw_meta_words(int B) { return (size_t)14 * B + 1; }
PwMeta pw_meta(int32_t* base, int B) {
    PwMeta m;
    m.ui = base;
    m.r = reinterpret_cast<float*>(base + 2 * (size_t)B);
    m.ustart = base + 3 * (size_t)B;
    m.ulen = m.ustart + B;
    m.icnt = m.ulen + B;
    m.def_row = m.icnt + B;
    m.def_n = m.def_row + 2 * (size_t)B;
    m.def_ptr = m.def_n + 2 * (size_t)B;
    m.def_pos = m.def_ptr + 2 * (size_t)B + 1;
    return m;
}

float* pw_table(cf_pw* e, int t, int64_t* n) {
    const int64_t nu = e->n_users * e->d, ni = e->n_items * e->d;
    const int64_t nk = e->kind == CF_PW_SVD ? (int64_t)e->d * e->d : 0;
    switch (t) {
        case 0: *n = nu; return e->U;
        case 1: *n = ni; return e->V;
        case 2: *n = nk; return e->K;
        case 3: *n = nu; return e->AU;
        case 4: *n = ni; return e->AV;
        case 5: *n = nk; return e->AK;
        default: *n = 0; return nullptr;
    }
}

size_t pw_svd_lds(int Dp) { return (size_t)(Dp + 4 * kPwTile) * (Dp + 2) * sizeof(float); }

template <int EPL, int NT2>
hipError_t launch_pw_svd_e(const cf_pw* e, const PwArgs& a) {
    const size_t lds = pw_svd_lds(a.Dp);
    hipError_t he = hipFuncSetAttribute((const void*)pw_svd_kernel<EPL, NT2>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (he != hipSuccess) return he;
    hipLaunchKernelGGL((pw_svd_kernel<EPL, NT2>), dim3(a.blocks), dim3(kBlock), lds, e->stream, a);
    return hipGetLastError();
}

hipError_t launch_pw_grad(const cf_pw* e, const PwArgs& a) {
    if (e->kind != CF_PW_SVD)
        return with_epl<8>(a.d, [&](auto w) {
            hipLaunchKernelGGL(pw_mf_kernel<decltype(w)::value>, dim3(a.blocks), dim3(kBlock), 0, e->stream, a);
        });
    switch (epl_for(a.d)) {   // (Dp / 16)^2 dK tiles over four waves
        case 1: return launch_pw_svd_e<1, 1>(e, a);
        case 2: return launch_pw_svd_e<2, 1>(e, a);
        case 4: return launch_pw_svd_e<4, 4>(e, a);
        default: return launch_pw_svd_e<8, 16>(e, a);
    }
}

hipError_t launch_pw_apply(const cf_pw* e, const PwArgs& a) {
    if (a.n_def == 0) return hipSuccess;
    const int blocks = (a.n_def + kGroupsPerBlock - 1) / kGroupsPerBlock;
    return with_epl<8>(a.d, [&](auto w) {
        hipLaunchKernelGGL(pw_apply_kernel<decltype(w)::value>, dim3(blocks), dim3(kBlock), 0, e->stream, a);
    });
}

}  // namespace

extern "C" {

int cf_pw_create(int64_t n_users, int64_t n_items, int32_t d, int32_t kind, float weight, float reg, float lr,
                 float acc_init, int32_t device, cf_pw** out) {
    if (!out || n_users < 1 || n_items < 2 || !(lr > 0.f) || !(acc_init > 0.f) || !(reg >= 0.f) ||
        !(weight > 0.f) || !std::isfinite(weight) || n_users > INT32_MAX || n_items > INT32_MAX)
        return cfi::set_error(CF_EINVAL, "bad pointwise configuration");
    if (d < 1 || d > kPwMaxD) return cfi::set_error(CF_EINVAL, "pointwise n_factors must be 1..128");
    if (kind != CF_PW_MF && kind != CF_PW_SVD) return cfi::set_error(CF_EINVAL, "kind must be CF_PW_MF or CF_PW_SVD");
    if (kind == CF_PW_SVD && weight != 1.f) return cfi::set_error(CF_EINVAL, "SVD takes weight 1");
    *out = nullptr;
    CF_TRY(cfi::open_device(device));
    cf_pw* e = new cf_pw();
    e->n_users = n_users; e->n_items = n_items; e->d = d; e->Dp = (d + 15) & ~15; e->kind = kind;
    e->weight = weight; e->s = (float)std::sqrt((double)weight);   // np.sqrt(weight) as a float32 constant
    e->reg = reg; e->lr = lr; e->acc_init = acc_init; e->device = device;
    e->ucnt.assign((size_t)n_users, 0);
    e->icnt.assign((size_t)n_items, 0);
    e->upos.assign((size_t)n_users, 0);
    auto bail = [&](int r) { cf_pw_destroy(e); return r; };
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(cfi::set_error(CF_EHIP, "hipStreamCreate failed"));
    const size_t nu = (size_t)n_users * d, ni = (size_t)n_items * d;
    const size_t nk = kind == CF_PW_SVD ? (size_t)d * d : 0;
    int r;
    if ((r = e->U.reset(nu, "U")) || (r = e->AU.reset(nu, "AU")) || (r = e->V.reset(ni, "V")) ||
        (r = e->AV.reset(ni, "AV")) || (r = e->K.reset(nk, "K")) || (r = e->AK.reset(nk, "AK")) ||
        (r = e->loss_acc.reset(1, "loss_acc")))
        return bail(r);
    if (hipMemsetAsync(e->U, 0, nu * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->V, 0, ni * 4, e->stream) != hipSuccess ||
        (nk && hipMemsetAsync(e->K, 0, nk * 4, e->stream) != hipSuccess) ||
        hipMemsetAsync(e->loss_acc, 0, 8, e->stream) != hipSuccess ||
        launch_fill(e->AU, (int64_t)nu, acc_init, e->stream) != hipSuccess ||
        launch_fill(e->AV, (int64_t)ni, acc_init, e->stream) != hipSuccess ||
        (nk && launch_fill(e->AK, (int64_t)nk, acc_init, e->stream) != hipSuccess) ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return bail(cfi::set_error(CF_EHIP, "pointwise init failed"));
    *out = e;
    return CF_OK;
}

int cf_pw_destroy(cf_pw* e) {
    return cfi::destroy_object(e);
}

int cf_pw_init_params(cf_pw* e, float mean, float stddev, int32_t truncated, uint64_t seed) {
    if (!e) return cfi::set_error(CF_EINVAL, "null pointwise object");
    CF_HIP(hipSetDevice(e->device));
    const int tr = truncated ? 1 : 0;   // tf.truncated_normal_initializer on every table (mf.py:26-31, svd.py:26-34)
    CF_HIP(launch_init_normal(e->U, e->n_users * e->d, mean, stddev, tr, mix64(seed ^ 0x51u), e->stream));
    CF_HIP(launch_init_normal(e->V, e->n_items * e->d, mean, stddev, tr, mix64(seed ^ 0x52u), e->stream));
    if (e->kind == CF_PW_SVD)
        CF_HIP(launch_init_normal(e->K, (int64_t)e->d * e->d, mean, stddev, tr, mix64(seed ^ 0x53u), e->stream));
    CF_HIP(hipStreamSynchronize(e->stream));
    return CF_OK;
}

int cf_pw_set_table(cf_pw* e, int32_t t, const float* src, int64_t n) {
    if (!e || !src) return cfi::set_error(CF_EINVAL, "null argument");
    int64_t want = 0;
    float* p = pw_table(e, t, &want);
    if (!p) return cfi::set_error(CF_EINVAL, "no such pointwise table (K and AK: SVD only)");
    CF_HIP(hipSetDevice(e->device));
    return cfi::copy_table_in(e->stream, p, want, src, n, "pointwise");
}

int cf_pw_get_table(cf_pw* e, int32_t t, float* dst, int64_t n) {
    if (!e || !dst) return cfi::set_error(CF_EINVAL, "null argument");
    int64_t want = 0;
    float* p = pw_table(e, t, &want);
    if (!p) return cfi::set_error(CF_EINVAL, "no such pointwise table (K and AK: SVD only)");
    CF_HIP(hipSetDevice(e->device));
    return cfi::copy_table_out(e->stream, p, want, dst, n, "pointwise");
}

int cf_pw_set_interactions(cf_pw* e, const int64_t* indptr, const int32_t* indices, int64_t nnz) {
    if (!e) return cfi::set_error(CF_EINVAL, "null CSR");
    CF_TRY(cfi::check_csr(indptr, indices, nnz, e->n_users, e->n_items));
    CF_HIP(hipSetDevice(e->device));
    return cfi::upload_csr(e->stream, e->indptr, e->indices, indptr, indices, nnz, e->n_users);
}

int cf_pw_step(cf_pw* e, const int32_t* ui, const float* r, int32_t B, double* loss_out) {
    if (!e || !ui || !r || B < 1) return cfi::set_error(CF_EINVAL, "bad arguments");
    if (B > (1 << 24)) return cfi::set_error(CF_EINVAL, "B must be <= 2^24");
    for (int p = 0; p < B; ++p) {
        if (ui[2 * p] < 0 || ui[2 * p] >= e->n_users || ui[2 * p + 1] < 0 || ui[2 * p + 1] >= e->n_items)
            return cfi::set_error(CF_EINVAL, "row " + std::to_string(p) + " out of range");
        if (!std::isfinite(r[p])) return cfi::set_error(CF_EINVAL, "rating " + std::to_string(p) + " is not finite");
    }
    CF_HIP(hipSetDevice(e->device));
    const int tiles = (B + kPwTile - 1) / kPwTile;
    const bool svd = e->kind == CF_PW_SVD;
    const int tpb = svd ? (tiles + kPwMaxBlocks - 1) / kPwMaxBlocks : 1;
    const int blocks = (tiles + tpb - 1) / tpb;
    CF_TRY(cfi::grow(e->stream, e->meta, pw_meta_words(B), "meta"));
    CF_TRY(cfi::grow(e->stream, e->part, (size_t)2 * B * e->d, "part"));
    CF_TRY(cfi::grow(e->stream, e->loss_partial, (size_t)tiles, "loss_partial"));
    // the block count is not monotone in B (513 tiles: 257 blocks, 512 tiles: 512); this bound is
    if (svd) CF_TRY(cfi::grow(e->stream, e->kpart, (size_t)std::min(kPwMaxBlocks, tiles) * e->Dp * e->Dp, "kpart"));
    // the batch ordered by user: users in order of first appearance, a user's rows in batch order
    e->h_meta.assign(pw_meta_words(B), 0);
    const PwMeta m = pw_meta(e->h_meta.data(), B);
    int32_t *const s_ui = m.ui, *const ustart = m.ustart, *const ulen = m.ulen, *const icnt = m.icnt;
    int32_t *const def_row = m.def_row, *const def_n = m.def_n, *const def_ptr = m.def_ptr, *const def_pos = m.def_pos;
    float* const s_r = m.r;
    for (int p = 0; p < B; ++p) {
        e->ucnt[(size_t)ui[2 * p]]++;
        e->icnt[(size_t)ui[2 * p + 1]]++;
    }
    int next = 0;
    for (int p = 0; p < B; ++p) {   // run starts, then the rows in place
        const size_t u = (size_t)ui[2 * p];
        if (e->ucnt[u] > 0) {
            e->upos[u] = next;
            next += e->ucnt[u];
            e->ucnt[u] = -e->ucnt[u];   // negative: the run is placed, -length
        }
    }
    for (int p = 0; p < B; ++p) {
        const size_t u = (size_t)ui[2 * p];
        const int len = -e->ucnt[u];
        const int at = e->upos[u]++;
        s_ui[2 * at] = ui[2 * p];
        s_ui[2 * at + 1] = ui[2 * p + 1];
        s_r[at] = r[p];
        ulen[at] = len;
        icnt[at] = e->icnt[(size_t)ui[2 * p + 1]];
    }
    // deferred rows: user runs that cross a tile boundary, then items seen more than once
    int nd = 0, npos = 0;
    def_ptr[0] = 0;
    for (int p = 0; p < B;) {
        const int len = ulen[p], end = p + len;
        for (int q = p; q < end; ++q) ustart[q] = p;
        if (p / kPwTile != (end - 1) / kPwTile) {
            def_row[nd] = s_ui[2 * p];
            def_n[nd] = len;
            for (int q = p; q < end; q = (q / kPwTile + 1) * kPwTile) def_pos[npos++] = q;
            def_ptr[++nd] = npos;
        }
        e->ucnt[(size_t)s_ui[2 * p]] = 0;
        p = end;
    }
    const int nd_u = nd;
    for (int p = 0; p < B; ++p) {   // icnt table: count > 1 -> the deferred entry's index + 2, negated
        const size_t i = (size_t)s_ui[2 * p + 1];
        if (icnt[p] > 1 && e->icnt[i] > 0) {
            def_row[nd] = (int32_t)i;
            def_n[nd] = icnt[p];
            def_ptr[nd + 1] = def_ptr[nd] + icnt[p];
            e->icnt[i] = -(nd + 2);
            ++nd;
        }
    }
    {   // the positions of every duplicated item, in sorted batch order
        std::vector<int32_t> fill(def_ptr + nd_u, def_ptr + nd);
        for (int p = 0; p < B; ++p) {
            const size_t i = (size_t)s_ui[2 * p + 1];
            if (icnt[p] > 1) {
                const int q = -e->icnt[i] - 2;
                def_pos[fill[(size_t)(q - nd_u)]++] = B + p;
            }
        }
    }
    for (int p = 0; p < B; ++p) e->icnt[(size_t)s_ui[2 * p + 1]] = 0;

    CF_HIP(hipMemcpyAsync(e->meta, e->h_meta.data(), pw_meta_words(B) * 4, hipMemcpyHostToDevice, e->stream));
    const PwMeta dm = pw_meta(e->meta, B);
    PwArgs a{};
    a.d = e->d; a.Dp = e->Dp; a.B = B; a.kind = e->kind;
    a.s = e->s; a.reg = e->reg; a.lr = e->lr;
    a.ui = dm.ui; a.r = dm.r;
    a.ustart = dm.ustart; a.ulen = dm.ulen; a.icnt = dm.icnt;
    a.def_row = dm.def_row; a.def_n = dm.def_n; a.def_ptr = dm.def_ptr; a.def_pos = dm.def_pos;
    a.n_def = nd; a.n_def_u = nd_u;
    a.U = e->U; a.AU = e->AU; a.V = e->V; a.AV = e->AV; a.K = e->K; a.AK = e->AK;
    a.part = e->part; a.kpart = e->kpart;
    a.tiles = tiles; a.tiles_per_block = tpb; a.blocks = blocks;
    a.loss_partial = e->loss_partial;
    a.loss_acc = e->loss_acc;
    CF_HIP(launch_pw_grad(e, a));
    CF_HIP(launch_pw_apply(e, a));
    if (svd) {
        hipLaunchKernelGGL(pw_kfold_kernel, dim3((e->d * e->d + kBlock - 1) / kBlock), dim3(kBlock), 0, e->stream, a);
        CF_HIP(hipGetLastError());
    }
    if (loss_out) CF_TRY(cfi::read_loss(e->stream, e->loss_partial, blocks, e->h_loss, loss_out));
    return CF_OK;
}

int cf_pw_take_loss(cf_pw* e, double* sum_out) {
    if (!e || !sum_out) return cfi::set_error(CF_EINVAL, "null argument");
    CF_HIP(hipSetDevice(e->device));
    return cfi::take_loss(e->stream, e->loss_acc, sum_out);
}

int cf_pw_eval(cf_pw* e, const int32_t* ui, const float* r, int64_t n, float lo, float hi, float* pred_out,
               double* sums_out) {
    if (!e || n < 0 || !sums_out || (n > 0 && (!ui || !r))) return cfi::set_error(CF_EINVAL, "bad arguments");
    if (!(lo <= hi)) return cfi::set_error(CF_EINVAL, "the rating range needs lo <= hi");
    if (n > ((int64_t)1 << 30)) return cfi::set_error(CF_EINVAL, "n must be <= 2^30");
    sums_out[0] = sums_out[1] = 0.0;
    if (n == 0) return CF_OK;
    for (int64_t p = 0; p < n; ++p) {
        if (ui[2 * p] < 0 || ui[2 * p] >= e->n_users || ui[2 * p + 1] < 0 || ui[2 * p + 1] >= e->n_items)
            return cfi::set_error(CF_EINVAL, "tuple " + std::to_string(p) + " out of range");
        if (!std::isfinite(r[p])) return cfi::set_error(CF_EINVAL, "rating " + std::to_string(p) + " is not finite");
    }
    CF_HIP(hipSetDevice(e->device));
    const int64_t nb = (n + kPwEvalRows - 1) / kPwEvalRows;
    cfi::DevBuf<int32_t> d_ui;
    cfi::DevBuf<float> d_r, d_pred;
    cfi::DevBuf<double> d_part;
    CF_TRY(d_ui.reset((size_t)2 * n, "eval ui"));
    CF_TRY(d_r.reset((size_t)n, "eval r"));
    CF_TRY(d_pred.reset((size_t)(pred_out ? n : 0), "eval pred"));
    CF_TRY(d_part.reset((size_t)2 * nb, "eval partials"));
    std::vector<double> h_part((size_t)2 * nb);
    hipError_t he = hipMemcpyAsync(d_ui, ui, (size_t)n * 8, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d_r, r, (size_t)n * 4, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) {
        PwEvalArgs a{};
        a.d = e->d; a.kind = e->kind; a.n = n; a.lo = lo; a.hi = hi;
        a.ui = d_ui; a.r = d_r; a.U = e->U; a.V = e->V; a.K = e->K;
        a.pred = d_pred; a.partial = d_part;
        he = with_epl<8>(a.d, [&](auto w) {
            hipLaunchKernelGGL(pw_eval_kernel<decltype(w)::value>, dim3((unsigned)nb), dim3(kBlock), 0, e->stream, a);
        });
    }
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) he = hipMemcpy(h_part.data(), d_part, (size_t)2 * nb * 8, hipMemcpyDeviceToHost);
    if (he == hipSuccess && pred_out) he = hipMemcpy(pred_out, d_pred, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return cfi::set_error(CF_EHIP, std::string("cf_pw_eval: ") + hipGetErrorString(he));
    double t0 = 0.0, t1 = 0.0;
    for (int64_t b = 0; b < nb; ++b) {   // block order
        t0 += h_part[(size_t)(2 * b)];
        t1 += h_part[(size_t)(2 * b + 1)];
    }
    sums_out[0] = t0;
    sums_out[1] = t1;
    return CF_OK;
}

int cf_pw_score_topk(cf_pw* e, const int32_t* users, int32_t n, int32_t k, int32_t exclude_train,
                     int32_t* idx_out, float* val_out) {
    if (!e) return cfi::set_error(CF_EINVAL, "bad arguments");
    if (e->kind != CF_PW_MF)
        return cfi::set_error(CF_EINVAL, "cf_pw_score_topk serves the MF kind (svd.py has no recommend)");
    CF_HIP(hipSetDevice(e->device));
    // wrmf.py:78-81, 98-111: U[test] V^T, top-k, train items dropped -- the rule of cf_score_topk
    const bool fused = k <= kFusedMaxWideK;
    return cfi::score_topk_chunks(
        e->stream, "cf_pw", e->n_users, e->n_items, e->indptr != nullptr, users, n, k, exclude_train, idx_out,
        val_out, !fused, [&](const int32_t* d_users, int m, uint32_t* keys, int32_t* d_idx, float* d_val) {
            if (fused) {   // all n users, straight to d_idx / d_val
                FusedTopkArgs f{};
                f.model = CF_BPR;
                f.d = e->d; f.Dp = (e->d + 7) & ~7; f.Dh = f.Dp / 2;
                f.n_users = m; f.n_items = e->n_items; f.k = k;
                f.users = d_users; f.U = e->U; f.V = e->V;
                f.exclude_train = exclude_train ? 1 : 0;
                f.indptr = e->indptr; f.indices = e->indices;
                f.idx_out = d_idx; f.val_out = d_val;
                return launch_fused_topk(f, e->stream);
            }
            ScoreArgs s{};
            s.model = CF_BPR;
            s.d = e->d; s.n_users = m; s.n_items = e->n_items;
            s.users = d_users; s.U = e->U; s.V = e->V;
            s.keys = keys;
            s.exclude_train = exclude_train ? 1 : 0;
            s.indptr = e->indptr; s.indices = e->indices;
            return launch_score(s, e->stream);
        });
}

}  // extern "C"
