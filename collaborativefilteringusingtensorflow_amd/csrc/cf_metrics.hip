// cf_metrics.hip -- the reference's ranking metrics on the device lists
// (src/metrics/ranking.py:11-120 with the truth of bprmf.py:117-123): hit
// labels by binary search in the user's sorted truth row, the per-user values
// walked in position order in fp64, and a fixed-order fp64 reduction to one
// row of sums per cutoff.  gfx950; no library sort or scan, no float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cf_kernels.h"
#include "cf_device.h"

// the walk is a chain of fp64 adds and divides whose order ranking.py fixes
#pragma clang fp contract(off)

namespace cfk {

// one user's running values while its list is walked in position order; the
// operation order is ranking.py's
struct MetricWalk {
    int hits = 0;
    double dcg = 0.0;     // hit discounts, ascending position (ranking.py:29-30, 53-54)
    double ideal = 0.0;   // disc[0 .. hits-1], ascending (the labels sorted descending)
    double ap = 0.0;      // ranking.py:62-66
    double mrr = 0.0;     // ranking.py:75-78
    double hr = 0.0;      // ranking.py:86
    double arhr = 0.0;    // ranking.py:94-96
};

// cutoffs[i] for a lane-varying i without indexing the kernel arguments
__device__ __forceinline__ int cutoff_at(const MetricsArgs& a, int i) {
    int v = a.cutoffs[0];
#pragma unroll
    for (int q = 1; q < kEvalMaxCut; ++q) v = i == q ? a.cutoffs[q] : v;
    return v;
}

__device__ __forceinline__ void metric_emit(const MetricWalk& w, int cutoff, int tlen, double* __restrict__ out) {
    const double h = (double)w.hits;
    out[0] = h / (double)cutoff;                         // pre
    out[1] = h / (tlen > 1 ? (double)tlen : 1.0);        // recall
    out[2] = w.dcg / (w.ideal > 1.0 ? w.ideal : 1.0);    // ndcg
    out[3] = w.ap / (double)tlen;                        // map (tlen >= 1: the engine rejects empty rows)
    out[4] = w.mrr;
    out[5] = w.hr;
    out[6] = w.arhr;
}

// G lanes per user (a power of two, 1..64), 64 / G users per wave.  Lane l of
// a group takes list positions l, l + G, ..: consecutive lanes read
// consecutive ids, and with G >= k the users of a wave read one contiguous
// piece of idx.  Each lane searches its id in the truth row (the loop's trip
// count differs between lanes; nothing crosses lanes inside it), the wave's
// hit bits are gathered with one ballot per chunk of G positions, and the
// group's first lane walks its G bits in position order.  Every lane of the
// wave runs the same number of chunks (kk is uniform), so the ballots see the
// whole wave; a group past the last user carries no hits and stores nothing.
template <int G>
__global__ __launch_bounds__(kBlock) void metrics_user_kernel(MetricsArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int l = lane & (G - 1);
    const int gshift = lane & ~(G - 1);   // first lane of this group inside the wave
    const int64_t r = (int64_t)blockIdx.x * (kBlock / G) + (threadIdx.x / G);
    bool valid = r < a.n;
    int32_t u = 0;
    if (valid) {
        u = a.users[r];
        valid = u >= 0 && (int64_t)u < a.n_users;   // checked by the engine; never index past the CSR
    }
    int64_t t0 = 0, t1 = 0;
    if (valid) {
        t0 = a.t_indptr[u];
        t1 = a.t_indptr[u + 1];
    }
    const int tlen = (int)(t1 - t0);
    const int32_t first = tlen > 0 ? a.t_indices[t0] : -1;   // T[0]: the LOOV truth (bprmf.py:121-123)
    const int32_t* __restrict__ row = a.idx + r * (int64_t)a.k;
    const int kk = a.cutoffs[a.n_cut - 1];   // positions past the last cutoff are never read
    constexpr unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);

    MetricWalk w;
    int ci = 0;
    double* __restrict__ out = a.per_user + r * (int64_t)a.n_cut * kEvalN;
    for (int base = 0; base < kk; base += G) {
        const int p = base + l;
        int32_t item = -1;
        if (valid && p < kk) item = row[p];
        bool hit = false;
        if (item >= 0 && tlen > 0) hit = sorted_contains(a.t_indices, t0, t1, item);   // a pad (-1) never hits
        const bool is_first = hit && item == first;
        const unsigned long long hb = (__ballot(hit) >> gshift) & gmask;
        const unsigned long long fb = (__ballot(is_first) >> gshift) & gmask;
        if (l == 0 && valid) {
            unsigned long long m = hb;   // fb is a subset: T[0] is in T
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const int pos = base + j;
                for (int c = cutoff_at(a, ci); ci < a.n_cut && c <= pos; c = cutoff_at(a, ci)) {
                    metric_emit(w, c, tlen, out + ci * kEvalN);   // the cutoffs this hit lies outside of
                    ++ci;
                }
                w.hits += 1;
                w.dcg += a.disc[pos];
                w.ideal += a.disc[w.hits - 1];
                w.ap += (double)w.hits / ((double)pos + 1.0);
                if (w.hits == 1) w.mrr = 1.0 / ((double)pos + 1.0);
                if (((fb >> j) & 1ull) && w.hr == 0.0) {
                    w.hr = 1.0;
                    w.arhr = 1.0 / (double)(pos + 1);
                }
            }
        }
    }
    if (l == 0 && valid)
        for (; ci < a.n_cut; ++ci) metric_emit(w, cutoff_at(a, ci), tlen, out + ci * kEvalN);
}

// Block b sums the rows [b * kMetricsRows, ..) of per_user [n, cols]: thread
// (wave w, column c) adds rows w, w + 4, .. in index order (a wave reads one
// row's columns side by side), then wave 0 adds the four in wave order.
constexpr int kMetricsRows = 1024;
__global__ __launch_bounds__(kBlock) void metrics_partial_kernel(const double* __restrict__ per_user, int64_t n,
                                                                 int cols, double* __restrict__ partial) {
    __shared__ double s_part[kWavesPerBlock][kWave];
    const int c = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int64_t r0 = (int64_t)blockIdx.x * kMetricsRows;
    const int64_t r1 = r0 + kMetricsRows < n ? r0 + kMetricsRows : n;
    double s = 0.0;
    if (c < cols)
        for (int64_t r = r0 + w; r < r1; r += kWavesPerBlock) s += per_user[r * cols + c];
    s_part[w][c] = s;
    __syncthreads();
    if (w == 0 && c < cols) {
        double t = s_part[0][c];
        for (int q = 1; q < kWavesPerBlock; ++q) t += s_part[q][c];
        partial[(int64_t)blockIdx.x * cols + c] = t;
    }
}

// one block: thread c folds column c of the block partials in block order
__global__ __launch_bounds__(kWave) void metrics_fold_kernel(const double* __restrict__ partial, int n_partial,
                                                             int cols, double* __restrict__ sums) {
    const int c = threadIdx.x;
    if (c >= cols) return;
    double t = 0.0;
    for (int b = 0; b < n_partial; ++b) t += partial[(int64_t)b * cols + c];
    sums[c] = t;
}

int metrics_partials(int64_t n) { return (int)((n + kMetricsRows - 1) / kMetricsRows); }

template <int G>
static void launch_user(const MetricsArgs& a, hipStream_t s) {
    const int64_t per_block = kBlock / G;
    hipLaunchKernelGGL(metrics_user_kernel<G>, dim3((unsigned)((a.n + per_block - 1) / per_block)), dim3(kBlock), 0,
                       s, a);
}

hipError_t launch_metrics(const MetricsArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int kk = a.cutoffs[a.n_cut - 1];
    if (kk <= 1) launch_user<1>(a, s);
    else if (kk <= 2) launch_user<2>(a, s);
    else if (kk <= 4) launch_user<4>(a, s);
    else if (kk <= 8) launch_user<8>(a, s);
    else if (kk <= 16) launch_user<16>(a, s);
    else if (kk <= 32) launch_user<32>(a, s);
    else launch_user<64>(a, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int cols = a.n_cut * kEvalN;
    const int nb = metrics_partials(a.n);
    hipLaunchKernelGGL(metrics_partial_kernel, dim3(nb), dim3(kBlock), 0, s, a.per_user, a.n, cols, a.partial);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(metrics_fold_kernel, dim3(1), dim3(kWave), 0, s, a.partial, nb, cols, a.sums);
    return hipGetLastError();
}

}  // namespace cfk
