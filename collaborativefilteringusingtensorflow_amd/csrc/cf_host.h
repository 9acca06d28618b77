// cf_host.h -- the host layer every native object shares (cf_engine.cpp and the
// ensemble, LRML and pointwise objects): the error text and status macros, the
// one owner of a device or pinned allocation, and the plumbing the objects have
// in common (device selection, CSR validation and upload, table copies, loss
// read-back, recommend staging).  Host only; no kernel lives here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cf_engine.h"
#include "cf_kernels.h"

namespace cfi {

int set_error(int code, const std::string& msg);   // cf_engine.cpp: the thread's cf_last_error text
inline int fail(int code, const std::string& msg) { return set_error(code, msg); }

#define CF_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return ::cfi::set_error(CF_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

#define CF_TRY(expr)            \
    do {                        \
        int _r = (expr);        \
        if (_r != CF_OK) return _r; \
    } while (0)

// bytes held by live buffers of every object in the process (cf_debug_live_bytes);
// defined in cf_engine.cpp
extern std::atomic<int64_t> g_live_bytes[2];   // [0] device, [1] pinned host

// The one owner of a device (Pinned: pinned host) allocation; p and cap are in
// elements.  It never synchronises: a caller that replaces a buffer a stream
// may still use synchronises first.  A failed allocation clears HIP's sticky
// error, so the next launch wrapper's hipGetLastError() does not report it.
template <class T, bool Pinned = false>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { release(); }
    void release() {
        if (p) (void)(Pinned ? hipHostFree((void*)p) : hipFree((void*)p));
        g_live_bytes[Pinned] -= (int64_t)(cap * sizeof(T));
        p = nullptr;
        cap = 0;
    }
    int reset(size_t n, const char* what) {   // always a fresh buffer of exactly n elements
        release();
        if (n == 0) return CF_OK;
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault)
                                    : hipMalloc((void**)&p, n * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return fail(CF_ENOMEM, std::string(Pinned ? "hipHostMalloc(" : "hipMalloc(") + what + ", " +
                                       std::to_string(n * sizeof(T)) + " B): " + hipGetErrorString(e));
        }
        cap = n;
        g_live_bytes[Pinned] += (int64_t)(n * sizeof(T));
        return CF_OK;
    }
    int reserve(size_t n, const char* what) { return cap >= n ? CF_OK : reset(n, what); }
    T* get() const { return p; }
    operator T*() const { return p; }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;

// ---------------------------------------------------------------------------
// What the ensemble, LRML and pointwise objects share
// ---------------------------------------------------------------------------

// the create preamble: a device must be visible, `device` must name one; selects it
inline int open_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(CF_EHIP, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(CF_EINVAL, "device ordinal out of range");
    CF_HIP(hipSetDevice(device));
    return CF_OK;
}

// cf_*_destroy of an object that owns `stream` on `device` and holds its memory in
// Buf members: the stream drains, the members release, the stream goes (cf_destroy's order)
template <class Obj>
int destroy_object(Obj* e) {
    if (!e) return CF_OK;
    (void)hipSetDevice(e->device);
    const hipStream_t stream = e->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete e;
    if (stream) (void)hipStreamDestroy(stream);
    return CF_OK;
}

// host CSR: indptr spans nnz and is monotone, every row sorted, unique and in range
inline int check_csr(const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_users,
                     int64_t n_items) {
    if (!indptr || (nnz > 0 && !indices)) return fail(CF_EINVAL, "null CSR");
    if (indptr[0] != 0 || indptr[n_users] != nnz) return fail(CF_EINVAL, "indptr does not span nnz");
    for (int64_t u = 0; u < n_users; ++u) {
        if (indptr[u + 1] < indptr[u]) return fail(CF_EINVAL, "indptr not monotone");
        for (int64_t k = indptr[u]; k < indptr[u + 1]; ++k)
            if (indices[k] < 0 || indices[k] >= n_items || (k > indptr[u] && indices[k - 1] >= indices[k]))
                return fail(CF_EINVAL, "CSR rows must hold sorted, unique, in-range items");
    }
    return CF_OK;
}

// a checked CSR replaces the one on the device (the stream may still read the old one)
inline int upload_csr(hipStream_t stream, DevBuf<int64_t>& d_indptr, DevBuf<int32_t>& d_indices,
                      const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_users) {
    CF_HIP(hipStreamSynchronize(stream));
    d_indptr.release();
    d_indices.release();
    CF_TRY(d_indptr.reset((size_t)n_users + 1, "indptr"));
    CF_TRY(d_indices.reset((size_t)(nnz > 0 ? nnz : 1), "indices"));
    CF_HIP(hipMemcpy(d_indptr, indptr, ((size_t)n_users + 1) * 8, hipMemcpyHostToDevice));
    if (nnz > 0) CF_HIP(hipMemcpy(d_indices, indices, (size_t)nnz * 4, hipMemcpyHostToDevice));
    return CF_OK;
}

// a step's buffer grows: the stream may still use the one it replaces
template <class T>
int grow(hipStream_t stream, DevBuf<T>& b, size_t n, const char* what) {
    if (b.cap >= n) return CF_OK;
    CF_HIP(hipStreamSynchronize(stream));
    return b.reset(n, what);
}

// cf_*_set_table / cf_*_get_table: p holds `want` floats (null: no such table), the caller n
inline int check_table(const float* p, int64_t want, const void* host, int64_t n, const char* what) {
    if (!host) return fail(CF_EINVAL, "null argument");
    if (!p || n != want)
        return fail(CF_EINVAL, std::string(what) + " table size mismatch: want " + std::to_string(want));
    return CF_OK;
}
inline int copy_table_in(hipStream_t stream, float* p, int64_t want, const float* host, int64_t n,
                         const char* what) {
    CF_TRY(check_table(p, want, host, n, what));
    CF_HIP(hipStreamSynchronize(stream));
    CF_HIP(hipMemcpy(p, host, (size_t)n * 4, hipMemcpyHostToDevice));
    return CF_OK;
}
inline int copy_table_out(hipStream_t stream, const float* p, int64_t want, float* host, int64_t n,
                          const char* what) {
    CF_TRY(check_table(p, want, host, n, what));
    CF_HIP(hipStreamSynchronize(stream));
    CF_HIP(hipMemcpy(host, p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return CF_OK;
}

// cf_*_take_loss: the running device sum, read and zeroed
inline int take_loss(hipStream_t stream, double* loss_acc, double* out) {
    CF_HIP(hipMemcpyAsync(out, loss_acc, 8, hipMemcpyDeviceToHost, stream));
    CF_HIP(hipMemsetAsync(loss_acc, 0, 8, stream));
    CF_HIP(hipStreamSynchronize(stream));
    return CF_OK;
}

// a step's loss: its n block partials, summed in block order
inline int read_loss(hipStream_t stream, const double* loss_partial, int n, std::vector<double>& h_loss,
                     double* out) {
    h_loss.resize((size_t)n);
    CF_HIP(hipMemcpyAsync(h_loss.data(), loss_partial, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    CF_HIP(hipStreamSynchronize(stream));
    double t = 0.0;
    for (int q = 0; q < n; ++q) t += h_loss[(size_t)q];
    *out = t;
    return CF_OK;
}

// The recommend staging of cf_*_score_topk (`who` is the object's prefix, "cf_ens").
// Checks the arguments, uploads the users and hands them to
//     hipError_t score(const int32_t* d_users, int m, uint32_t* keys, int32_t* d_idx, float* d_val)
// in chunks of at most 65,535 users (grid.y) and 256 MiB of keys; `score` fills
// keys [m, n_items] and launch_topk selects from them.  keyed == false: `score`
// writes d_idx / d_val itself, for all n users at once, and no keys are held.
template <class Score>
int score_topk_chunks(hipStream_t stream, const char* who, int64_t n_users, int64_t n_items, bool have_csr,
                      const int32_t* users, int32_t n, int32_t k, int32_t exclude_train, int32_t* idx_out,
                      float* val_out, bool keyed, Score score) {
    if (n < 0 || !idx_out || (n > 0 && !users)) return fail(CF_EINVAL, "bad arguments");
    if (k < 1 || k > 4096) return fail(CF_EINVAL, "k must be 1..4096");
    if (exclude_train && !have_csr)
        return fail(CF_ESTATE, std::string("exclude_train needs ") + who + "_set_interactions");
    if (n == 0) return CF_OK;
    for (int r = 0; r < n; ++r)
        if (users[r] < 0 || users[r] >= n_users) return fail(CF_EINVAL, "user id out of range");
    const size_t row_bytes = (size_t)n_items * 4;
    const int chunk = !keyed ? n : (int)std::max<size_t>(
        1, std::min<size_t>(std::min<size_t>((size_t)n, 65535), ((size_t)256 << 20) / row_bytes));
    DevBuf<uint32_t> keys;
    DevBuf<int32_t> d_users, d_idx;
    DevBuf<float> d_val;
    CF_TRY(keys.reset(keyed ? (size_t)chunk * n_items : 0, "recommend keys"));
    CF_TRY(d_users.reset((size_t)n, "recommend users"));
    CF_TRY(d_idx.reset((size_t)n * k, "recommend idx"));
    CF_TRY(d_val.reset((size_t)n * k, "recommend val"));
    hipError_t he = hipMemcpyAsync(d_users, users, (size_t)n * 4, hipMemcpyHostToDevice, stream);
    for (int u0 = 0; he == hipSuccess && u0 < n; u0 += chunk) {
        const int m = std::min(chunk, n - u0);
        he = score(d_users + u0, m, keys.get(), d_idx + (size_t)u0 * k, d_val + (size_t)u0 * k);
        if (he != hipSuccess || !keyed) break;
        cfk::TopkArgs t{};
        t.k = k;
        t.n_items = n_items;
        t.keys = keys;
        t.idx_out = d_idx + (size_t)u0 * k;
        t.val_out = d_val + (size_t)u0 * k;
        he = cfk::launch_topk(t, m, stream);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he == hipSuccess) he = hipMemcpy(idx_out, d_idx, (size_t)n * k * 4, hipMemcpyDeviceToHost);
    if (he == hipSuccess && val_out) he = hipMemcpy(val_out, d_val, (size_t)n * k * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(CF_EHIP, std::string(who) + "_score_topk: " + hipGetErrorString(he));
    return CF_OK;
}

}  // namespace cfi
