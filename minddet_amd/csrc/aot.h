// aot.h -- host-side helpers shared by every entry point of libminddet_hip.so (the kernels' shared device code: device.h).
// Argument checking for the MindSpore AOT-operator ABI (see include/minddet_hip.h) and
// stream-ordered scratch.  Mutable globals: the LDS-attribute cache and the per-stream scratch pool below, nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <initializer_list>

#include "../../include/minddet_hip.h"

#define MD_HIP_TRY(expr)                       \
    do {                                       \
        hipError_t e__ = (expr);               \
        if (e__ != hipSuccess) return MD_ERR_HIP; \
    } while (0)

namespace md {

// The one checked product of the size tests: the product of the factors, INT64_MAX when it does not fit int64_t -- a value that fails
// every limit test (include/minddet_hip.h "Conventions": an extent product that does not fit counts as over every size limit).  The
// entry points test products of caller extents through this, never through a raw `*`, which would be undefined where it wraps.
static inline int64_t mul(std::initializer_list<int64_t> factors) {
    int64_t n = 1;
    for (int64_t f : factors)
        if (__builtin_mul_overflow(n, f, &n)) return INT64_MAX;
    return n;
}
// a + b for non-negative terms, INT64_MAX when it does not fit (and INT64_MAX stays INT64_MAX)
static inline int64_t add(int64_t a, int64_t b) {
    int64_t n;
    return __builtin_add_overflow(a, b, &n) ? INT64_MAX : n;
}
// Sz: a non-negative count for the scratch layouts (below: "Scratch sizes have one owner").  It is 128 bits wide and sticks at INF
// (2^126) through every operator, so a layout function written in plain arithmetic on Sz extents cannot wrap, and an element count
// above int64_t that a later division brings back (4 ceil(B C H W / chunk)) still gives the exact byte count.  The conversions out are
// explicit; the one to int64_t answers INT64_MAX for a count that does not fit -- the value that fails every limit test, and that
// ws_answer() below turns into the -1 of md_<op>_workspace_bytes.  A layout function computes in Sz locals and converts each part once,
// where it fills its struct.
struct Sz {
    __int128 v;
    static constexpr __int128 INF = (__int128)1 << 126;
    Sz(int64_t x = 0) : v(x < 0 ? INF : (__int128)x) { }
    static Sz wide(__int128 x) { Sz s; s.v = x < 0 || x >= INF ? INF : x; return s; }
    bool fits() const { return v <= (__int128)INT64_MAX; }
    explicit operator int64_t() const { return fits() ? (int64_t)v : INT64_MAX; }
    explicit operator bool() const { return v != 0; }
    friend Sz operator*(Sz a, Sz b) {
        __int128 r;
        return a.v == INF || b.v == INF || __builtin_mul_overflow(a.v, b.v, &r) ? wide(INF) : wide(r);
    }
    friend Sz operator+(Sz a, Sz b) { return wide(a.v + b.v); }                                  // (both <= 2^126: no wrap)
    friend Sz operator-(Sz a, Sz b) { return a.v == INF || b.v == INF ? wide(INF) : wide(a.v - b.v); }
    friend Sz operator/(Sz a, Sz b) { return a.v == INF || b.v == INF || b.v == 0 ? wide(INF) : wide(a.v / b.v); }
    friend bool operator<(Sz a, Sz b) { return a.v < b.v; }
    friend bool operator>(Sz a, Sz b) { return a.v > b.v; }
    friend bool operator<=(Sz a, Sz b) { return a.v <= b.v; }
    friend bool operator>=(Sz a, Sz b) { return a.v >= b.v; }
    friend bool operator==(Sz a, Sz b) { return a.v == b.v; }
};

// Args: the one argument-check layer of every AOT entry point (the rule is stated once, in include/minddet_hip.h "Conventions").
// A view over (nparam, params, ndims, shapes, dtypes) that is built, filled with the op's operands and asked for rc() BEFORE the
// entry point makes any device or runtime call.  The first failure latches its code; every accessor is safe whatever the caller passed:
// d() / numel() answer -1 for an operand that tensor() / optional() did not accept, and never index past ndims[i].
constexpr int ANY = -1;   // tensor(i, dtype, ANY): any rank
constexpr const char *F32 = "float32", *BF16 = "bfloat16", *I32 = "int32", *I64 = "int64", *U8 = "uint8";
struct Args {
    int nparam; void **params; int *ndims; int64_t **shapes; const char **dtypes;
    int err = MD_OK;
    unsigned ok = 0;      // bit i: operand i is described (ndims[i], shapes[i]) and was accepted
    bool oversize = false;   // an accepted operand other than a workspace has an extent above INT32_MAX (the kernels index with int)
                             // or an element count that does not fit int64_t

    // nparam in [lo, hi] (hi - lo trailing operands, e.g. the workspace, may be left out) and a params array
    Args(int np, void **p, int *nd, int64_t **sh, const char **dt, int lo, int hi) : nparam(np), params(p), ndims(nd), shapes(sh), dtypes(dt) {
        if (np < lo || np > hi) err = MD_ERR_NPARAM;
        else if (!p) err = MD_ERR_ARG;
    }
    // the descriptor checks come first (1, 2); an extent no op can take is the first of the size limits (4)
    int rc() const { return err ? err : oversize ? MD_ERR_SIZE : MD_OK; }
    bool require(bool cond, int code = MD_ERR_ARG) {
        if (!cond && !err) err = code;
        return cond;
    }
    // the op's attribute struct; an op that requires it reads this pointer only after rc() == 0
    template <typename T> const T *attrs(const void *extra) { require(extra != nullptr); return (const T *)extra; }
    // required operand i: described, of rank in [rank, rank_hi] (ANY = not looked at), of dtype `dt` where the caller names one
    // (dtypes == NULL or dtypes[i] == NULL passes, dt == nullptr = not looked at)
    // No extent may be negative (2).  capped: no extent may exceed INT32_MAX either (rc() then answers 4 once the descriptors pass).
    bool tensor(int i, const char *dt, int rank = ANY, int rank_hi = ANY, bool capped = true) {
        if (err) return false;
        if (i < 0 || i >= nparam || i >= 32 || !ndims || !shapes || !shapes[i] || ndims[i] < 0) return require(false);
        if (rank != ANY && (ndims[i] < rank || ndims[i] > (rank_hi == ANY ? rank : rank_hi))) return require(false);
        if (dt && dtypes && dtypes[i] && strcmp(dtypes[i], dt) != 0) return require(false);
        for (int k = 0; k < ndims[i]; ++k) {
            if (shapes[i][k] < 0) return require(false);
            if (capped && shapes[i][k] > INT32_MAX) oversize = true;
        }
        if (capped && prod(i) == INT64_MAX) oversize = true;    // an element count that does not fit int64_t
        ok |= 1u << i;
        return true;
    }
    // operand of the five reference-ABI ops whose shape the caller may leave out (shapes[i] == NULL: numel(i) is then -1)
    bool loose(int i, const char *dt) {
        const bool described = i >= 0 && i < nparam && ndims && shapes && shapes[i];
        if (described) return tensor(i, dt);
        return require(i >= 0 && i < nparam && !(dt && dtypes && dtypes[i] && strcmp(dtypes[i], dt) != 0));
    }
    // operand whose pointer may be NULL (or that lies past nparam): then nothing else is looked at
    bool optional(int i, const char *dt, int rank = ANY, int rank_hi = ANY) { return !given(i) || tensor(i, dt, rank, rank_hi); }
    // the optional trailing workspace: bytes of any rank, and no cap on an extent (a workspace larger than the op takes is legal)
    bool scratch(int i) { return !given(i) || tensor(i, U8, ANY, ANY, false); }
    bool given(int i) const { return !err && i >= 0 && i < nparam && params[i] != nullptr; }
    int rank(int i) const { return i >= 0 && i < 32 && (ok >> i & 1) ? ndims[i] : -1; }
    // extent k of operand i; k < 0 counts from the last
    int64_t d(int i, int k) const {
        const int nd = rank(i);
        if (k < 0) k += nd;
        return k >= 0 && k < nd ? shapes[i][k] : -1;
    }
    int64_t numel(int i) const { return rank(i) < 0 ? -1 : prod(i); }
    // bytes of the caller's workspace operand, -1 when it is absent (the scratch pool then serves) or not described
    int64_t workspace(int i) const { return i < nparam && params[i] && ndims && shapes && shapes[i] ? prod(i) : -1; }
    // element count, INT64_MAX when it does not fit int64_t (as md::mul): never wrapped, so never small by accident
    int64_t prod(int i) const {
        int64_t n = 1;
        for (int k = 0; k < ndims[i]; ++k)
            if (__builtin_mul_overflow(n, shapes[i][k], &n)) return INT64_MAX;
        return n;
    }
    // operands i, j agree in rank and every extent
    bool same_shape(int i, int j) const {
        bool same = rank(i) >= 0 && rank(i) == rank(j);
        for (int k = 0; same && k < rank(i); ++k) same = shapes[i][k] == shapes[j][k];
        return same;
    }
    template <typename T> T *ptr(int i) const { return i >= 0 && i < nparam && !err ? (T *)params[i] : nullptr; }
    // the data pointers an op with non-zero work dereferences: non-NULL, except for an operand described as empty
    bool have(std::initializer_list<int> idx) {
        for (int i : idx)
            if (!given(i) && numel(i) != 0) return require(false);
        return !err;
    }
};
#define MD_ARGS nparam, params, ndims, shapes, dtypes

static inline bool fits_i32(long long x) { return x <= 0x7fffffffLL; }
// byte ranges [a, a + an) and [b, b + bn) share a byte (an, bn >= 0, INT64_MAX from md::mul included: unsigned, so nothing wraps into UB)
static inline bool ranges_overlap(const void *a, int64_t an, const void *b, int64_t bn) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)bn && pb < pa + (uintptr_t)an;
}
// an output that shares its address with an input or with another output (operands [0, n_in) are inputs, [n_in, n_all) outputs)
static inline bool aliased(void **params, int n_in, int n_all) {
    for (int o = n_in; o < n_all; ++o) {
        if (!params[o]) continue;
        for (int k = 0; k < o; ++k)
            if (params[k] == params[o]) return true;
    }
    return false;
}
// the one launch epilogue: the launches of the call were accepted by the runtime
static inline int launched() { return hipGetLastError() == hipSuccess ? MD_OK : MD_ERR_HIP; }
// grid of a 1-D grid-stride kernel over `total` elements, 256 per workgroup, at most `cap` workgroups
static inline unsigned grid1d(size_t total, size_t cap = 16384) {
    const size_t b = (total + 255) / 256;
    return (unsigned)(b > cap ? cap : (b == 0 ? 1 : b));
}

// pool buffers grow in 1 MiB steps, doubling: few regrowths even when the first calls are small
static inline size_t align_up_pow2_chunk(size_t b) {
    size_t w = (size_t)1 << 20;
    while (w < b) w <<= 1;
    return w;
}

// Scratch: a caller-provided workspace (params[ws_index], size from shapes) or, when the caller passes none, a buffer of the library's
// per-(device, stream) pool.  r03: the fallback used to be hipMallocAsync + hipFreeAsync per call, which blocks the host behind queued
// work (measured ~7 ms per call) -- a MindSpore-side caller binding the ops as INTEGRATION 1 shows would have paid it on
// every NMS / top-k call.  The pool keeps ONE buffer per stream, grown on demand (hipMallocAsync / hipFreeAsync on that stream, so a
// queued kernel never loses its memory) and reused by every later call on the stream: steady state makes no driver call at all.  Reuse
// is safe because an op's kernels and the next op's kernels on one stream execute in order.  md_scratch_release() frees the pool.
// Not for use under stream capture: a pool buffer that GROWS inside a captured region would be allocated by the graph -- a captured
// caller passes the workspace param (as the Python host always does).
struct ScratchPoolEntry { int dev; hipStream_t stream; void *ptr; size_t bytes; };
struct ScratchPool {
    ScratchPoolEntry e[64];
    int n = 0;
    int lock = 0;
};
inline ScratchPool g_scratch_pool;
static inline void *pool_acquire(size_t bytes, hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    ScratchPool &P = g_scratch_pool;
    while (__atomic_exchange_n(&P.lock, 1, __ATOMIC_ACQUIRE)) { }
    void *out = nullptr;
    int slot = -1;
    for (int i = 0; i < P.n; ++i)
        if (P.e[i].dev == dev && P.e[i].stream == s) { slot = i; break; }
    if (slot < 0 && P.n < 64) {
        slot = P.n++;
        P.e[slot] = {dev, s, nullptr, 0};
    }
    if (slot >= 0) {
        ScratchPoolEntry &en = P.e[slot];
        if (en.bytes < bytes) {
            const size_t want = align_up_pow2_chunk(bytes);
            void *np = nullptr;
            if (hipMallocAsync(&np, want, s) == hipSuccess) {
                if (en.ptr) (void)hipFreeAsync(en.ptr, s);   // behind every kernel already queued on s that uses it
                en.ptr = np;
                en.bytes = want;
            }
        }
        if (en.bytes >= bytes) out = en.ptr;
    }
    __atomic_store_n(&P.lock, 0, __ATOMIC_RELEASE);
    return out;
}
static inline int pool_release() {
    ScratchPool &P = g_scratch_pool;
    while (__atomic_exchange_n(&P.lock, 1, __ATOMIC_ACQUIRE)) { }
    int rc = MD_OK;
    // hipFree, not hipFreeAsync: a stream the pool remembers may have been destroyed by its owner since (its handle would be invalid);
    // hipFree waits for the device, which is what a caller releasing memory before unloading the library wants anyway
    for (int i = 0; i < P.n; ++i)
        if (P.e[i].ptr && hipFree(P.e[i].ptr) != hipSuccess) rc = MD_ERR_HIP;
    P.n = 0;
    __atomic_store_n(&P.lock, 0, __ATOMIC_RELEASE);
    return rc;
}
struct Scratch {
    void *ptr = nullptr;
    bool owned = false;     // true: more than 64 (device, stream) pairs are live -- a one-call stream-ordered allocation
    hipStream_t stream = nullptr;
    int acquire(size_t bytes, const Args &a, int ws_index, hipStream_t s) {
        stream = s;
        if (bytes == 0) bytes = 16;
        if (ws_index < a.nparam && a.params[ws_index]) {
            int64_t have = a.workspace(ws_index);
            if (have >= 0 && (size_t)have < bytes) return MD_ERR_SIZE;
            ptr = a.params[ws_index];
            owned = false;
            return MD_OK;
        }
        ptr = pool_acquire(bytes, s);
        if (ptr) return MD_OK;
        if (hipMallocAsync(&ptr, bytes, s) != hipSuccess) return MD_ERR_HIP;
        owned = true;
        return MD_OK;
    }
    ~Scratch() {
        if (owned && ptr) (void)hipFreeAsync(ptr, stream);
    }
};

// acquire, then the alignment the op's carve of the buffer needs: MD_ERR_ARG for a caller's workspace that does not have it (a pool
// buffer always does)
static inline int acquire_aligned(Scratch &ws, size_t bytes, const Args &a, int ws_index, hipStream_t s, size_t align) {
    if (int rc = ws.acquire(bytes, a, ws_index, s)) return rc;
    return (uintptr_t)ws.ptr % align != 0 ? MD_ERR_ARG : MD_OK;
}

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline Sz align_up(Sz x, int64_t a) { return (x + (a - 1)) / a * a; }

// Scratch sizes have one owner (include/minddet_hip.h "Conventions"): per op one host function of the extents fills the byte offsets of
// the workspace's parts and their total; the exported md_<op>_workspace_bytes returns that total (-1 for a negative extent, below) and
// the entry point acquires and carves with the same values.
// what md_<op>_workspace_bytes answers for a checked total: -1 for a byte count that does not fit int64_t
static inline int64_t ws_answer(int64_t total) { return total == INT64_MAX || total < 0 ? -1 : total; }
static inline bool any_negative(std::initializer_list<int64_t> extents) {
    for (int64_t v : extents)
        if (v < 0) return true;
    return false;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device) instead of once per launch: it is a driver call on the
// launch path of every layer otherwise (r02 ADVICE; the YOLOv5s step is launch-bound) and would also run inside graph capture.
// Cache keyed by the kernel's host address (lock-free insert; a full table or a device id >= 8 just sets the attribute again).  The
// set-and-store of one slot is serialised by the slot's lock, so the cached value is always the value the driver holds (r03 ADVICE: two
// host threads raising one kernel's size concurrently could otherwise leave the cache above the driver's value).  This cache is the
// library's only mutable global besides the per-stream scratch pool below; `inline` gives the whole library ONE instance.
struct LdsAttrSlot { const void *k; int set[8]; int lock; };
inline LdsAttrSlot g_lds_attr[128];
static inline int ensure_dyn_lds(const void *k, int lds) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return MD_ERR_HIP;
    const unsigned h0 = (unsigned)(((uintptr_t)k >> 3) * 2654435761u >> 16);
    for (unsigned p = 0; p < 128 && dev >= 0 && dev < 8; ++p) {
        LdsAttrSlot &sl = g_lds_attr[(h0 + p) & 127];
        const void *cur = __atomic_load_n(&sl.k, __ATOMIC_ACQUIRE);
        if (cur == nullptr) {
            const void *expected = nullptr;
            cur = __atomic_compare_exchange_n(&sl.k, &expected, k, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE) ? k : expected;
        }
        if (cur != k) continue;
        if (__atomic_load_n(&sl.set[dev], __ATOMIC_ACQUIRE) >= lds) return MD_OK;
        while (__atomic_exchange_n(&sl.lock, 1, __ATOMIC_ACQUIRE)) { }
        int rc = MD_OK;
        if (sl.set[dev] < lds) {
            if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) rc = MD_ERR_HIP;
            else __atomic_store_n(&sl.set[dev], lds, __ATOMIC_RELEASE);
        }
        __atomic_store_n(&sl.lock, 0, __ATOMIC_RELEASE);
        return rc;
    }
    return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess ? MD_OK : MD_ERR_HIP;
}

// records which conv-family kernel the calling host thread launched last (md_conv2d_last_kernel); defined in conv.hip
void md_note_conv_kernel(int id);
// activation bytes above which a conv-family op slices the batch: md_conv_tune.chunk_limit of the call (tests lower it), default 2 GiB - 64 KiB
static inline long long md_chunk_limit(const md_conv_tune *t) {
    return t && t->chunk_limit > 0 && t->chunk_limit < 0x7fff0000 ? (long long)t->chunk_limit : 0x7fff0000LL;
}

}  // namespace md
