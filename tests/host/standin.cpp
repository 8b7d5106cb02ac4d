// standin.cpp -- a stand-in for the HIP runtime: exactly the symbols the objects of minddet_amd/csrc/*.hip import, nothing else, so a
// program linked against it (and NOT against the real runtime) cannot open a device wherever it runs.  Allocation is host malloc,
// launches do nothing, and every call is written into a ledger (standin.h) that the replay program prints per case.
#include "standin.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <mutex>

namespace {
// one object built on first use: the objects' module constructors call __hipRegisterFunction before this file's statics would exist
struct State {
    std::mutex mu;
    std::string ledger;
    std::map<const void *, std::string> names;    // kernel host address -> device name (from __hipRegisterFunction)
    std::map<void *, size_t> live;                 // live allocations -> bytes
    long allocs = 0, frees = 0, fail_in = 0;
};
State &st() { static State *s = new State; return *s; }
#define g_mu st().mu
#define g_ledger st().ledger
#define g_names st().names
#define g_live st().live
#define g_allocs st().allocs
#define g_frees st().frees
#define g_fail_in st().fail_in
struct CallConfig { dim3_t grid, block; size_t lds; void *stream; };
thread_local CallConfig t_cfg;

void note(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void note(const char *fmt, ...) {
    char buf[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> l(g_mu);
    g_ledger += ' ';
    g_ledger += buf;
}
std::string kernel_name(const void *k) {
    std::lock_guard<std::mutex> l(g_mu);
    auto it = g_names.find(k);
    if (it != g_names.end()) return it->second;
    char buf[32];
    snprintf(buf, sizeof buf, "k%p", k);
    return buf;
}
int alloc(void **p, size_t bytes, void *stream) {
    {
        std::lock_guard<std::mutex> l(g_mu);
        if (g_fail_in > 0) {
            --g_fail_in;
            g_ledger += " malloc_failed";
            if (p) *p = nullptr;
            return 2;   // hipErrorOutOfMemory
        }
    }
    void *q = malloc(bytes ? bytes : 1);
    if (!q) return 2;
    {
        std::lock_guard<std::mutex> l(g_mu);
        g_live[q] = bytes;
        ++g_allocs;
    }
    *p = q;
    note("malloc:%zu:%p", bytes, stream);
    return 0;
}
int release(void *p, const char *what, void *stream) {
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> l(g_mu);
        auto it = g_live.find(p);
        if (it == g_live.end()) {
            g_ledger += " free_of_unknown_pointer";
            return 1;
        }
        bytes = it->second;
        g_live.erase(it);
        ++g_frees;
    }
    free(p);
    note("%s:%zu:%p", what, bytes, stream);
    return 0;
}
}  // namespace

std::string standin_take_ledger() {
    std::lock_guard<std::mutex> l(g_mu);
    std::string out;
    out.swap(g_ledger);
    return out;
}
void standin_fail_alloc(long n) {
    std::lock_guard<std::mutex> l(g_mu);
    g_fail_in = n;
}
void standin_balance(long *allocs, long *frees, long *live) {
    std::lock_guard<std::mutex> l(g_mu);
    *allocs = g_allocs; *frees = g_frees; *live = (long)g_live.size();
}

extern "C" {
int hipGetDevice(int *dev) { note("getdevice"); *dev = 0; return 0; }
int hipGetLastError() { note("lasterror"); return 0; }
int hipMallocAsync(void **p, size_t bytes, void *stream) { return alloc(p, bytes, stream); }
int hipFreeAsync(void *p, void *stream) { return release(p, "freeasync", stream); }
int hipFree(void *p) { return release(p, "free", nullptr); }
int hipMemsetAsync(void *, int value, size_t bytes, void *stream) { note("memset:%d:%zu:%p", value, bytes, stream); return 0; }
int hipFuncSetAttribute(const void *k, int attr, int value) { note("attr:%s:%d:%d", kernel_name(k).c_str(), attr, value); return 0; }
int hipLaunchKernel(const void *k, dim3_t grid, dim3_t block, void **, size_t lds, void *stream) {
    note("launch:%s:%u,%u,%u:%u,%u,%u:%zu:%p", kernel_name(k).c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, lds, stream);
    return 0;
}
unsigned __hipPushCallConfiguration(dim3_t grid, dim3_t block, size_t lds, void *stream) {
    t_cfg = {grid, block, lds, stream};
    return 0;
}
int __hipPopCallConfiguration(dim3_t *grid, dim3_t *block, size_t *lds, void **stream) {
    *grid = t_cfg.grid; *block = t_cfg.block; *lds = t_cfg.lds; *stream = t_cfg.stream;
    return 0;
}
void **__hipRegisterFatBinary(const void *) { static void *module; return &module; }
void __hipUnregisterFatBinary(void **) { }
void __hipRegisterFunction(void **, const void *host, char *, const char *name, unsigned, void *, void *, void *, void *, int *) {
    std::lock_guard<std::mutex> l(g_mu);
    g_names[host] = name;
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) { }
}
