// replay.cpp -- replays calls of the library's C ABI on the host, against the stand-in runtime (standin.cpp), so that host sanitizers
// see the argument checks, the size arithmetic, the scratch pool and the launch arithmetic of every entry point.  No device exists for
// this program: the stand-in is the only runtime it is linked with.
//
//   replay cases FILE [FIRST]   one line of FILE per command, from command number FIRST on; one "R <id> <rc> <ledger>" line each
//       CALL id sym stream n nullmask extra  then per operand:  offset|N  shape_is_null  rank  dtype|-  extent...
//            nullmask: 1 params, 2 ndims, 4 shapes, 8 dtypes passed as NULL; extra: the attribute struct's bytes in hex, or -
//            offset: the operand's data pointer as an offset into the arena (never dereferenced), N: a NULL pointer
//       WS id sym k v0 .. vk-1     int64_t sym(int64_t x k); the line's rc is the answer
//       FAILALLOC id n             the next n allocations fail
//       RELEASE id                 md_scratch_release()
//       BALANCE id                 rc = live allocations; the ledger holds the totals
//   replay lds                  md::ensure_dyn_lds on 130 fake kernels (more than its table holds)
//   replay threads              8 threads, 8 streams: md::pool_acquire with growth, md::ensure_dyn_lds on shared kernels
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>

#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "aot.h"      // minddet_amd/csrc, on the include path
#include "standin.h"

namespace {
constexpr size_t ARENA = (size_t)1 << 30;
typedef int (*aot_fn)(int, void **, int *, int64_t **, const char **, void *, void *);

void *resolve(const std::string &sym) {
    void *f = dlsym(RTLD_DEFAULT, sym.c_str());
    if (!f) {
        fprintf(stderr, "replay: no symbol %s\n", sym.c_str());
        exit(3);
    }
    return f;
}

long long run_call(std::istringstream &in, char *arena) {
    std::string sym, extra_hex;
    unsigned long long stream;
    int n, nullmask;
    in >> sym >> stream >> n >> nullmask >> extra_hex;
    std::vector<void *> params(n > 0 ? n : 0);
    std::vector<int> ndims(params.size());
    std::vector<std::vector<int64_t>> ext(params.size());
    std::vector<int64_t *> shapes(params.size());
    std::vector<std::string> names(params.size());
    std::vector<const char *> dtypes(params.size());
    for (size_t i = 0; i < params.size(); ++i) {
        std::string off;
        int shape_null, rank;
        in >> off >> shape_null >> rank >> names[i];
        params[i] = off == "N" ? nullptr : arena + strtoull(off.c_str(), nullptr, 10);
        ndims[i] = rank;
        ext[i].resize(rank > 0 ? rank : 0);
        for (auto &e : ext[i]) in >> e;
        shapes[i] = shape_null ? nullptr : ext[i].data();      // (rank 0: a one-past pointer of an empty vector, never read)
        dtypes[i] = names[i] == "-" ? nullptr : names[i].c_str();
    }
    if (in.fail()) {
        fprintf(stderr, "replay: malformed CALL line\n");
        exit(3);
    }
    // the attribute struct in a heap block of exactly its size: a read past it is a report
    std::vector<unsigned char> *extra = nullptr;
    if (extra_hex != "-") {
        extra = new std::vector<unsigned char>(extra_hex.size() / 2);
        for (size_t k = 0; k < extra->size(); ++k) (*extra)[k] = (unsigned char)strtoul(extra_hex.substr(2 * k, 2).c_str(), nullptr, 16);
    }
    aot_fn f = (aot_fn)resolve(sym);
    const int rc = f(n, nullmask & 1 ? nullptr : params.data(), nullmask & 2 ? nullptr : ndims.data(), nullmask & 4 ? nullptr : shapes.data(),
                     nullmask & 8 ? nullptr : dtypes.data(), (void *)(uintptr_t)stream, extra ? extra->data() : nullptr);
    delete extra;
    return rc;
}

long long run_ws(std::istringstream &in) {
    std::string sym;
    int k;
    int64_t v[6] = {0, 0, 0, 0, 0, 0};
    in >> sym >> k;
    for (int i = 0; i < k && i < 6; ++i) in >> v[i];
    if (in.fail() || k < 1 || k > 6) {
        fprintf(stderr, "replay: malformed WS line\n");
        exit(3);
    }
    void *f = resolve(sym);
    switch (k) {
    case 1: return ((int64_t(*)(int64_t))f)(v[0]);
    case 2: return ((int64_t(*)(int64_t, int64_t))f)(v[0], v[1]);
    case 3: return ((int64_t(*)(int64_t, int64_t, int64_t))f)(v[0], v[1], v[2]);
    case 4: return ((int64_t(*)(int64_t, int64_t, int64_t, int64_t))f)(v[0], v[1], v[2], v[3]);
    case 5: return ((int64_t(*)(int64_t, int64_t, int64_t, int64_t, int64_t))f)(v[0], v[1], v[2], v[3], v[4]);
    default: return ((int64_t(*)(int64_t, int64_t, int64_t, int64_t, int64_t, int64_t))f)(v[0], v[1], v[2], v[3], v[4], v[5]);
    }
}

int replay_cases(const char *path, long first) {
    char *arena = (char *)mmap(nullptr, ARENA, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (arena == MAP_FAILED) return 3;
    std::ifstream file(path);
    if (!file) return 3;
    std::string line;
    for (long no = 0; std::getline(file, line); ++no) {
        if (no < first || line.empty()) continue;
        std::istringstream in(line);
        std::string cmd, id;
        in >> cmd >> id;
        printf("B %ld %s\n", no, id.c_str());      // the command a sanitizer report that follows belongs to
        fflush(stdout);
        long long rc = 0;
        if (cmd == "CALL") rc = run_call(in, arena);
        else if (cmd == "WS") rc = run_ws(in);
        else if (cmd == "FAILALLOC") { long n; in >> n; standin_fail_alloc(n); }
        else if (cmd == "RELEASE") rc = ((int (*)())resolve("md_scratch_release"))();
        else if (cmd == "BALANCE") {
            long a, f, live;
            standin_balance(&a, &f, &live);
            rc = live;
            printf("R %s %lld allocs:%ld frees:%ld\n", id.c_str(), rc, a, f);
            continue;
        } else {
            fprintf(stderr, "replay: unknown command %s\n", cmd.c_str());
            return 3;
        }
        printf("R %s %lld%s\n", id.c_str(), rc, standin_take_ledger().c_str());
    }
    printf("END\n");
    return 0;
}

// fake kernel addresses: distinct, 8-byte spaced like functions never are, enough to collide in the table
const void *fake_kernel(int i) { return (const void *)(uintptr_t)(0x100000 + 64 * (uintptr_t)i); }

int drive_lds() {
    const int sizes[4] = {70000, 70000, 90000, 80000};      // set, cached, raised, cached (lower than the value held)
    for (int step = 0; step < 4; ++step)
        for (int i = 0; i < 130; ++i) {
            const int rc = md::ensure_dyn_lds(fake_kernel(i), sizes[step]);
            printf("L %d %d %d%s\n", step, i, rc, standin_take_ledger().c_str());
        }
    printf("END\n");
    return 0;
}

int drive_threads() {
    std::vector<std::thread> th;
    int bad = 0;
    for (int t = 0; t < 8; ++t)
        th.emplace_back([t, &bad] {
            hipStream_t s = (hipStream_t)(uintptr_t)(0x1000 * (t + 1));
            for (int it = 0; it < 200; ++it) {
                void *p = md::pool_acquire(((size_t)1 << 20) * (1 + it / 40) + it, s);
                if (!p) __atomic_fetch_add(&bad, 1, __ATOMIC_RELAXED);
                if (md::ensure_dyn_lds(fake_kernel(it % 4), 66000 + 100 * it + t) != MD_OK) __atomic_fetch_add(&bad, 1, __ATOMIC_RELAXED);
            }
        });
    for (auto &x : th) x.join();
    const int rc = md::pool_release();
    long a, f, live;
    standin_balance(&a, &f, &live);
    printf("T %d %d allocs:%ld frees:%ld live:%ld\nEND\n", bad, rc, a, f, live);
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cases" && argc > 2) return replay_cases(argv[2], argc > 3 ? atol(argv[3]) : 0);
    if (mode == "lds") return drive_lds();
    if (mode == "threads") return drive_threads();
    fprintf(stderr, "usage: replay cases FILE [FIRST] | lds | threads\n");
    return 2;
}
