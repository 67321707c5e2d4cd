// Host build of pyitd_amd/csrc/itd_memory.hpp for tests/test_memory_host.py: the owning buffer type over malloc-backed, counting
// stand-ins for the six runtime calls it uses, with a switch that makes the k-th allocation fail.  Built with g++ and the host
// sanitizers; never touches a GPU.  Test infrastructure: nothing in pyitd_amd/ uses this.
//
// usage: memory_host <case>; prints one event per line as the stand-ins are called ("malloc dev <id> <bytes>", "free dev <id>",
// "memset <id> <value> <bytes>", "sync"), what the case reports ("<name> <value>") and, last, "live <blocks still allocated>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };

namespace {
struct Block { int id; bool pinned; };
std::map<void *, Block> g_live;
int g_allocs = 0, g_fail_at = 0;   // allocations so far (of both kinds); the one that fails (0: none)

hipError_t stand_in_alloc(void **p, size_t bytes, bool pinned, unsigned flags)
{
    if (++g_allocs == g_fail_at) { printf("refuse %s %zu\n", pinned ? "pin" : "dev", bytes); return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    g_live[*p] = Block{g_allocs, pinned};
    if (pinned) printf("malloc pin %d %zu flags %u\n", g_allocs, bytes, flags);
    else printf("malloc dev %d %zu\n", g_allocs, bytes);
    return hipSuccess;
}
hipError_t stand_in_free(void *p, bool pinned)
{
    const auto it = g_live.find(p);
    if (it == g_live.end() || it->second.pinned != pinned) { printf("bad-free\n"); return 1; }
    printf("free %s %d\n", pinned ? "pin" : "dev", it->second.id);
    g_live.erase(it);
    free(p);
    return hipSuccess;
}
}  // namespace

hipError_t hipMalloc(void **p, size_t bytes) { return stand_in_alloc(p, bytes, false, 0); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) { return stand_in_alloc(p, bytes, true, flags); }
hipError_t hipFree(void *p) { return stand_in_free(p, false); }
hipError_t hipHostFree(void *p) { return stand_in_free(p, true); }
hipError_t hipMemset(void *p, int value, size_t bytes)
{
    printf("memset %d %d %zu\n", g_live.at(p).id, value, bytes);
    memset(p, value, bytes);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize() { printf("sync\n"); return hipSuccess; }

#include "../../pyitd_amd/csrc/itd_memory.hpp"

using itd::Buf;
using itd::Pinned;

static void report(const char *name, long long v) { printf("%s %lld\n", name, v); }

static void run(const char *what)
{
    if (!strcmp(what, "reserve")) {
        Buf<double> b;
        report("rc", b.reserve(100));
        double *first = b;
        report("rc", b.reserve(60));          // large enough: nothing happens
        report("same", first == b.get() && b.bytes() == 100);
        report("rc", b.reserve(200));         // frees, then allocates exactly what was asked for
        report("bytes", (long long)b.bytes());
    } else if (!strcmp(what, "reserve_fails")) {
        Buf<void> b;
        report("rc", b.reserve(100));
        g_fail_at = 2;
        hipError_t why = hipSuccess;
        report("rc", b.reserve(200, &why));
        report("why", why);
        report("empty", b.get() == nullptr && b.bytes() == 0 && !b);
        report("rc", b.reserve(50));          // and it can be used again
    } else if (!strcmp(what, "alloc_fails")) {
        g_fail_at = 1;
        Buf<int32_t> b;
        report("hip", b.alloc(64));
        report("empty", b.get() == nullptr && b.bytes() == 0);
    } else if (!strcmp(what, "release")) {
        Buf<int32_t> b;
        report("hip", b.alloc(64));
        b.release();
        report("empty", b.get() == nullptr && b.bytes() == 0);
        b.release();
        printf("scope-ends\n");
    } else if (!strcmp(what, "move")) {
        Buf<char> a, c;
        report("hip", a.alloc(10));
        report("hip", c.alloc(20));
        char *p = a;
        Buf<char> b(std::move(a));
        report("moved", b.get() == p && b.bytes() == 10 && a.get() == nullptr && a.bytes() == 0);
        c = std::move(b);                      // frees what c held
        report("moved", c.get() == p && c.bytes() == 10 && b.get() == nullptr && b.bytes() == 0);
        printf("scope-ends\n");
    } else if (!strcmp(what, "retire")) {
        std::vector<Buf<void>> retired;
        {
            Buf<void> ws;
            report("hip", ws.alloc(100));
            retired.push_back(std::move(ws));  // handed on: a captured graph may still hold its pointers
            report("hip", ws.alloc(200));
            retired.push_back(std::move(ws));
            report("hip", ws.alloc(400));
            printf("owner-ends\n");
        }
        printf("list-ends\n");
    } else if (!strcmp(what, "counted")) {
        int64_t total = 0;
        Buf<double> a, b;
        Pinned<double> h;
        report("hip", a.alloc(100, &total));
        report("hip", b.alloc(50));
        report("rc", b.reserve(70));
        report("hip", h.alloc(30));
        report("total", total);
        std::vector<Buf<double>> retired;
        retired.push_back(std::move(a));
        report("hip", a.alloc(300, &total));
        a.release();
        report("total", total);                // every block ever counted stays counted
    } else if (!strcmp(what, "pinned")) {
        Pinned<void> plain, mapped;
        report("hip", plain.alloc(16));
        report("hip", mapped.alloc(256, nullptr, 6));
        report("rc", plain.reserve(32));
    } else if (!strcmp(what, "poison")) {      // (the test sets PYITD_POISON)
        Buf<unsigned char> d;
        Pinned<unsigned char> h;
        report("hip", d.alloc(8));
        report("filled", d[0] == 0xFF && d[7] == 0xFF);
        report("hip", hipMemset(d, 0, 8));     // a zero fill of the caller's comes behind the poison
        report("hip", h.alloc(8));
        report("rc", d.reserve(16));
    } else {
        printf("unknown-case\n");
    }
}

int main(int argc, char **argv)
{
    run(argc > 1 ? argv[1] : "");
    report("live", (long long)g_live.size());
    return 0;
}
