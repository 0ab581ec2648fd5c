// CPU test of webdgs_amd/csrc/devmem.h against a counting wdgs_alloc / wdgs_free that can be told to fail its k-th request: every block is freed
// exactly once, a re-allocation frees before it asks, a failed allocation leaves the handle EMPTY (no pointer, no count), release / adopt move a
// block without freeing it.  Built and run by tests/test_devmem.py (g++; no GPU, no HIP).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

typedef struct ihipStream_t* hipStream_t;   // all the header needs of HIP: the type of the stream it passes through
#include "../../webdgs_amd/csrc/devmem.h"

namespace {
struct Mock {
    int requests = 0;            // calls of wdgs_alloc, failed ones included
    int fail_at = 0;             // the request with this number (1-based) fails; 0: none
    std::map<void*, int> frees;  // block -> times freed
    std::map<void*, size_t> bytes;
    std::vector<std::string> log;   // "alloc <bytes>" / "free"
    int live() const {
        int n = 0;
        for (const auto& kv : frees) n += kv.second == 0;
        return n;
    }
    bool each_freed_once() const {
        for (const auto& kv : frees) if (kv.second != 1) return false;
        return true;
    }
} g;
}  // namespace

int wdgs_alloc(void** p, size_t bytes, bool zero, hipStream_t stream) {
    (void)zero; (void)stream;
    *p = nullptr;
    g.requests++;
    g.log.push_back("alloc " + std::to_string(bytes));
    if (g.requests == g.fail_at) return 3;
    *p = std::malloc(bytes ? bytes : 16);   // (never handed back to the C library while the test runs: addresses stay unique)
    g.frees[*p] = 0;
    g.bytes[*p] = bytes;
    return 0;
}
void wdgs_free(void* p) {
    g.log.push_back("free");
    if (!g.frees.count(p)) { std::printf("FAILED: free of a block that was never allocated\n"); std::exit(1); }
    g.frees[p]++;
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

using wdgs::DevMem;

static_assert(!std::is_copy_constructible<DevMem<int>>::value && !std::is_copy_assignable<DevMem<int>>::value, "DevMem must not be copyable");

struct Three { DevMem<float> a; DevMem<unsigned> b, c; };   // an op struct in miniature
static int refill(Three& t, size_t n) {   // "free all, then allocate all"
    t.a.reset(); t.b.reset(); t.c.reset();
    if (int r = t.a.alloc(n, true, nullptr)) return r;
    if (int r = t.b.alloc(n, true, nullptr)) return r;
    return t.c.alloc(n, true, nullptr);
}
static bool empty_or_valid(const DevMem<unsigned>& m, size_t n) { return (!m && m.get() == nullptr && m.count() == 0) || (m && m.get() != nullptr && m.count() == n); }

int main() {
    {   // empty by default; destruction of an empty handle frees nothing
        DevMem<int> m;
        CHECK(!m && m.get() == nullptr && m.count() == 0);
        m.reset();
    }
    CHECK(g.requests == 0 && g.log.empty());

    {   // alloc records the count and asks for count * sizeof(T) bytes; the destructor frees
        DevMem<double> m;
        CHECK(m.alloc(5, true, nullptr) == 0);
        CHECK(m && m.count() == 5 && g.bytes[m.get()] == 40);
        double* raw = m;   // the implicit conversion kernel launch lines rely on
        CHECK(raw == m.get());
        CHECK(m + 2 == m.get() + 2);
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    {   // a request for no elements still yields a block (wdgs_alloc's rule), with count() == 0
        DevMem<char> m;
        CHECK(m.alloc(0, false, nullptr) == 0);
        CHECK(m && m.count() == 0 && g.bytes[m.get()] == 0);
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    {   // reset frees once, and the destructor not again
        DevMem<int> m;
        CHECK(m.alloc(3, false, nullptr) == 0);
        m.reset();
        CHECK(!m && m.count() == 0 && g.live() == 0);
        m.reset();
    }
    CHECK(g.each_freed_once());

    {   // alloc on a full handle frees the old block BEFORE it requests the new one
        DevMem<int> m;
        CHECK(m.alloc(4, false, nullptr) == 0);
        int* first = m;
        g.log.clear();
        CHECK(m.alloc(8, false, nullptr) == 0);
        CHECK(g.log.size() == 2 && g.log[0] == "free" && g.log[1] == "alloc 32");
        CHECK(g.frees[first] == 1 && m.count() == 8 && g.frees[m.get()] == 0);
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    {   // move construction: the source is left empty, nothing is freed until the target goes
        DevMem<int> a;
        CHECK(a.alloc(4, false, nullptr) == 0);
        int* block = a;
        DevMem<int> b(std::move(a));
        CHECK(!a && a.count() == 0 && b.get() == block && b.count() == 4 && g.frees[block] == 0);
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    {   // move assignment onto a full handle frees the target's old block, once; self-move changes nothing
        DevMem<int> a, b;
        CHECK(a.alloc(4, false, nullptr) == 0 && b.alloc(6, false, nullptr) == 0);
        int *pa = a, *pb = b;
        b = std::move(a);
        CHECK(g.frees[pb] == 1 && g.frees[pa] == 0 && b.get() == pa && b.count() == 4 && !a && a.count() == 0);
        DevMem<int>& self = b;
        b = std::move(self);
        CHECK(b.get() == pa && b.count() == 4 && g.frees[pa] == 0);
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    {   // a failed alloc leaves the handle empty -- the old block is gone, pointer and count say so -- and the same request asks for memory again
        DevMem<int> m;
        CHECK(m.alloc(4, false, nullptr) == 0);
        int* old = m;
        g.fail_at = g.requests + 1;
        CHECK(m.alloc(16, false, nullptr) == 3);
        CHECK(!m && m.get() == nullptr && m.count() == 0 && g.frees[old] == 1);
        const int before = g.requests;
        CHECK(m.alloc(16, false, nullptr) == 0);
        CHECK(g.requests == before + 1 && m && m.count() == 16);
        g.fail_at = 0;
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    {   // release hands the block out without freeing it; adopt takes one in (freeing what the handle held), and frees it in the end
        DevMem<int> a, b;
        CHECK(a.alloc(4, false, nullptr) == 0 && b.alloc(2, false, nullptr) == 0);
        int *pa = a, *pb = b;
        int* out = a.release();
        CHECK(out == pa && !a && a.count() == 0 && g.frees[pa] == 0);
        b.adopt(out, 4);
        CHECK(g.frees[pb] == 1 && g.frees[pa] == 0 && b.get() == pa && b.count() == 4);
    }
    CHECK(g.live() == 0 && g.each_freed_once());
    {   // ... and a released block that nobody adopts stays the caller's
        DevMem<int> a;
        CHECK(a.alloc(4, false, nullptr) == 0);
        int* out = a.release();
        { DevMem<int> gone(std::move(a)); }
        CHECK(g.frees[out] == 0);
        wdgs_free(out);
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    {   // three handles filled with "reset all, then allocate all", the second allocation failing: each is empty or valid, nothing leaks
        Three t;
        CHECK(refill(t, 10) == 0);
        CHECK(t.a.count() == 10 && t.b.count() == 10 && t.c.count() == 10);
        g.log.clear();
        g.fail_at = g.requests + 2;
        CHECK(refill(t, 20) == 3);
        g.fail_at = 0;
        CHECK(g.log.size() == 5 && g.log[0] == "free" && g.log[1] == "free" && g.log[2] == "free" && g.log[3] == "alloc 80" && g.log[4] == "alloc 80");
        CHECK(t.a && t.a.count() == 20);
        CHECK(!t.b && t.b.count() == 0 && !t.c && t.c.count() == 0);
        CHECK(empty_or_valid(t.b, 20) && empty_or_valid(t.c, 20));
        CHECK(g.live() == 1);
        CHECK(refill(t, 20) == 0);   // the retry allocates all three again
        CHECK(t.a.count() == 20 && t.b.count() == 20 && t.c.count() == 20 && g.live() == 3);
    }
    CHECK(g.live() == 0 && g.each_freed_once());

    for (auto& kv : g.frees) std::free(kv.first);
    std::printf("devmem: ok\n");
    return 0;
}
