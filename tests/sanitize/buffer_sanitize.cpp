// The buffer owner of csrc/device_buffer.h under -fsanitize=address,undefined (tests/test_buffer_cpu.py builds and runs this
// program), over a fake allocator that records every call, aborts on a double free or a free of memory it did not hand out,
// and fails the n-th allocation on request with an out-of-memory or another error code. Every case runs for the device-like
// policy (failures split into SBMBP_ERR_NOMEM / SBMBP_ERR_HIP) and for the pinned-like one (every failure SBMBP_ERR_HIP).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../sbm-bp_amd/csrc/device_buffer.h"

static std::string last_error;
namespace sbmbp {
void set_error(const std::string &msg) { last_error = msg; }
}  // namespace sbmbp
using namespace sbmbp;

static int failures = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

struct call { char what; void *p; size_t bytes; };  // 'a' allocation, 'f' free, 'x' refused allocation

template <bool PINNED> struct fake_memory {
    static std::vector<call> &log() { static std::vector<call> l; return l; }
    static std::map<void *, size_t> &live() { static std::map<void *, size_t> m; return m; }
    static int &fail_in() { static int n = 0; return n; }    // fail the n-th allocation from now (0 = none)
    static bool &fail_oom() { static bool b = false; return b; }
    static void fail_nth(int n, bool oom) { fail_in() = n; fail_oom() = oom; }
    static alloc_status allocate(void **p, size_t bytes) {
        if (fail_in() > 0 && --fail_in() == 0) {
            log().push_back(call{'x', nullptr, bytes});
            if (fail_oom()) return alloc_status{PINNED ? SBMBP_ERR_HIP : SBMBP_ERR_NOMEM, "out of memory"};
            return alloc_status{SBMBP_ERR_HIP, "invalid value"};
        }
        *p = std::malloc(bytes);
        if (!*p) std::abort();
        live()[*p] = bytes;
        log().push_back(call{'a', *p, bytes});
        return alloc_status{SBMBP_OK, "no error"};
    }
    static void release(void *p) {
        auto it = live().find(p);
        if (it == live().end()) { std::fprintf(stderr, "fake_memory: free of %p, which is not live\n", p); std::abort(); }
        log().push_back(call{'f', p, it->second});
        live().erase(it);
        std::free(p);
    }
    static const char *name() { return PINNED ? "fakeHostMalloc" : "fakeMalloc"; }
    static size_t live_bytes() { size_t s = 0; for (auto &kv : live()) s += kv.second; return s; }
};

template <bool PINNED> void cases() {
    typedef fake_memory<PINNED> mem;
    typedef buffer<double, mem> buf;
    auto &log = mem::log();
    const int nomem = PINNED ? SBMBP_ERR_HIP : SBMBP_ERR_NOMEM;

    {  // alloc: max(n, 1) * sizeof(T) bytes, the account moves by exactly that, and back at the end
        uint64_t acct = 1000;
        {
            buf a, b;
            EXPECT(!a && a.capacity() == 0 && !a.owns());
            EXPECT(a.alloc(0, &acct) == SBMBP_OK && a && a.owns() && a.capacity() == 0);
            EXPECT(log.back().what == 'a' && log.back().bytes == 8 && acct == 1008);
            EXPECT(b.alloc(37, &acct) == SBMBP_OK && b.capacity() == 37);
            EXPECT(log.back().bytes == 37 * 8 && acct == 1008 + 37 * 8);
            b[36] = 1.0;  // (the last element is the buffer's: the sanitizer watches)
            EXPECT(b.get() == static_cast<double *>(b) && b + 1 == b.get() + 1);
            EXPECT(a.alloc(5, &acct) == SBMBP_OK);  // alloc over an owned buffer releases it first
            EXPECT(log[log.size() - 2].what == 'f' && log.back().what == 'a' && acct == 1000 + 5 * 8 + 37 * 8);
        }
        EXPECT(acct == 1000 && mem::live().empty());
    }
    {  // ensure: no call within the capacity; beyond it one free, then one allocation; the account ends at the new size
        uint64_t acct = 0;
        buf a;
        EXPECT(a.ensure(0, &acct) == SBMBP_OK && !a && acct == 0);  // nothing asked for, nothing held
        EXPECT(a.ensure(10, &acct) == SBMBP_OK && acct == 80);
        const size_t n0 = log.size();
        double *p0 = a;
        EXPECT(a.ensure(10, &acct) == SBMBP_OK && a.ensure(3, &acct) == SBMBP_OK && a.ensure(0) == SBMBP_OK);
        EXPECT(log.size() == n0 && a.get() == p0 && acct == 80);
        EXPECT(a.ensure(11, &acct) == SBMBP_OK);
        EXPECT(log.size() == n0 + 2 && log[n0].what == 'f' && log[n0].p == p0 && log[n0].bytes == 80 && log[n0 + 1].what == 'a' && log[n0 + 1].bytes == 88);
        EXPECT(acct == 88 && a.capacity() == 11);
        // a failing ensure: empty, capacity 0, the account reduced by the old size
        mem::fail_nth(1, true);
        EXPECT(a.ensure(12, &acct) == nomem);
        EXPECT(!a && a.capacity() == 0 && !a.owns() && acct == 0 && mem::live().empty());
        EXPECT(a.ensure(12, &acct) == SBMBP_OK && acct == 96);  // and the next call starts over
    }
    {  // replace: a failure leaves the old buffer and the account; a success frees the old one exactly once
        uint64_t acct = 0;
        buf a;
        EXPECT(a.alloc(4, &acct) == SBMBP_OK);
        double *p0 = a;
        a[3] = 7.0;
        mem::fail_nth(1, false);
        const size_t n0 = log.size();
        EXPECT(a.replace(9, &acct) == SBMBP_ERR_HIP);
        EXPECT(a.get() == p0 && a[3] == 7.0 && a.capacity() == 4 && acct == 32 && log.size() == n0 + 1 && log.back().what == 'x');
        EXPECT(a.replace(9, &acct) == SBMBP_OK);
        EXPECT(log.size() == n0 + 3 && log[n0 + 1].what == 'a' && log[n0 + 2].what == 'f' && log[n0 + 2].p == p0);  // new first, then the old goes
        EXPECT(a.get() != p0 && a.capacity() == 9 && acct == 72);
        // the same by hand, as the prior tables of a batch do it: allocate locals, then move-assign
        buf fresh;
        EXPECT(fresh.alloc(2, &acct) == SBMBP_OK && acct == 72 + 16);
        double *p1 = a;
        a = std::move(fresh);
        EXPECT(log.back().what == 'f' && log.back().p == p1 && acct == 16 && !fresh && !fresh.owns());
    }
    {  // borrow: never freed, never accounted; over an owned buffer it releases that buffer first
        uint64_t acct = 0;
        double theirs[4] = {0, 0, 0, 0};
        const size_t n0 = log.size();
        {
            buf v;
            v.borrow(theirs + 1);
            EXPECT(v.get() == theirs + 1 && !v.owns() && v.capacity() == 0);
            v.borrow(theirs);
            v.reset();
            EXPECT(!v);
            v.borrow(theirs);
            buf w(std::move(v));  // a moved borrow is still a borrow
            EXPECT(!v && w.get() == theirs && !w.owns());
        }
        EXPECT(log.size() == n0 && acct == 0);
        buf a;
        EXPECT(a.alloc(6, &acct) == SBMBP_OK && acct == 48);
        double *p0 = a;
        a.borrow(theirs);
        EXPECT(log.back().what == 'f' && log.back().p == p0 && acct == 0 && a.get() == theirs && !a.owns());
        EXPECT(a.ensure(2, &acct) == SBMBP_OK && a.owns() && a.get() != theirs && acct == 16);  // growing a view makes an owner; theirs stays
    }
    {  // move empties the source; the account travels with the memory
        uint64_t acct = 0;
        buf a;
        EXPECT(a.alloc(3, &acct) == SBMBP_OK);
        double *p0 = a;
        buf b(std::move(a));
        EXPECT(!a && a.capacity() == 0 && !a.owns() && b.get() == p0 && b.capacity() == 3 && acct == 24);
        a = std::move(b);
        EXPECT(!b && a.get() == p0 && acct == 24);
        a = std::move(a);  // self-assignment keeps it
        EXPECT(a.get() == p0 && acct == 24);
        a.reset();
        a.reset();
        EXPECT(acct == 0);
    }
    {  // unaccounted buffers touch no counter
        uint64_t acct = 5;
        buf a;
        EXPECT(a.alloc(8) == SBMBP_OK && a.ensure(80) == SBMBP_OK && a.replace(3) == SBMBP_OK);
        a.reset();
        EXPECT(acct == 5);
    }
    {  // failure codes, and the byte count in the text
        buf a;
        mem::fail_nth(1, true);
        EXPECT(a.alloc(1000) == nomem);
        EXPECT(last_error == std::string(mem::name()) + "(8000 B): out of memory");
        mem::fail_nth(1, false);
        EXPECT(a.alloc(0) == SBMBP_ERR_HIP);
        EXPECT(last_error == std::string(mem::name()) + "(8 B): invalid value");
        EXPECT(!a && mem::live().empty());
    }
    {  // a struct of several buffers destroyed after a failure half way: every allocation freed exactly once, the account at 0
        uint64_t acct = 0;
        const size_t n0 = log.size();
        struct engine_like {
            buf a, b[2], c;
            buffer<int, mem> d;
        };
        {
            engine_like e;
            auto build = [&]() -> int {
                int r;
                if ((r = e.a.alloc(10, &acct)) != SBMBP_OK) return r;
                if ((r = e.b[0].alloc(20, &acct)) != SBMBP_OK) return r;
                if ((r = e.b[1].alloc(30, &acct)) != SBMBP_OK) return r;  // this one fails
                if ((r = e.c.alloc(40, &acct)) != SBMBP_OK) return r;
                return e.d.alloc(50, &acct);
            };
            mem::fail_nth(3, true);
            EXPECT(build() == nomem && acct == 240 && mem::live().size() == 2);
        }
        EXPECT(acct == 0 && mem::live().empty());
        size_t na = 0, nf = 0;
        for (size_t i = n0; i < log.size(); ++i) { na += log[i].what == 'a'; nf += log[i].what == 'f'; }
        EXPECT(na == 2 && nf == 2);
    }
    EXPECT(mem::live().empty() && mem::live_bytes() == 0);
}

int main() {
    cases<false>();
    cases<true>();
    // at exit the fakes hold nothing, and every allocation they recorded has its one free
    for (int pinned = 0; pinned < 2; ++pinned) {
        const std::vector<call> &log = pinned ? fake_memory<true>::log() : fake_memory<false>::log();
        size_t na = 0, nf = 0;
        for (const call &c : log) { na += c.what == 'a'; nf += c.what == 'f'; }
        EXPECT(na == nf && na > 0);
    }
    EXPECT(fake_memory<false>::live().empty() && fake_memory<true>::live().empty());
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("buffer_sanitize ok\n");
    return 0;
}
